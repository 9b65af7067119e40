#!/usr/bin/env python3
"""Batched default (Graves A / B) transducer beam search (BeamSearchTransducer.default_batch, csrc/rnnt_default.hip) at the width of
BASELINE config 5 as tools/bench_transducer_greedy.py builds it: encoder states of T' = 374 frames x 256, one LSTM layer of 512
units behind a 512-wide embedding, joint space 320, |V| = 5000; beams 4 and 8; B = 16 and 32 utterances per call.

Weights: seeded, as in tools/bench_transducer_alsd.py; lin_out's bias at blank is set by bisection so that the greedy search emits
about `--tokens` labels per utterance (config 5 trains on 100 labels per 374 frames), and every value of `--blank-extra` is then added
to it, one model per value.  The pops a frame takes depend on how peaked the model is: a seeded model is far flatter than a trained
one, and the extra bias stands in for training.  Nobody has run this on trained weights; the JSON says which weights it used.

  batched   median over `--iters` calls of default_batch (host clock around calls that end in their result copy): utt/s, the time
            per step (a step is one pop of every utterance; null when an utterance overflowed, because the call then holds the
            per-utterance searches of the overflowed ones as well), the steps enqueued, the reads of the done flags, the utterances
            that overflowed (and were searched again per utterance INSIDE the timed call), and the pops per frame the device
            counted, as mean and maximum over W = min(beam, V)
  per_utt   the per-utterance default search (BeamSearchTransducer.__call__) of the same search object on the first `--per-utt`
            utterances of the same states: median over `--per-utt-iters` rounds after one warm-up round

Usage: python tools/bench_transducer_default.py [--iters 5] [--out profiles/transducer_default_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_transducer_alsd import decoder, wall      # noqa: E402

DEV = "cuda"


def bench(a):
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    dec, g, tokens = decoder(a)
    res = dict(greedy_tokens_per_utt=tokens, frames_per_call=a.T,
               weights="seeded (torch.manual_seed(0): embedding N(0, 1), lin_out N(0, 2 / sqrt(320)), the rest as initialised); blank "
                       "bias calibrated to the greedy token count, plus blank_extra")
    states = {B: torch.randn(B, a.T, 256, generator=g).to(DEV) for B in a.B}
    bias = dec.joint_network.lin_out.bias
    base = float(bias.detach()[0])
    for extra in a.blank_extra:
        with torch.no_grad():
            bias[0] = base + extra
        for beam in a.beams:
            search = BeamSearchTransducer(decoder=dec, beam_size=beam)
            W = min(beam, a.V)
            for B, hs in states.items():
                want = search.default_batch(hs)
                passes, reads, over, pops = search.passes, search.host_reads, len(search.overflowed), list(search.pops)
                m = min(B, a.per_utt)
                one = [search(hs[b]) for b in range(m)]
                same = sum([h.yseq for h in x] == [h.yseq for h in y] for x, y in zip(want, one))
                t_b = wall(lambda: search.default_batch(hs), a.iters, warm=1)
                t_u = wall(lambda: [search(hs[b]) for b in range(m)], a.per_utt_iters, warm=1)
                frames = sum(p[1] for p in pops)
                res["extra%g_beam%d_B%d" % (extra, beam, B)] = dict(
                    batched=dict(utt_per_s=B / t_b, call_ms=t_b * 1e3, step_us=None if over else t_b * 1e6 / max(passes, 1), steps=passes,
                                 least_steps=W * a.T, done_reads=reads - 1, overflowed=over,
                                 pops_per_frame_mean_over_W=sum(p[0] for p in pops) / float(max(frames, 1)) / W,
                                 pops_per_frame_max_over_W=max(p[2] for p in pops) / float(W)),
                    per_utt=dict(utt_per_s=m / t_u, ms_per_utt=t_u * 1e3 / m, utterances=m),
                    speedup=(t_u / m) / (t_b / B), nbest=len(want[0]), best_len=len(want[0][0].yseq) - 1,
                    same_nbest_as_per_utt="%d of %d" % (same, m))
                print("extra %g beam %d B %d: batched %.1f ms (%d steps, %d overflowed), per-utterance %.1f ms each"
                      % (extra, beam, B, t_b * 1e3, passes, over, t_u * 1e3 / m), file=sys.stderr, flush=True)
    with torch.no_grad():
        bias[0] = base
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--per-utt-iters", dest="per_utt_iters", type=int, default=3)
    ap.add_argument("--per-utt", dest="per_utt", type=int, default=8, help="utterances the per-utterance search is timed on")
    ap.add_argument("--T", type=int, default=374)
    ap.add_argument("--V", type=int, default=5000)
    ap.add_argument("--B", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--beams", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--blank-extra", dest="blank_extra", type=float, nargs="+", default=[0.0, 4.0, 8.0])
    ap.add_argument("--tokens", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark measures the GPU"
    import espnet_amd
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer as S
    espnet_amd.set_precision("fp32")
    res = dict(T=a.T, V=a.V, D_enc=256, dunits=512, embed=512, joint=320, iters=a.iters, per_utt_iters=a.per_utt_iters,
               blank_extra=a.blank_extra, default_max_pops=S.default_max_pops, default_chunk_steps=S.default_chunk_steps,
               default_step_budget=S.default_step_budget, default_max_rows=S.default_max_rows)
    res.update(bench(a))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
