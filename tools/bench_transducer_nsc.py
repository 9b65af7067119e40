#!/usr/bin/env python3
"""Batched N-step constrained transducer beam search (BeamSearchTransducer.nsc_batch, csrc/rnnt_nsc.hip) at the width of BASELINE
config 5 as tools/bench_transducer_greedy.py builds it: encoder states of T' = 374 frames x 256, one LSTM layer of 512 units behind
a 512-wide embedding, joint space 320, |V| = 5000; (nstep, prefix_alpha) = (1, 1) and (2, 1); beams 4 and 8; B = 16 and 32
utterances per call.  Weights are seeded; lin_out's bias at blank is set by bisection so that the greedy search emits about
`--tokens` labels per utterance (config 5 trains on 100 labels per 374 frames).

  batched   median over `--iters` calls of nsc_batch (host clock around calls that end in their one device-to-host copy), utt/s and
            the time per frame (T frames per call, each of nstep expansions and, when nstep > 1, the pass of the last blank term)
  per_utt   B calls of the per-utterance nsc search (BeamSearchTransducer.__call__, search_type "nsc") of the same search object on
            the same states, timed the same way, with its passes and blocking host reads per utterance

The number of utterances whose n-best sequences are the same both ways is reported per configuration (seeded weights: float32 may
order a near-tie differently; tests/test_gpu_rnnt_nsc.py compares the two where no decision is that close).

Launches per frame come from a profiler run of its own, per (nstep, prefix_alpha):
  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_transducer_nsc.py --trace 2 --nstep 2
  python tools/bench_transducer_nsc.py --launches DIR --trace 2 --nstep 2 --out profiles/transducer_nsc_bench.json
(--trace N: only N nsc_batch calls at B = 16, nothing timed; --launches: kernel dispatches of that run / (N x frames), the set-up
- seeded weights, encoder projection, buffer fills, the initial prediction step - included, merged into the JSON of an earlier run).

Usage: python tools/bench_transducer_nsc.py [--iters 12] [--out profiles/transducer_nsc_bench.json]"""
import argparse
import csv
import glob
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_transducer_alsd import decoder, wall      # noqa: E402

DEV = "cuda"
CONFIGS = ((1, 1), (2, 1))                          # (nstep, prefix_alpha)


def bench(a):
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    dec, g, tokens = decoder(a)
    res = dict(greedy_tokens_per_utt=tokens, frames_per_call=a.T)
    states = {B: torch.randn(B, a.T, 256, generator=g).to(DEV) for B in (16, 32)}
    for nstep, alpha in CONFIGS:
        for beam in (4, 8):
            search = BeamSearchTransducer(decoder=dec, beam_size=beam, search_type="nsc", nstep=nstep, prefix_alpha=alpha)
            for B, hs in states.items():
                want = search.nsc_batch(hs)
                one = [search(hs[b]) for b in range(B)]
                same = sum([h.yseq for h in x] == [h.yseq for h in y] for x, y in zip(want, one))
                n_pass, reads = search.passes, search.host_reads
                t_b = wall(lambda: search.nsc_batch(hs), a.iters, warm=2)
                t_u = wall(lambda: [search(hs[b]) for b in range(B)], a.per_utt_iters, warm=0)
                res["nstep%d_alpha%d_beam%d_B%d" % (nstep, alpha, beam, B)] = dict(
                    batched=dict(utt_per_s=B / t_b, call_ms=t_b * 1e3, frame_us=t_b * 1e6 / a.T, rows=B * min(beam, a.V)),
                    per_utt=dict(utt_per_s=B / t_u, call_ms=t_u * 1e3, ms_per_utt=t_u * 1e3 / B, passes=n_pass, host_reads=reads),
                    speedup=t_u / t_b, nbest=len(want[0]), best_len=len(want[0][0].yseq) - 1, same_nbest_as_per_utt=same)
                print("nstep %d alpha %d beam %d B %d: batched %.1f ms, per-utterance %.1f ms"
                      % (nstep, alpha, beam, B, t_b * 1e3, t_u * 1e3), file=sys.stderr, flush=True)
    return res


def trace(a):
    """a.trace calls of nsc_batch at B = 16, nothing timed: the process a kernel trace is taken of.  The blank bias is not
    calibrated here (that would run the greedy search in the traced process): the launches of a frame do not depend on the data"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    dec, g, _ = decoder(a, calibrated=False)
    hs = torch.randn(16, a.T, 256, generator=g).to(DEV)
    search = BeamSearchTransducer(decoder=dec, beam_size=a.trace_beam, search_type="nsc", nstep=a.nstep, prefix_alpha=a.prefix_alpha)
    for _ in range(a.trace):
        search.nsc_batch(hs)
    torch.cuda.synchronize()


def launches(a):
    """kernel dispatches per frame from the kernel statistics of a traced --trace run"""
    files = glob.glob(os.path.join(a.launches, "**", "*kernel_stats.csv"), recursive=True)
    assert files, "no kernel statistics under %s" % a.launches
    n = sum(int(row["Calls"]) for f in files for row in csv.DictReader(open(f)))
    return dict(calls=a.trace, beam=a.trace_beam, B=16, nstep=a.nstep, prefix_alpha=a.prefix_alpha, kernel_dispatches=n,
                launches_per_frame=n / (a.trace * a.T),
                includes="the process's set-up: seeded weights, encoder projection, buffer fills, the initial prediction step, the "
                         "result's concatenation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--per-utt-iters", dest="per_utt_iters", type=int, default=1)
    ap.add_argument("--T", type=int, default=374)
    ap.add_argument("--V", type=int, default=5000)
    ap.add_argument("--nstep", type=int, default=2, help="--trace / --launches only")
    ap.add_argument("--prefix-alpha", dest="prefix_alpha", type=int, default=1, help="--trace / --launches only")
    ap.add_argument("--tokens", type=float, default=100.0)
    ap.add_argument("--trace", type=int, default=None)
    ap.add_argument("--trace-beam", type=int, default=4)
    ap.add_argument("--launches", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))
    if a.launches:
        res["launches_nstep%d_alpha%d" % (a.nstep, a.prefix_alpha)] = launches(a)
    else:
        assert torch.cuda.is_available(), "the benchmark measures the GPU"
        import espnet_amd
        espnet_amd.set_precision("fp32")
        if a.trace is not None:
            trace(a)
            return
        res.update(dict(T=a.T, V=a.V, D_enc=256, dunits=512, embed=512, joint=320, configs=[list(c) for c in CONFIGS], iters=a.iters,
                        per_utt_iters=a.per_utt_iters))
        res.update(bench(a))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
