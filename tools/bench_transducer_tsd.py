#!/usr/bin/env python3
"""Batched time-synchronous transducer beam search (BeamSearchTransducer.tsd_batch, csrc/rnnt_tsd.hip) at the width of BASELINE
config 5 as tools/bench_transducer_greedy.py builds it: encoder states of T' = 374 frames x 256, one LSTM layer of 512 units behind
a 512-wide embedding, joint space 320, |V| = 5000, max_sym_exp 2; beams 4 and 8; B = 1, 16 and 32 utterances per call.  Weights are
seeded; lin_out's bias at blank is set by bisection so that the greedy search emits about `--tokens` labels per utterance (config 5
trains on 100 labels per 374 frames).

  batched   median over `--iters` calls of tsd_batch (host clock around calls that end in their one device-to-host copy), utt/s and
            the time per pass (T x max_sym_exp passes per call)
  per_utt   B calls of the per-utterance tsd search (BeamSearchTransducer.__call__, search_type "tsd") on the same states, timed the
            same way, with its passes and blocking host reads per utterance

Both return the same n-best sequences, which is asserted for every utterance of every configuration.

Launches per pass come from a profiler run of its own:
  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_transducer_tsd.py --trace 2 --trace-beam 4
  python tools/bench_transducer_tsd.py --launches DIR --trace 2 --out profiles/transducer_tsd_bench.json
(--trace N: only N tsd_batch calls at B = 16, nothing timed; --launches: kernel dispatches of that run / (N x passes), the set-up
- seeded weights, encoder projection, buffer fills, the initial prediction step - included, merged into the JSON of an earlier run).

Usage: python tools/bench_transducer_tsd.py [--iters 12] [--out profiles/transducer_tsd_bench.json]"""
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


def bench(a):
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    dec, g, tokens = decoder(a)
    passes = a.T * a.max_sym_exp
    res = dict(greedy_tokens_per_utt=tokens, passes_per_call=passes)
    states = {B: torch.randn(B, a.T, 256, generator=g).to(DEV) for B in (1, 16, 32)}
    for beam in (4, 8):
        search = BeamSearchTransducer(decoder=dec, beam_size=beam, search_type="tsd", max_sym_exp=a.max_sym_exp)
        for B, hs in states.items():
            want = search.tsd_batch(hs)
            one = [search(hs[b]) for b in range(B)]
            assert [[h.yseq for h in nb] for nb in want] == [[h.yseq for h in nb] for nb in one], "n-best sequences differ"
            n_pass, reads = search.passes, search.host_reads
            t_b = wall(lambda: search.tsd_batch(hs), a.iters, warm=2)
            t_u = wall(lambda: [search(hs[b]) for b in range(B)], a.per_utt_iters, warm=0)
            res["beam%d_B%d" % (beam, B)] = dict(
                batched=dict(utt_per_s=B / t_b, call_ms=t_b * 1e3, pass_us=t_b * 1e6 / passes, rows=B * min(beam, a.V)),
                per_utt=dict(utt_per_s=B / t_u, call_ms=t_u * 1e3, ms_per_utt=t_u * 1e3 / B, passes=n_pass, host_reads=reads),
                speedup=t_u / t_b, nbest=len(want[0]), best_len=len(want[0][0].yseq) - 1, same_nbest_as_per_utt=True)
            print("beam %d B %d: batched %.1f ms, per-utterance %.1f ms" % (beam, B, t_b * 1e3, t_u * 1e3), file=sys.stderr, flush=True)
    return res


def trace(a):
    """a.trace calls of tsd_batch at B = 16, nothing timed: the process a kernel trace is taken of.  The blank bias is not
    calibrated here (that would run the greedy search in the traced process): the launches of a pass do not depend on the data"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    dec, g, _ = decoder(a, calibrated=False)
    hs = torch.randn(16, a.T, 256, generator=g).to(DEV)
    search = BeamSearchTransducer(decoder=dec, beam_size=a.trace_beam, search_type="tsd", max_sym_exp=a.max_sym_exp)
    for _ in range(a.trace):
        search.tsd_batch(hs)
    torch.cuda.synchronize()


def launches(a):
    """kernel dispatches per pass from the kernel statistics of a traced --trace run"""
    files = glob.glob(os.path.join(a.launches, "**", "*kernel_stats.csv"), recursive=True)
    assert files, "no kernel statistics under %s" % a.launches
    n = sum(int(row["Calls"]) for f in files for row in csv.DictReader(open(f)))
    passes = a.T * a.max_sym_exp
    return dict(calls=a.trace, beam=a.trace_beam, B=16, kernel_dispatches=n, launches_per_pass=n / (a.trace * passes),
                includes="the process's set-up: seeded weights, encoder projection, buffer fills, the initial prediction step, the "
                         "result's concatenation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--per-utt-iters", dest="per_utt_iters", type=int, default=3)
    ap.add_argument("--T", type=int, default=374)
    ap.add_argument("--V", type=int, default=5000)
    ap.add_argument("--max-sym-exp", dest="max_sym_exp", type=int, default=2)
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
        res["launches"] = launches(a)
    else:
        assert torch.cuda.is_available(), "the benchmark measures the GPU"
        import espnet_amd
        espnet_amd.set_precision("fp32")
        if a.trace is not None:
            trace(a)
            return
        res.update(dict(T=a.T, V=a.V, D_enc=256, dunits=512, embed=512, joint=320, max_sym_exp=a.max_sym_exp, iters=a.iters,
                        per_utt_iters=a.per_utt_iters))
        res.update(bench(a))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
