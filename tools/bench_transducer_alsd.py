#!/usr/bin/env python3
"""Batched alignment-length-synchronous transducer beam search (BeamSearchTransducer.alsd_batch, csrc/rnnt_alsd.hip) at the width
of BASELINE config 5 as tools/bench_transducer_greedy.py builds it: encoder states of T' = 374 frames x 256, one LSTM layer of 512
units behind a 512-wide embedding, joint space 320, |V| = 5000, u_max 50; beams 4 and 8; B = 1, 16 and 32 utterances per call.
Weights are seeded; lin_out's bias at blank is set by bisection so that the greedy search emits about `--tokens` labels per
utterance (config 5 trains on 100 labels per 374 frames).

  batched   median over `--iters` calls of alsd_batch (host clock around calls that end in their one device-to-host copy), utt/s and
            the time per step (T + min(u_max, T - 1) steps per call)
  per_utt   B calls of the per-utterance alsd search (BeamSearchTransducer.__call__, search_type "alsd") on the same states, timed
            the same way, with its passes and blocking host reads per utterance

Launches per step come from a profiler run of its own:
  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_transducer_alsd.py --trace 2 --trace-beam 4
  python tools/bench_transducer_alsd.py --launches DIR --trace 2 --out profiles/transducer_alsd_bench.json
(--trace N: only N alsd_batch calls at B = 16, nothing timed; --launches: kernel dispatches of that run / (N x steps), the set-up
- seeded weights, encoder projection, buffer fills, the initial prediction step - included, merged into the JSON of an earlier run).

Usage: python tools/bench_transducer_alsd.py [--iters 12] [--out profiles/transducer_alsd_bench.json]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_transducer_greedy import calibrate, median      # noqa: E402

DEV = "cuda"


def wall(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return median(ts)


def decoder(a, calibrated=True):
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    from espnet_amd.nets.transducer.rnn_decoder import DecoderRNNT
    torch.manual_seed(0)
    dec = DecoderRNNT(256, a.V, "lstm", 1, 512, 0, 512, 320, "tanh").to(DEV).eval()
    with torch.no_grad():
        dec.embed.weight.normal_(0, 1)
        dec.embed.weight[0].zero_()
        dec.joint_network.lin_out.weight.normal_(0, 2.0 / 320 ** 0.5)
    g = torch.Generator().manual_seed(1)
    hs16 = torch.randn(16, a.T, 256, generator=g).to(DEV)
    tokens = None
    if calibrated:
        tokens = calibrate(BeamSearchTransducer(decoder=dec, beam_size=1), dec.joint_network.lin_out, hs16, a.tokens)
    return dec, g, tokens


def bench(a):
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    dec, g, tokens = decoder(a)
    steps = a.T + min(a.u_max, a.T - 1)
    res = dict(greedy_tokens_per_utt=tokens, steps_per_call=steps)
    states = {B: torch.randn(B, a.T, 256, generator=g).to(DEV) for B in (1, 16, 32)}
    for beam in (4, 8):
        search = BeamSearchTransducer(decoder=dec, beam_size=beam, search_type="alsd", u_max=a.u_max)
        for B, hs in states.items():
            want = search.alsd_batch(hs)
            one = search(hs[0])
            same = [h.yseq for h in one] == [h.yseq for h in want[0]]      # seeded weights: float32 may order a near-tie differently
            passes, reads = search.passes, search.host_reads
            t_b = wall(lambda: search.alsd_batch(hs), a.iters, warm=2)
            t_u = wall(lambda: [search(hs[b]) for b in range(B)], a.iters, warm=1)
            res["beam%d_B%d" % (beam, B)] = dict(
                batched=dict(utt_per_s=B / t_b, call_ms=t_b * 1e3, step_us=t_b * 1e6 / steps, rows=B * min(beam, a.V)),
                per_utt=dict(utt_per_s=B / t_u, call_ms=t_u * 1e3, ms_per_utt=t_u * 1e3 / B, passes=passes, host_reads=reads),
                speedup=t_u / t_b, nbest=len(want[0]), best_len=len(want[0][0].yseq) - 1, same_nbest_as_per_utt=same)
            print("beam %d B %d: batched %.1f ms, per-utterance %.1f ms" % (beam, B, t_b * 1e3, t_u * 1e3), file=sys.stderr, flush=True)
    return res


def trace(a):
    """a.trace calls of alsd_batch at B = 16, nothing timed: the process a kernel trace is taken of.  The blank bias is not
    calibrated here (that would run the greedy search in the traced process): the launches of a step do not depend on the data"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    dec, g, _ = decoder(a, calibrated=False)
    hs = torch.randn(16, a.T, 256, generator=g).to(DEV)
    search = BeamSearchTransducer(decoder=dec, beam_size=a.trace_beam, search_type="alsd", u_max=a.u_max)
    for _ in range(a.trace):
        search.alsd_batch(hs)
    torch.cuda.synchronize()


def launches(a):
    """kernel dispatches per step from the kernel statistics of a traced --trace run"""
    files = glob.glob(os.path.join(a.launches, "**", "*kernel_stats.csv"), recursive=True)
    assert files, "no kernel statistics under %s" % a.launches
    n = sum(int(row["Calls"]) for f in files for row in csv.DictReader(open(f)))
    steps = a.T + min(a.u_max, a.T - 1)
    return dict(calls=a.trace, beam=a.trace_beam, B=16, kernel_dispatches=n, launches_per_step=n / (a.trace * steps),
                includes="the process's set-up: seeded weights, encoder projection, buffer fills, the initial prediction step, the "
                         "result's concatenation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--T", type=int, default=374)
    ap.add_argument("--V", type=int, default=5000)
    ap.add_argument("--u-max", dest="u_max", type=int, default=50)
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
        res.update(dict(T=a.T, V=a.V, D_enc=256, dunits=512, embed=512, joint=320, u_max=a.u_max, iters=a.iters))
        res.update(bench(a))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
