#!/usr/bin/env python3
"""CTC segmentation throughput at the size of a long recording: T = 90000 frames (15 minutes at 10 ms), a transcript of about
L = 50000 characters, window W = 8000, |V| = 40, for batches of 1 / 8 / 32 recordings and tokens of at most S = 1 and S = 3
characters.

  run     ops.ctc_segment_run on precomputed emission rows: one window attempt (fill, walk back, prefix sums, segments), with the
          device time of the fill and of the walk back (torch.profiler), per column
  gather  ops.ctc_segment_emissions (once per call of ctc_segment_batch)
  numpy   the float32 NumPy restatement of tests/ctc_segmentation_restatement.py for ONE recording at a TENTH of the length
          (T = 9000, L = 5000, W = 800) on the CPU, scaled per cell for comparison: an interpreted loop, not a compiled one

Usage: python tools/bench_ctc_segmentation.py [--iters 3] [--batches 1,8,32] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHARS = ["_"] + [chr(ord("a") + i) for i in range(26)]
MULTI = ["th", "he", "in", "er", "an", "the", "ing", "and"]


def recording(seed, T, L, S, V):
    """-> (text, lp [T,V] fp32): random letters in utterances of 30-60 characters, about L characters in all, and log-posteriors
    with a bump for every character at evenly drawn frames, so that the window has a path to follow"""
    from espnet_amd.nets.ctc_segmentation import CtcSegmentationParameters, prepare_text
    rng = np.random.default_rng(seed)
    text, n = [], 1
    while n < L - 61:
        k = int(rng.integers(30, 61))
        text.append("".join(rng.choice(CHARS[1:], k)) + "\n")
        n += k + 1
    cfg = CtcSegmentationParameters(char_list=CHARS + (MULTI if S == 3 else []))
    gt, _ = prepare_text(cfg, text)
    pos = np.sort(rng.choice(np.arange(3, T - 3), gt.shape[0] - 1, replace=False))
    z = rng.normal(0, 2, (T, V)).astype(np.float32)
    z[:, 0] += 4
    z[pos, gt[1:, 0]] += 8
    return text, torch.log_softmax(torch.from_numpy(z), -1).numpy()


def kernel_us(fn, keys, reps=2):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        for key in keys:
            if key in ev.key:
                us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
                out[key] = out.get(key, 0.0) + us / reps
    return out


def bench(B, T, L, S, W, V, iters):
    from espnet_amd import ops
    from espnet_amd.nets.ctc_segmentation import CtcSegmentationParameters, _plan, prepare_text
    dev = "cuda:0"
    cfg = CtcSegmentationParameters(char_list=CHARS + (MULTI if S == 3 else []), min_window_size=W)
    text, lp = recording(0, T, L, S, V)
    gt, begins = prepare_text(cfg, text)
    tok, gtu, llens, utt, nutt = _plan(cfg, [T] * B, [gt] * B, [begins] * B, V, 1 << 40)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lpz = up(lp)[None].expand(B, T, V).contiguous()
    lens_d, tok_d, gtu_d, llens_d, utt_d, nutt_d = (up(x) for x in (np.full(B, T, np.int32), tok, gtu, llens, utt, nutt))
    sel = torch.arange(B, dtype=torch.int32, device=dev)
    Lc, Sg = gtu.shape[1], gtu.shape[2]
    res = ops.ctc_segment_result(B, T, Lc, utt.shape[1] - 1, dev)
    ws = torch.empty(ops.ctc_segment_workspace_layout(B, B, T, Lc, Sg, W)[3], dtype=torch.uint8, device=dev)
    gather = lambda: ops.ctc_segment_emissions(lpz, lens_d, tok_d, 0, False)
    em = gather()
    run = lambda: ops.ctc_segment_run(em, gtu_d, tok_d, lens_d, llens_d, sel, utt_d, nutt_d, res, W, 30, 0.01, workspace=ws)
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        run()
    torch.cuda.synchronize()
    t_run = (time.perf_counter() - t0) / iters
    t0 = time.perf_counter()
    gather()
    torch.cuda.synchronize()
    t_gather = time.perf_counter() - t0
    status = ops.ctc_segment_fetch(res)["info"][:, 0].tolist()
    ks = kernel_us(run, ("seg_fill", "seg_backtrack", "seg_prefix", "seg_segments"), reps=1)
    out = dict(B=B, T=T, L=int(Lc), S=int(Sg), W=W, U=int(tok.shape[1]), ring_in_lds=ops.ctc_segment_ring_in_lds(Sg, W, T),
               status=sorted(set(status)), run_ms=t_run * 1e3, gather_ms=t_gather * 1e3, recordings_per_s=B / (t_run + t_gather),
               workspace_gib=ws.numel() / 2 ** 30)
    if ks:
        out["fill_us_per_column"] = ks.get("seg_fill", 0.0) / Lc
        out["backtrack_us_per_column"] = ks.get("seg_backtrack", 0.0) / Lc
        out["kernel_ms"] = {k: round(v / 1e3, 3) for k, v in ks.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--T", type=int, default=90000)
    ap.add_argument("--L", type=int, default=50000)
    ap.add_argument("--W", type=int, default=8000)
    ap.add_argument("--V", type=int, default=40)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark measures the GPU"
    for S in (1, 3):
        for B in (int(b) for b in a.batches.split(",")):
            print(json.dumps(bench(B, a.T, a.L, S, a.W, a.V, a.iters)), flush=True)
    if not a.no_numpy:
        import ctc_segmentation_restatement as R
        from espnet_amd.nets.ctc_segmentation import CtcSegmentationParameters, prepare_text
        T, L, W = a.T // 10, a.L // 10, a.W // 10
        text, lp = recording(0, T, L, 1, a.V)
        gt, _ = prepare_text(CtcSegmentationParameters(char_list=CHARS), text)
        t0 = time.perf_counter()
        r = R.trellis(lp, gt, 0, W, np.float32)
        t = time.perf_counter() - t0
        print(json.dumps(dict(numpy_tenth_length=dict(T=T, L=int(gt.shape[0]), S=1, W=W, status=int(r["status"]), seconds=t,
                                                      us_per_column=t * 1e6 / gt.shape[0], us_per_cell=t * 1e6 / (gt.shape[0] * W)))),
              flush=True)


if __name__ == "__main__":
    main()
