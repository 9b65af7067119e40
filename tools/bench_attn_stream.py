#!/usr/bin/env python
"""Times the memory-linear attention forward (csrc/attn_stream.hip, ops.attn_fwd_stream) beside the paths that store the
probabilities, for fp32 and bf16 storage, with and without relative positions, at B * H = 32 (batch, head) pairs:
at T = 4096 beside the fused long-row forward (F_.attn_fwd_fused), at T = 8192 and 22 528 (fifteen minutes of 10 ms frames behind
conv2d subsampling) beside the GEMM + softmax + GEMM composition where that fits into free device memory and its kernels
take the shape.  Writes one JSON file.  With --train: forward + backward without relative positions, the streamed pair
(F_.attn_fwd_stream with lse, F_.attn_stream_bwd: csrc/attn_stream_bwd.hip) beside today's route - the stored-P kernels at 4096
keys, GEMM + softmax in both directions beyond - into profiles/attn_stream_train_bench.json.  With --train --rel: forward +
backward of one rel-pos block (F_.attn_block_fwd / attn_block_bwd) at 8192 keys, the streamed route (csrc/attn_stream_bwd_rel.hip)
beside the GEMM + softmax route of the same code with the threshold raised, every round's span kept, into
profiles/attn_stream_train_rel_bench.json.

    python tools/bench_attn_stream.py [--train [--rel]] [--out profiles/attn_stream_bench.json] [--commit <id>] [--T 4096 8192 22528]

Times are device events around at least `iters` calls and at least 50 ms of work after `warmup` calls, the best of `rounds`
alternating rounds; peak memory is the rise of torch.cuda.max_memory_allocated over one call (operands excluded).  tflops counts
the two (three with positions) T x T x 64 products of the streamed kernel over its time."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOW_MS = 50.0


def _window(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def timed(fn, warmup, iters):
    first = _window(fn, warmup, iters)
    more = int(WINDOW_MS / max(first, 1e-4)) + 1
    return first if more <= iters else _window(fn, 0, more)


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def train_rows(args, res):
    """forward + backward, no relative positions: streamed against today's route, alternating in the same call"""
    import espnet_amd
    from espnet_amd import functional as F_, ops
    dev, B, H, dk = "cuda", args.B, args.H, 64
    D = H * dk
    for prec in ("fp32", "bf16"):
        espnet_amd.set_precision(prec)
        adt = ops.act_dtype()
        for T in args.T:
            torch.manual_seed(T)
            qkv, dctx = (torch.randn(B * T, n, device=dev).to(adt) for n in (3 * D, D))
            dqkv = torch.empty_like(qkv)
            qu, k, v = (F_._MV(qkv, i * D, 3 * D) for i in range(3))
            mask = torch.ones(B, 1, T, dtype=torch.uint8, device=dev)
            stored = ops.attn_fwd_supported(T, T, dk, False)
            drop = (args.drop, 7) if args.drop > 0.0 else None       # attention dropout: both routes draw the same mask

            def stream():
                lse = torch.empty(H * B * T, device=dev, dtype=torch.float32)
                cx = F_.attn_fwd_stream(qu, None, k, v, None, mask, B, T, T, H, dk, lse=lse, drop=drop)
                assert F_.attn_stream_bwd(dctx, cx, lse, qu, k, v, mask, B, T, T, H, dk, dqkv=dqkv, drop=drop) is not None

            def other():
                P, Pd = F_.attn_stored_fwd(qu, None, k, v, None, mask, B, T, T, H, dk, drop=drop)[:2]
                F_.attn_core_bwd(dctx, P, qu, None, k, v, None, B, T, T, H, dk, Pd=Pd if drop else None, attn_drop=drop or (0.0, 0), dqkv=dqkv)
            need = H * B * T * T * (2 * qkv.element_size() if stored else 8 if prec == "fp32" else 12) * (2 if drop else 1)
            fits = need < 0.8 * torch.cuda.mem_get_info()[0]
            row = dict(precision=prec, T=T, drop=args.drop, other="stored_p" if stored else "gemm_softmax", rounds=[], stream_peak_bytes=peak_rise(stream),
                       other_peak_bytes=None)
            try:
                if fits:
                    row["other_peak_bytes"] = peak_rise(other)
            except ops._lib.EamdError as e:          # today's route cannot run: its own kernels decline the shape
                fits, row["other_error"] = False, str(e)
            for _ in range(args.rounds):
                r = dict(stream_ms=timed(stream, args.warmup, args.iters))
                if fits:
                    r["other_ms"] = timed(other, args.warmup, args.iters)
                row["rounds"].append(r)
            row["stream_ms"] = min(r["stream_ms"] for r in row["rounds"])
            row["other_ms"] = min(r["other_ms"] for r in row["rounds"]) if fits else None
            row["stream_tflops"] = B * H * T * T * dk * 2 * 9 / (row["stream_ms"] * 1e-3) / 1e12      # 2 forward + 3 + 4 backward products
            res["rows"].append(row)
            print(json.dumps({k_: v_ for k_, v_ in row.items() if k_ != "rounds"}), flush=True)
            del qkv, dqkv, dctx, qu, k, v
            torch.cuda.empty_cache()
    espnet_amd.set_precision("fp32")


def train_rel_rows(args, res):
    """forward + backward of one rel-pos attention block through F_.attn_block_fwd / attn_block_bwd: the streamed route (threshold
    at its default) against the GEMM + softmax route the same code takes with the threshold raised, alternating"""
    import espnet_amd
    from espnet_amd import functional as F_, ops
    dev, B, H, dk = "cuda", args.B, args.H, 64
    D = H * dk
    default = F_.ATTN_STREAM_TRAIN_REL_KEYS
    for prec in ("fp32", "bf16"):
        espnet_amd.set_precision(prec)
        adt = ops.act_dtype()
        for T in args.T:
            torch.manual_seed(T)
            qkv, qu, qv, dctx, p = (torch.randn(r, n, device=dev).to(adt) for r, n in ((B * T, 3 * D), (B * T, D), (B * T, D), (B * T, D), (T, D)))
            dqkv = torch.empty_like(qkv)
            k, v = F_._MV(qkv, D, 3 * D), F_._MV(qkv, 2 * D, 3 * D)
            mask = torch.ones(B, 1, T, dtype=torch.uint8, device=dev)
            drop = (args.drop, 7)                                    # attention dropout: both routes draw the same mask

            def block(keys, route):
                F_.ATTN_STREAM_TRAIN_REL_KEYS = keys
                try:
                    cx, kept = F_.attn_block_fwd(qu, qv, k, v, p, mask, B, T, T, H, dk, drop, None, True, False, True)
                    assert kept.route == route, kept.route
                    F_.attn_block_bwd(kept, dctx, cx, qu, qv, k, v, p, B, T, T, H, dk, drop, None, dqkv=dqkv)
                finally:
                    F_.ATTN_STREAM_TRAIN_REL_KEYS = default
            stream, other = (lambda: block(default, "stream")), (lambda: block(1 << 30, "gemm"))
            fits = H * B * T * T * ((16 if prec == "fp32" else 20) + (8 if args.drop > 0.0 else 0)) < 0.8 * torch.cuda.mem_get_info()[0]
            row = dict(precision=prec, T=T, B=B, drop=args.drop, other="gemm_softmax", rounds=[], stream_peak_bytes=peak_rise(stream),
                       other_peak_bytes=peak_rise(other) if fits else None)
            for _ in range(args.rounds):
                r = dict(stream_ms=timed(stream, args.warmup, args.iters))
                if fits:
                    r["other_ms"] = timed(other, args.warmup, args.iters)
                row["rounds"].append(r)
            for name in ("stream_ms", "other_ms") if fits else ("stream_ms",):
                row[name + "_span"] = [min(r[name] for r in row["rounds"]), max(r[name] for r in row["rounds"])]
            res["rows"].append(row)
            print(json.dumps({k_: v_ for k_, v_ in row.items() if k_ != "rounds"}), flush=True)
            del qkv, dqkv, qu, qv, dctx, p, k, v
            torch.cuda.empty_cache()
    espnet_amd.set_precision("fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", help="forward + backward rows (no relative positions)")
    ap.add_argument("--rel", action="store_true", help="with --train: one rel-pos block, streamed against GEMM + softmax, at --T (default 8192)")
    ap.add_argument("--drop", type=float, default=0.0, help="with --train: attention dropout p inside both routes (same mask)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--T", type=int, nargs="+", default=None)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    rel_train = args.train and args.rel
    if args.T is None:
        args.T = [8192] if rel_train else [4096, 8192, 22528]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "attn_stream_train_rel_bench.json" if rel_train else
                                "attn_stream_train_bench.json" if args.train else "attn_stream_bench.json")
        if args.train and args.drop > 0.0:
            args.out = args.out.replace("_bench", "_drop_bench")
    import espnet_amd
    from espnet_amd import functional as F_, ops
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except (OSError, subprocess.CalledProcessError):
            commit = "unknown"
    dev, B, H, dk = "cuda", args.B, args.H, 64
    D = H * dk
    res = dict(commit=commit, device=torch.cuda.get_device_name(0), pairs=B * H, QB=ops.ATTN_STREAM_QB, KT=ops.ATTN_STREAM_KT, rows=[])
    if args.train:
        (train_rel_rows if args.rel else train_rows)(args, res)
    for prec in () if args.train else ("fp32", "bf16"):
        espnet_amd.set_precision(prec)
        adt = ops.act_dtype()
        for rel in (True, False):
            for T in args.T:
                torch.manual_seed(T)
                mk = lambda *s: torch.randn(*s, device=dev).to(adt)  # noqa: E731
                qkv = mk(B * T, 3 * D)
                k, v = F_._MV(qkv, D, 3 * D), F_._MV(qkv, 2 * D, 3 * D)
                qu = mk(B * T, D) if rel else F_._MV(qkv, 0, 3 * D)
                qv, p = (mk(B * T, D), mk(T, D)) if rel else (None, None)
                mask = torch.ones(B, 1, T, dtype=torch.uint8, device=dev)
                stream = lambda: F_.attn_fwd_stream(qu, qv, k, v, p, mask, B, T, T, H, dk)  # noqa: E731

                def composed():
                    P = F_.attn_scores_fwd(qu, qv, k, p, mask, B, T, T, H, dk)
                    return F_.attn_context_fwd(P, v, B, T, T, H, dk)
                if ops.attn_fwd_supported(T, T, dk, rel):
                    other_name, other = "fused_long_row", lambda: F_.attn_fwd_fused(qu, qv, k, v, p, mask, B, T, T, H, dk)  # noqa: E731
                    need = H * B * T * T * qkv.element_size()
                else:
                    other_name, other = "gemm_softmax_gemm", composed
                    need = H * B * T * T * 4 * (2 if rel else 1) + (H * B * T * T * 2 if prec == "bf16" else 0)
                assert stream() is not None
                row = dict(precision=prec, rel=rel, T=T, other=other_name, rounds=[])
                fits = need < 0.8 * torch.cuda.mem_get_info()[0]
                row["stream_peak_bytes"] = peak_rise(stream)
                row["other_peak_bytes"] = None
                try:
                    if fits:
                        row["other_peak_bytes"] = peak_rise(other)
                except ops._lib.EamdError as e:          # the composition's own kernels decline the shape
                    fits, row["other_error"] = False, str(e)
                for _ in range(args.rounds):
                    r = dict(stream_ms=timed(stream, args.warmup, args.iters))
                    if fits:
                        r["other_ms"] = timed(other, args.warmup, args.iters)
                    row["rounds"].append(r)
                row["stream_ms"] = min(r["stream_ms"] for r in row["rounds"])
                row["other_ms"] = min(r["other_ms"] for r in row["rounds"]) if fits else None
                row["stream_tflops"] = B * H * T * T * dk * 2 * (3 if rel else 2) / (row["stream_ms"] * 1e-3) / 1e12
                res["rows"].append(row)
                print(json.dumps({k_: v_ for k_, v_ in row.items() if k_ != "rounds"}), flush=True)
                del qkv, k, v, qu, qv, p
                torch.cuda.empty_cache()
    espnet_amd.set_precision("fp32")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
