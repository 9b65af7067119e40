#!/usr/bin/env python
"""Times the E-Branchformer's gating-unit kernels (csrc/cgmlp.hip) at B = 32, T = 249, Ch = 1024, K = 31 and, in the same
run, the same formulas composed from torch float32 ops on the device (restated here, not imported), alternating the two;
then one 12-layer encoder training step (forward + backward, fp32) at config-2 width (256 wide, 4 heads, 2048 units)
beside the Conformer's.  Writes one JSON file.

    python tools/bench_branchformer.py [--out profiles/branchformer_bench.json] [--B 32 --T 249 --Ch 1024 --K 31]

Times are device events around at least `iters` calls and at least 50 ms of work after `warmup` calls; the best of
`rounds` alternating rounds is reported and every round is kept.  For the kernels the JSON also gives the least traffic
(one read of every operand, one write of every result) and the share of 6.3 TB/s it amounts to over the measured time."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.3e12
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


def t_csgu(a, gamma, beta, w, bias):
    Ch, K = w.shape[0], w.shape[-1]
    r, g = F.gelu(a).chunk(2, dim=-1)
    n = F.layer_norm(g, (Ch,), gamma, beta, 1e-12)
    return r * F.conv1d(n.transpose(1, 2), w, bias, padding=(K - 1) // 2, groups=Ch).transpose(1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branchformer_bench.json"))
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=249)
    ap.add_argument("--Ch", type=int, default=1024)
    ap.add_argument("--K", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=12)
    args = ap.parse_args()
    import espnet_amd
    from espnet_amd import functional as F_
    from espnet_amd.espnet2 import ConformerEncoder, EBranchformerEncoder
    espnet_amd.set_precision("fp32")
    dev, (B, T, Ch, K) = "cuda", (args.B, args.T, args.Ch, args.K)
    torch.manual_seed(0)
    a = torch.randn(B, T, 2 * Ch, device=dev, requires_grad=True)
    gamma, beta, bias = (torch.randn(Ch, device=dev, requires_grad=True) for _ in range(3))
    w = (torch.randn(Ch, 1, K, device=dev) / K ** 0.5).requires_grad_(True)
    dy = torch.randn(B, T, Ch, device=dev)
    par = (a, gamma, beta, w, bias)

    def fwd(fn):
        with torch.no_grad():
            fn()

    def fb(fn):
        for t in par:
            t.grad = None
        fn().backward(dy)

    hip = lambda: F_.CSGUFn.apply(a, gamma, beta, w, bias, 1e-12)  # noqa: E731
    tor = lambda: t_csgu(*par)  # noqa: E731
    res = dict(shape=dict(B=B, T=T, Ch=Ch, K=K), rounds=[])
    for _ in range(args.rounds):
        res["rounds"].append(dict(
            hip_fwd_ms=timed(lambda: fwd(lambda: F_.run(F_.CSGUFn, a, gamma, beta, w, bias, 1e-12)), args.warmup, args.iters),
            torch_fwd_ms=timed(lambda: fwd(tor), args.warmup, args.iters),
            hip_fwd_bwd_ms=timed(lambda: fb(hip), args.warmup, args.iters),
            torch_fwd_bwd_ms=timed(lambda: fb(tor), args.warmup, args.iters)))
    for k in res["rounds"][0]:
        res[k] = min(r[k] for r in res["rounds"])
    rows = B * T
    res["fwd_min_bytes"] = rows * 3 * Ch * 4                       # read a, write y
    res["fwd_bwd_min_bytes"] = rows * (3 + 2 + 1 + 2) * Ch * 4     # + read a, dy, write da
    res["hip_fwd_hbm_share"] = res["fwd_min_bytes"] / (res["hip_fwd_ms"] * 1e-3) / HBM
    res["hip_fwd_bwd_hbm_share"] = res["fwd_bwd_min_bytes"] / (res["hip_fwd_bwd_ms"] * 1e-3) / HBM

    xs, ilens = torch.randn(B, 4 * T + 3, 80, device=dev), [4 * T + 3] * B       # conv2d input: T frames behind it
    kw = dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=args.layers, dropout_rate=0.1)
    encs = dict(e_branchformer=EBranchformerEncoder(80, cgmlp_linear_units=2 * Ch, cgmlp_conv_kernel=K, use_ffn=True,
                                                    macaron_ffn=True, **kw),
                conformer=ConformerEncoder(80, macaron_style=True, cnn_module_kernel=K, **kw))
    steps = {}
    for name, enc in encs.items():
        enc = enc.to(dev).train()

        def step():
            enc.zero_grad(set_to_none=True)
            enc(xs, ilens)[0].sum().backward()
        steps[name] = step
    res["step_rounds"] = [{n + "_step_ms": timed(s, 2, 5) for n, s in steps.items()} for _ in range(args.rounds)]
    for k in res["step_rounds"][0]:
        res[k] = min(r[k] for r in res["step_rounds"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("rounds")}))


if __name__ == "__main__":
    main()
