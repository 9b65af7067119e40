#!/usr/bin/env python
"""Times the WPE step of DNN_WPE (wpe_one_iteration: correlations, solve, filter; forward and forward + backward) on the
HIP kernels of csrc/wpe.hip, and in the same run the same computation composed from torch ops on the device (complex128
matmul + torch.linalg.solve, what a user would otherwise write), alternating the two.  Writes one JSON file.

    python tools/bench_wpe.py [--out profiles/wpe_bench.json] [--B 8 --T 1000 --C 8 --F 257 --taps 5 --delay 3]

Times are device events around `iters` calls after `warmup` calls.  Bytes and FLOPs are the algorithm's, computed from the
shape: forward reads y and power and writes x; the correlation pass forms the upper triangle of R and P (8 real FLOPs per
complex multiply-add), the solve is an LDL^H factorisation plus two substitutions, the filter N C multiply-adds per frame.
The peaks: 6.29 TB/s (measured HBM copy rate of an MI355X) and 78.6 TFLOP/s (the MI355X datasheet's fp64 vector rate)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12
FP64_FLOPS = 78.6e12
EPS = 1e-10


def synth(B, T, C, F, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.complex(torch.randn(*s, generator=g), torch.randn(*s, generator=g))  # noqa: E731
    s = rn(B, T, 1, F)
    y = 0.3 * rn(B, T, C, F)
    for d in range(12):
        y[:, d:] += (0.7 ** d) * rn(1, 1, C, F) * s[:, :T - d]
    return y


def torch_wpe(y, power, taps, delay):
    """y [B,T,C,F] complex64 on the device, power [B,T,F] -> enhanced complex128; every utterance fills the batch"""
    B, T, C, F = y.shape
    yd = y.to(torch.complex128)
    pad = torch.cat([yd.new_zeros(B, delay + taps - 1, C, F), yd], dim=1)
    h = torch.stack([pad[:, taps - 1 - k:taps - 1 - k + T] for k in range(taps)], dim=2).reshape(B, T, taps * C, F)
    w = 1.0 / torch.clamp(power.double(), min=EPS)
    w = w * (torch.arange(T, device=y.device) >= delay + taps - 1).to(w.dtype)[None, :, None]
    hf = h.permute(0, 3, 2, 1)                                          # [B,F,N,T]
    hw = hf * w.permute(0, 2, 1)[:, :, None, :]
    R = hw @ hf.conj().transpose(-1, -2)
    P = hw @ yd.permute(0, 3, 1, 2).conj()                              # [B,F,T,C]
    G = torch.linalg.solve(R, P)
    return yd - (G.conj().transpose(-1, -2) @ hf).permute(0, 3, 2, 1)                # [B,F,C,T] -> [B,T,C,F]


def timed(fn, warmup, iters):
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


def main():
    ap = argparse.ArgumentParser()
    for k, v in dict(B=8, T=1000, C=8, F=257, taps=5, delay=3, warmup=3, iters=10, rounds=3).items():
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wpe_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wpe.py needs a GPU: a timing taken anywhere else says nothing")
    from espnet_amd.nets.frontends.wpe import wpe_one_iteration
    dev = "cuda"
    y = synth(a.B, a.T, a.C, a.F).to(dev)
    yr = torch.view_as_real(y).contiguous()
    power = (y.real ** 2 + y.imag ** 2).mean(2).contiguous()

    def hip_fwd():
        with torch.no_grad():
            return wpe_one_iteration(yr, power, None, a.taps, a.delay)

    def hip_fwd_bwd():
        p = power.clone().requires_grad_(True)
        wpe_one_iteration(yr, p, None, a.taps, a.delay).square().sum().backward()
        return p.grad

    def torch_fwd():
        with torch.no_grad():
            return torch_wpe(y, power, a.taps, a.delay)

    def torch_fwd_bwd():
        p = power.clone().requires_grad_(True)
        x = torch_wpe(y, p, a.taps, a.delay)
        (x.real ** 2 + x.imag ** 2).sum().backward()
        return p.grad

    # the two compute the same thing: compare before timing (fp32 outputs of an fp64 computation against complex128)
    x_hip, x_ref = torch.view_as_complex(hip_fwd()), torch_fwd()
    g_hip, g_ref = hip_fwd_bwd(), torch_fwd_bwd()
    agree = dict(x=float((x_hip - x_ref).abs().max() / x_ref.abs().max()),
                 gpower=float((g_hip - g_ref).abs().max() / g_ref.abs().max()))
    del x_hip, x_ref, g_hip, g_ref
    fns = dict(hip_fwd=hip_fwd, torch_fwd=torch_fwd, hip_fwd_bwd=hip_fwd_bwd, torch_fwd_bwd=torch_fwd_bwd)
    times = {k: [] for k in fns}
    for _ in range(a.rounds):                                           # alternate: other work shares the machine
        for k, fn in fns.items():
            times[k].append(timed(fn, a.warmup, a.iters))
    ms = {k: min(v) for k, v in times.items()}
    N = a.C * a.taps
    btf = a.B * a.T * a.F
    fwd_bytes = btf * (2 * a.C * 8 + 4)
    fwd_flops = btf * 8 * (N * (N + 1) // 2 + N * a.C + N * a.C) + a.B * a.F * 8 * (N ** 3 // 3 + 2 * N * N * a.C)
    bwd_bytes = btf * (3 * a.C * 8 + 2 * 4)                             # y, x, gx read; power read, gpower written
    bwd_flops = btf * 8 * (2 * N * a.C + a.C) + a.B * a.F * 8 * 2 * N * N * a.C
    res = dict(shape=dict(B=a.B, T=a.T, C=a.C, F=a.F, taps=a.taps, delay=a.delay), device=torch.cuda.get_device_name(0),
               warmup=a.warmup, iters=a.iters, rounds=a.rounds, ms_best=ms, ms_all=times, max_rel_diff_hip_vs_torch=agree,
               speedup_fwd=ms["torch_fwd"] / ms["hip_fwd"], speedup_fwd_bwd=ms["torch_fwd_bwd"] / ms["hip_fwd_bwd"],
               fwd=dict(bytes=fwd_bytes, flops_fp64=fwd_flops,
                        hbm_fraction=fwd_bytes / HBM_BYTES_PER_S / (ms["hip_fwd"] * 1e-3),
                        fp64_fraction=fwd_flops / FP64_FLOPS / (ms["hip_fwd"] * 1e-3)),
               fwd_bwd=dict(bytes=fwd_bytes + bwd_bytes, flops_fp64=fwd_flops + bwd_flops,
                            hbm_fraction=(fwd_bytes + bwd_bytes) / HBM_BYTES_PER_S / (ms["hip_fwd_bwd"] * 1e-3),
                            fp64_fraction=(fwd_flops + bwd_flops) / FP64_FLOPS / (ms["hip_fwd_bwd"] * 1e-3)),
               peaks=dict(hbm_bytes_per_s=HBM_BYTES_PER_S, fp64_flops=FP64_FLOPS))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(ms_best=ms, speedup_fwd=res["speedup_fwd"], speedup_fwd_bwd=res["speedup_fwd_bwd"], agree=agree)))


if __name__ == "__main__":
    main()
