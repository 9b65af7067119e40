#!/usr/bin/env python
"""Times the WPD convolutional beamformer (covariance, filter vector, apply; forward and forward + backward) on the HIP
kernels of csrc/wpd.hip, and in the same run (a) the same computation composed from torch ops on the device (complex128
matmul + torch.linalg.solve, what a user would otherwise write) and (b) the two-stage chain WPD replaces, this project's
WPE followed by its MVDR filter and apply, alternating the three.  Writes one JSON file.

    python tools/bench_wpd.py [--out profiles/wpd_bench.json] [--B 8 --T 1000 --C 8 --F 257 --btaps 5 --bdelay 3]

Times are device events around `iters` calls after `warmup` calls; the best of `rounds` alternating rounds is reported and
every round is kept.  The speech PSD Phi and the reference vector u are inputs of all three (the mask estimator and the
PSD kernels are common to them).  The backward is that of L = sum |enhanced|^2 to power, Phi and u (WPE -> MVDR: to power
and the two PSDs and u)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_wpe import synth, timed  # noqa: E402

EPS = 1e-6


def torch_wpd(y, power, phi, u, btaps, bdelay):
    """y [B,T,C,F] complex64 on the device, power [B,T,F], phi [B,F,C,C], u [B,C] -> enhanced [B,T,F] complex128; every
    utterance fills the batch"""
    B, T, C, F = y.shape
    yd = y.to(torch.complex128)
    pad = torch.cat([yd.new_zeros(B, bdelay + btaps, C, F), yd], dim=1)
    v = torch.stack([yd] + [pad[:, btaps - k:btaps - k + T] for k in range(btaps)], dim=2).reshape(B, T, (btaps + 1) * C, F)
    w = 1.0 / torch.clamp(power.double(), min=EPS)
    w = w * (torch.arange(T, device=y.device) >= bdelay + btaps - 1).to(w.dtype)[None, :, None]
    vf = v.permute(0, 3, 2, 1)                                          # [B,F,N,T]
    Rf = (vf * w.permute(0, 2, 1)[:, :, None, :]) @ vf.conj().transpose(-1, -2)
    N = Rf.shape[-1]
    X = torch.linalg.solve(Rf, torch.eye(N, C, dtype=Rf.dtype, device=y.device).expand(B, F, N, C))
    M = X @ phi.to(torch.complex128)
    tau = M[:, :, :C].diagonal(dim1=-2, dim2=-1).sum(-1) + 1e-15
    h = torch.einsum("bfic,bc->bfi", M, u.to(M.dtype)) / tau[..., None]
    return (h.conj()[:, :, None, :] @ vf).squeeze(2).permute(0, 2, 1)


def main():
    ap = argparse.ArgumentParser()
    for k, v in dict(B=8, T=1000, C=8, F=257, btaps=5, bdelay=3, warmup=3, iters=10, rounds=3).items():
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wpd_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wpd.py needs a GPU: a timing taken anywhere else says nothing")
    from espnet_amd import ops
    from espnet_amd.nets.frontends import beamformer as BF
    from espnet_amd.nets.frontends import conv_beamformer as CB
    from espnet_amd.nets.frontends.wpe import wpe_one_iteration
    dev = "cuda"
    K, D = a.btaps, a.bdelay
    y = synth(a.B, a.T, a.C, a.F).to(dev)
    yr = torch.view_as_real(y).contiguous()
    power = (y.real ** 2 + y.imag ** 2).mean(2).contiguous()
    logits = torch.randn(2, a.B, a.C, a.T, a.F, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        psd = ops.bf_psd(yr, logits)[0]
    phi_r, psd_n = psd[0].contiguous(), psd[1].contiguous()
    phi = torch.view_as_complex(phi_r)
    u = torch.softmax(torch.randn(a.B, a.C, generator=torch.Generator().manual_seed(2)), -1).to(dev)

    def hip(p, ph, uu):
        Rf = CB.get_covariances_from_power(yr, p, D, K, None, eps=EPS)
        return CB.perform_WPD_filtering(CB.get_WPD_filter_v2(ph, Rf, uu), yr, D, K, None)

    def chain(p, ps, pn, uu):
        x = wpe_one_iteration(yr, p, None, K, D)
        return BF.apply_beamforming_vector(BF.get_mvdr_vector(ps, pn, uu), x)

    def leaves(*ts):
        return [t.clone().requires_grad_(True) for t in ts]

    def hip_fwd():
        with torch.no_grad():
            return hip(power, phi_r, u)

    def hip_fwd_bwd():
        p, ph, uu = leaves(power, phi_r, u)
        hip(p, ph, uu).square().sum().backward()
        return p.grad, ph.grad, uu.grad

    def torch_fwd():
        with torch.no_grad():
            return torch_wpd(y, power, phi, u, K, D)

    def torch_fwd_bwd():
        p, ph, uu = leaves(power, phi, u)
        e = torch_wpd(y, p, ph, uu, K, D)
        (e.real ** 2 + e.imag ** 2).sum().backward()
        return p.grad, ph.grad, uu.grad

    def chain_fwd():
        with torch.no_grad():
            return chain(power, phi_r, psd_n, u)

    def chain_fwd_bwd():
        p, ps, pn, uu = leaves(power, phi_r, psd_n, u)
        chain(p, ps, pn, uu).square().sum().backward()
        return p.grad

    with torch.no_grad():
        Rf = ops.wpd_cov(yr, power, None, K, D, EPS)
        h = ops.wpd_vector(Rf, phi_r, u, keep=False)[0]
    kernels = dict(cov=lambda: ops.wpd_cov(yr, power, None, K, D, EPS), vector=lambda: ops.wpd_vector(Rf, phi_r, u, keep=True),
                   apply=lambda: ops.wpd_apply(h, yr, None, K, D))

    # the HIP path and the torch path compute the same thing: compare before timing
    e_hip, e_ref = torch.view_as_complex(hip_fwd()), torch_fwd()
    g_hip, g_ref = hip_fwd_bwd(), torch_fwd_bwd()
    rel = lambda x, r: float((x - r).abs().max() / r.abs().max())  # noqa: E731
    agree = dict(enhanced=rel(e_hip, e_ref), gpower=rel(g_hip[0], g_ref[0]), gphi=rel(torch.view_as_complex(g_hip[1]), g_ref[1]),
                 gu=rel(g_hip[2], g_ref[2]))
    del e_hip, e_ref, g_hip, g_ref
    fns = dict(hip_fwd=hip_fwd, torch_fwd=torch_fwd, wpe_mvdr_fwd=chain_fwd, hip_fwd_bwd=hip_fwd_bwd, torch_fwd_bwd=torch_fwd_bwd,
               wpe_mvdr_fwd_bwd=chain_fwd_bwd, **{"kernel_" + k: v for k, v in kernels.items()})
    times = {k: [] for k in fns}
    for _ in range(a.rounds):                                           # alternate: other work shares the machine
        for k, fn in fns.items():
            times[k].append(timed(fn, a.warmup, a.iters))
    ms = {k: min(v) for k, v in times.items()}
    res = dict(shape=dict(B=a.B, T=a.T, C=a.C, F=a.F, btaps=K, bdelay=D), device=torch.cuda.get_device_name(0),
               warmup=a.warmup, iters=a.iters, rounds=a.rounds, ms_best=ms, ms_all=times, max_rel_diff_hip_vs_torch=agree,
               speedup_vs_torch_fwd=ms["torch_fwd"] / ms["hip_fwd"], speedup_vs_torch_fwd_bwd=ms["torch_fwd_bwd"] / ms["hip_fwd_bwd"],
               wpd_over_wpe_mvdr_fwd=ms["hip_fwd"] / ms["wpe_mvdr_fwd"],
               wpd_over_wpe_mvdr_fwd_bwd=ms["hip_fwd_bwd"] / ms["wpe_mvdr_fwd_bwd"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "ms_all"}))


if __name__ == "__main__":
    main()
