#!/usr/bin/env python3
"""MVDR beamforming front-end at CHiME-like size (B = 32, T = 1000, C = 6, F = 257, two masks): time per call of the three
forward kernels and of the whole DNN_Beamformer forward, next to the bytes each kernel has to move and the time HBM needs
for them, and - on the same device, for scale - the same arithmetic composed from torch.einsum / torch.linalg on complex64.

  time       median over bursts of back-to-back calls between two device events (warm-up burst first)
  bytes      what the algorithm must read and write once, from the shapes: the spectrum, the logits and the outputs; the
             chunk partials the PSD kernel spills and re-reads are listed separately (they are overhead, not floor)
  floor      bytes / HBM peak (--hbm-tbs, 8 TB/s unless given)

Usage: python tools/bench_beamformer.py [--B 32] [--T 1000] [--C 6] [--F 257] [--bursts 7] [--calls 20]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(fn, bursts, calls):
    """median over bursts of the mean time of `calls` back-to-back calls, in microseconds"""
    for _ in range(max(2, calls // 4)):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(bursts):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / calls)
    return dict(us=median(ts), us_min=min(ts), us_max=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--C", type=int, default=6)
    ap.add_argument("--F", type=int, default=257)
    ap.add_argument("--bursts", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s for the floors")
    ap.add_argument("--blayers", type=int, default=3)
    ap.add_argument("--bunits", type=int, default=300)
    ap.add_argument("--bprojs", type=int, default=320)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark measures the GPU"
    import espnet_amd
    from espnet_amd import ops
    from espnet_amd.nets.frontends.dnn_beamformer import DNN_Beamformer

    espnet_amd.set_precision("fp32")
    B, T, C, F, S = a.B, a.T, a.C, a.F, 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, C, F, 2, generator=g).cuda()
    z = torch.randn(S, B, C, T, F, generator=g).cuda()
    u = torch.softmax(torch.randn(B, C, generator=g), dim=-1).cuda()
    psd, feat, nrm = ops.bf_psd(x, z)
    w = ops.bf_mvdr(psd[0], psd[1], u)
    y = ops.bf_apply(w, x)
    out_psd = (psd, feat, nrm)
    nx, nz = x.numel() * 4, z.numel() * 4
    nchunk = -(-T // ops.BF_TCHUNK)
    bytes_ = dict(
        psd=nx + nz + psd.numel() * 4 + feat.numel() * 4 + nrm.numel() * 4,
        mvdr=2 * psd[0].numel() * 4 + u.numel() * 4 + w.numel() * 4,
        apply=nx + w.numel() * 4 + y.numel() * 4)
    res = dict(B=B, T=T, C=C, F=F, S=S, device=torch.cuda.get_device_name(0), hbm_tbs=a.hbm_tbs,
               psd_partials_bytes=2 * 4 * nchunk * S * B * (C * C + 1) * F)

    xc = torch.view_as_complex(x)

    def torch_psd():
        m = torch.sigmoid(z).mean(dim=2)
        wgt = (m / (m.sum(dim=2, keepdim=True) + 1e-15)).to(torch.complex64)
        return torch.einsum("sbtf,btcf,btef->sbfce", wgt, xc, xc.conj())

    pc = torch.view_as_complex(psd)
    eye = 1e-15 * torch.eye(C, device="cuda", dtype=torch.complex64)

    def torch_mvdr():
        N = torch.linalg.solve(pc[1] + eye, pc[0])
        W = N / (N.diagonal(dim1=-2, dim2=-1).sum(-1)[..., None, None] + 1e-15)
        return torch.einsum("bfec,bc->bfe", W, u.to(torch.complex64))

    wc = torch.view_as_complex(w)

    def torch_apply():
        return torch.einsum("bfc,btcf->btf", wc.conj(), xc)

    kernels = dict(psd=(lambda: ops.bf_psd(x, z, out=out_psd), torch_psd),
                   mvdr=(lambda: ops.bf_mvdr(psd[0], psd[1], u, out=w), torch_mvdr),
                   apply=(lambda: ops.bf_apply(w, x, out=y), torch_apply))
    for name, (ours, theirs) in kernels.items():
        r = timed(ours, a.bursts, a.calls)
        floor = bytes_[name] / (a.hbm_tbs * 1e12) * 1e6
        r.update(bytes=bytes_[name], hbm_floor_us=floor, floor_over_time=floor / r["us"],
                 achieved_tbs=bytes_[name] / r["us"] * 1e-6)
        r["torch_complex64"] = timed(theirs, max(3, a.bursts // 2), max(2, a.calls // 4))
        res[name] = r
    del z
    model = DNN_Beamformer(F, "blstmp", a.blayers, a.bunits, a.bprojs, 2, 0.0, 320).cuda().eval()
    ilens = [int(v) for v in torch.linspace(T, int(0.7 * T), B).round().tolist()]
    for b, n in enumerate(ilens):
        x[b, n:] = 0
    with torch.no_grad():
        res["dnn_beamformer_forward"] = timed(lambda: model(x, ilens), max(3, a.bursts // 2), 2)
    res["dnn_beamformer_forward"]["mask_estimator"] = dict(btype="blstmp", blayers=a.blayers, bunits=a.bunits, bprojs=a.bprojs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
