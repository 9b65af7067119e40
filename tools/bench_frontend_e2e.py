#!/usr/bin/env python3
"""Multichannel RNN E2E with a jointly trained front-end, at CHiME-like size (B = 32, T = 1000, F = 257, 80 mel filters, VGG
width 64, C = 6 channels):

  kernels   time per call of the four feature-transform kernels and of the VGG front-end's input gradient, next to the bytes
            each has to move, the time HBM needs for them (--hbm-tbs, 8 TB/s unless given) and - on the same device, for
            scale - the same arithmetic in torch float32
  step      one training step (forward + backward, eager: the frontend draws on the host per call) of the config-4-size
            model (VGG-BLSTM 3 x 1024, location-aware attention, LSTM decoder 1024) on 6-channel spectra with the
            beamformer draw, with the pass-through draw, and of the same model on 80 log-mel features without a frontend

  time      median over bursts of back-to-back calls between two device events (warm-up burst first)

Usage: python tools/bench_frontend_e2e.py [--B 32] [--T 1000] [--no-step] [--precision fp32]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_beamformer import timed  # noqa: E402


def kernels(a):
    from espnet_amd import ops
    from espnet_amd.nets.frontends.feature_transform import LogMel
    B, T, F, M, C1 = a.B, a.T, a.F, a.M, a.C1
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    lens_h = [T - 9 * i for i in range(B)]
    lens = torch.tensor(lens_h, dtype=torch.int32, device=dev)
    spec = torch.randn(B, T, F, 2, generator=g).to(dev)
    pad = (torch.arange(T)[None, :] >= torch.tensor(lens_h)[:, None]).to(dev)
    spec[pad] = 0
    lm = LogMel(16000, (F - 1) * 2, M).to(dev)
    mel = lm.melmat
    gm = torch.randn(B, T, M, generator=g).to(dev)
    bias, scale = torch.randn(M, generator=g).to(dev), (0.5 + torch.rand(M, generator=g)).to(dev)
    n = lens.float()[:, None, None]
    x = ops.ft_logmel_fwd(spec, mel, lm._lo, lm._hi, lens)
    dy = torch.randn(B, T, M, C1, generator=g).to(dev)
    w = (torch.randn(C1, 1, 3, 3, generator=g) / 3).to(dev)
    cx = torch.view_as_complex(spec)

    def t_logmel():
        h = (torch.matmul(cx.real ** 2 + cx.imag ** 2, mel) + 1e-20).log()
        return h.masked_fill(pad[:, :, None], 0.0)

    def t_logmel_bwd():
        r = (gm / (torch.matmul(cx.real ** 2 + cx.imag ** 2, mel) + 1e-20)).masked_fill(pad[:, :, None], 0.0)
        return 2.0 * spec * torch.matmul(r, mel.t())[..., None]

    def t_mvn():
        z = (x + bias) * scale
        return z - z.sum(1, keepdim=True) / n

    def t_mvn_bwd():
        return scale * (gm - gm.sum(1, keepdim=True) / n)

    def t_conv():
        return torch.nn.functional.conv_transpose2d(dy.permute(0, 3, 1, 2), w, padding=1)

    nspec, nfeat = spec.numel() * 4, x.numel() * 4
    rows = [
        ("eamd_ft_logmel_fwd", lambda: ops.ft_logmel_fwd(spec, mel, lm._lo, lm._hi, lens), nspec + nfeat, t_logmel),
        ("eamd_ft_logmel_bwd", lambda: ops.ft_logmel_bwd(spec, gm, mel, lm._lo, lm._hi, lm._mlo, lm._mhi, lens), 2 * nspec + nfeat,
         t_logmel_bwd),
        ("eamd_ft_mvn_fwd", lambda: ops.ft_mvn_fwd(x, lens, bias, scale, True, True, False), 2 * nfeat, t_mvn),
        ("eamd_ft_mvn_bwd", lambda: ops.ft_mvn_bwd(gm, lens, scale, True), 2 * nfeat, t_mvn_bwd),
        ("eamd_conv3x3_c1_bwd_x", lambda: ops.conv3x3_c1_bwd_x(dy, w, B, T, M, C1), dy.numel() * 4 + nfeat, t_conv),
    ]
    out = {}
    for name, fn, nbytes, tfn in rows:
        k, t = timed(fn, a.bursts, a.calls), timed(tfn, a.bursts, max(2, a.calls // 4))
        floor = nbytes / (a.hbm_tbs * 1e12) * 1e6
        out[name] = dict(us=round(k["us"], 1), us_min=round(k["us_min"], 1), us_max=round(k["us_max"], 1), mbytes=round(nbytes / 1e6, 1),
                         floor_us=round(floor, 1), hbm_frac=round(floor / k["us"], 3), tbs=round(nbytes / k["us"] / 1e6, 2),
                         torch_us=round(t["us"], 1))
        print("%-22s %8.1f us (%.1f .. %.1f)  %7.1f MB  floor %6.1f us  of the floor %.2f  (%.2f TB/s)   torch %9.1f us" % (
            name, k["us"], k["us_min"], k["us_max"], nbytes / 1e6, floor, floor / k["us"], nbytes / k["us"] / 1e6, t["us"]), flush=True)
    return out


def step(a):
    from espnet_amd.nets.e2e_asr import E2E
    from tools.bench_rnn import run
    B, T, C, F, M, L, V = a.B, a.T, a.C, a.F, a.M, 100, 5000
    base = dict(elayers=3, subsample="1_1_1_1", etype="vggblstm", eunits=1024, eprojs=1024, dtype="lstm", dlayers=1, dunits=1024,
                atype="location", aheads=4, awin=5, aconv_chans=10, aconv_filts=100, mtlalpha=0.5, lsm_type="", lsm_weight=0.0,
                sampling_probability=0.0, adim=1024, dropout_rate=0.0, dropout_rate_decoder=0.0, verbose=0, char_list=None,
                outdir=None, ctc_type="builtin", sym_space="<space>", sym_blank="<blank>", context_residual=False,
                use_frontend=False, replace_sos=False)
    fe = dict(base, use_frontend=True, use_wpe=False, wtype="blstmp", wlayers=3, wunits=300, wprojs=320, wdropout_rate=0.0,
              wpe_taps=5, wpe_delay=3, use_dnn_mask_for_wpe=False, use_beamformer=True, btype="blstmp", blayers=3, bunits=300,
              bprojs=320, bnmask=2, badim=320, ref_channel=-1, bdropout_rate=0.0, fbank_fs=16000, n_mels=M, fbank_fmin=0.0,
              fbank_fmax=None, stats_file=None, apply_uttmvn=True, uttmvn_norm_means=True, uttmvn_norm_vars=False)
    g = torch.Generator().manual_seed(0)
    ilens = [T - 7 * i for i in range(B)]
    ys = torch.randint(1, V - 1, (B, L), generator=g)
    out = {}
    torch.manual_seed(0)
    feats = torch.randn(B, T, M, generator=g).cuda()
    out["no_frontend"] = run("config4 on %d log-mel features" % M, E2E(M, V, argparse.Namespace(**base)), feats, ilens, ys,
                             graph=False, quiet=True)
    del feats
    torch.cuda.empty_cache()
    xs = torch.randn(B, T, C, F, 2, generator=g)
    for b, n in enumerate(ilens):
        xs[b, n:] = 0
    xs = xs.cuda()
    for name, bf in (("frontend_beamformer_draw", True), ("frontend_passthrough_draw", False)):
        torch.manual_seed(0)
        np.random.seed(0)
        m = E2E(F, V, argparse.Namespace(**fe))
        # one branch of the per-step draw at a time: with use_frontend_for_all the only choice is the beamformer, without
        # a beamformer the only choice is pass-through (frontend.py:101-109)
        m.frontend.use_frontend_for_all = bf
        if not bf:
            m.frontend.use_beamformer = False
        out[name] = run("config4 + frontend (%s) on %d-channel spectra" % (name, C), m, xs, ilens, ys, graph=False, quiet=True)
        del m
        torch.cuda.empty_cache()
    for k, v in out.items():
        print("%-28s %8.1f ms per eager step (best of 2), loss %.4f, grad norm %.4f, peak mem %.1f GB, %.1f M parameters" % (
            k, v["ms_per_step"], v["loss"], v["grad_norm"], v["peak_mem_gb"], v["params_m"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--C", type=int, default=6)
    ap.add_argument("--F", type=int, default=257)
    ap.add_argument("--M", type=int, default=80)
    ap.add_argument("--C1", type=int, default=64)
    ap.add_argument("--bursts", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s for the floors")
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark measures the GPU"
    import espnet_amd
    espnet_amd.set_precision(a.precision)
    res = dict(shape=dict(B=a.B, T=a.T, C=a.C, F=a.F, M=a.M, C1=a.C1), precision=a.precision, kernels=kernels(a))
    if not a.no_step:
        res["step"] = step(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
