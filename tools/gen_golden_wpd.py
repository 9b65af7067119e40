#!/usr/bin/env python3
"""WPD fixture, by RUNNING THE REFERENCE's espnet2/enh/layers/conv_beamformer.py (PyTorch CPU, float64):

  tests/golden/wpd.npz   per case `<case>/...` of tests/wpd_restatement.CASES at F = 5: the inputs y, power, phi, u (stored
                         as float32: the float64 run computes on exactly these values) and ilens, and `ws` (B, F, N) and
                         `enhanced` (B, T, F) of get_covariances -> get_WPD_filter_v2 -> perform_WPD_filtering with
                         inverse_power = 1 / clamp(power, 1e-6).

The reference sums over all frames of the padded batch; this project stops at each utterance's length (DESIGN.md section
4).  So an utterance that fills the batch is recorded from the batch, and a shorter one from the reference run on that
utterance alone, cut to its length.

The reference computes on torch_complex.ComplexTensor, a package that is absent here: install_complex() of
oracle/gen_golden_beamformer.py provides the stand-in on torch's native complex tensors, and this script adds the two
functions conv_beamformer.py needs beyond it, functional.pad and functional.reverse.  conv_beamformer.py is loaded by
path; the one module it imports from the espnet package (frontends.beamformer, used only by its __main__ example) is
replaced by an empty module.

Complex arrays are stored with a trailing (re, im) axis, in the reference's layouts.

Usage: python tools/gen_golden_wpd.py --ref <reference checkout> [--out tests/golden]
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_golden_beamformer import install_complex  # noqa: E402

F = 5
EPS = 1e-6


def load_reference(ref):
    install_complex()
    fc = sys.modules["torch_complex.functional"]

    def pad(x, pad, mode="constant", value=0):
        f = torch.nn.functional.pad
        return torch.complex(f(x.real, pad, mode, value), f(x.imag, pad, mode, value))

    fc.pad = pad
    fc.reverse = lambda x, dim: torch.flip(x, dims=(dim,))
    for name in ("espnet", "espnet.nets", "espnet.nets.pytorch_backend", "espnet.nets.pytorch_backend.frontends",
                 "espnet.nets.pytorch_backend.frontends.beamformer"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["espnet.nets.pytorch_backend.frontends"].beamformer = sys.modules["espnet.nets.pytorch_backend.frontends.beamformer"]
    spec = importlib.util.spec_from_file_location("ref_conv_beamformer",
                                                  os.path.join(ref, "espnet2", "enh", "layers", "conv_beamformer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ri(t):
    return torch.view_as_real(t.detach().resolve_conj()).numpy().copy()


def run_reference(mod, y, power, phi, u, btaps, bdelay):
    """y [B,T,C,F], power [B,T,F], phi [B,F,C,C], u [B,C] in this project's layouts, float64 -> (ws (B,F,N), enhanced (B,T,F))"""
    Y = y.permute(0, 3, 2, 1)                                                     # (B, F, C, T)
    inverse_power = 1.0 / torch.clamp(power.permute(0, 2, 1), min=EPS)            # (B, F, T)
    Rf = mod.get_covariances(Y, inverse_power, bdelay, btaps, get_vector=False)
    ws = mod.get_WPD_filter_v2(phi, Rf, u)
    enhanced = mod.perform_WPD_filtering(ws, Y, bdelay, btaps)                    # (B, F, T)
    return ws, enhanced.permute(0, 2, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import wpd_restatement as W
    mod = load_reference(args.ref)
    out = {}
    for ci, (C, K, D, T, ilens) in enumerate(W.CASES):
        y32, z, phi32, u32 = W.inputs(ci, F)
        power32 = W.masked_power(y32, z).float()
        y, power, phi, u = y32.to(torch.complex128), power32.double(), phi32.to(torch.complex128), u32.double()
        ws, enhanced = run_reference(mod, y, power, phi, u, K, D)
        for b, n in enumerate(ilens):
            if n < T:                                                              # the reference on this utterance alone
                wb, eb = run_reference(mod, y[b:b + 1, :n], power[b:b + 1, :n], phi[b:b + 1], u[b:b + 1], K, D)
                ws[b], enhanced[b, :n], enhanced[b, n:] = wb[0], eb[0], 0
        key = W.IDS[ci]
        out.update({key + "/y": ri(y32), key + "/power": power32.numpy(), key + "/phi": ri(phi32), key + "/u": u32.numpy(),
                    key + "/ilens": np.asarray(ilens, np.int64), key + "/ws": ri(ws), key + "/enhanced": ri(enhanced)})
    path = os.path.join(args.out, "wpd.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
