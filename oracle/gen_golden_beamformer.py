#!/usr/bin/env python3
"""MVDR beamformer fixture, by RUNNING THE REFERENCE (kan-bayashi/espnet v0.9.5, PyTorch CPU) in the build container:

  beamformer.npz   per case `<case>/...`: the multi-channel spectrum, lengths and seeded weights (stored as float32: the
                   float64 run computes on exactly these values), and from the reference's DNN_Beamformer run in
                   float64: psd_speech, psd_noise, u, ws, enhanced, mask_speech and the parameter gradients of
                   L = sum |enhanced|^2.  `<case>/zero_grads`: parameters whose gradient is identically zero (the bias
                   in front of the softmax over channels: softmax is shift invariant) - the float64 run gives rounding
                   noise for them, 1e-12 of the largest gradient or less, which is no yardstick and is not recorded.
                   `<case>/err32/<name>`: the reference's OWN float32-vs-float64 discrepancy of that quantity on the same
                   inputs and weights, max |f32 - f64| / max |f64| - the yardstick of the fp32 kernels' tests.
                   `state_dict_keys`: the keys of the reference Frontend(use_beamformer=True, blayers=1).

The reference's front-end computes on torch_complex.ComplexTensor, a package that is absent here.  `install_complex()`
puts a stand-in into sys.modules - ComplexTensor, functional.einsum and functional.trace on torch's native complex
tensors - BEFORE gen_golden.install_stubs() would install its inert one.

Complex arrays are stored with a trailing (re, im) axis.  Layouts are the reference's: psd (B, F, C, C), ws (B, F, C),
enhanced (B, T, F), mask_speech (B, T, C, F).

Usage: python oracle/gen_golden_beamformer.py [--ref /root/reference] [--out tests/golden]
"""
import argparse
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import install_stubs, save  # noqa: E402

# name: (B, T, C, F, ilens, ref_channel); 2-layer blstmp of 8 units / projections, attention width 8.  One utterance is
# shorter than the batch (its padded frames enter the mask normaliser), every utterance has at least 4 C frames (with
# fewer frames than channels the noise PSD is singular).  With C = 2 the attention reference sees the same feature on
# both channels (|psd[0,1]| = |psd[1,0]|), u = (1/2, 1/2) whatever the weights: C = 2 runs with the fixed reference.
CASES = {
    "c3": (2, 40, 3, 17, (40, 23), -1),
    "c2ref0": (2, 40, 2, 33, (40, 23), 0),
    "c8": (2, 36, 8, 17, (36, 33), -1),
}
LAYERS, UNITS, PROJS, ADIM = 2, 8, 8, 8


def install_complex():
    class _Meta(type):
        def __instancecheck__(cls, obj):
            return torch.is_tensor(obj) and obj.is_complex()

    class ComplexTensor(metaclass=_Meta):
        def __new__(cls, real, imag=None):
            real = torch.as_tensor(real)
            if real.is_complex():
                return real
            return torch.complex(real, torch.zeros_like(real) if imag is None else torch.as_tensor(imag))

    def _cx(ops):
        dt = torch.complex128 if any(o.dtype in (torch.float64, torch.complex128) for o in ops) else torch.complex64
        return [o.to(dt) for o in ops]

    def einsum(equation, *operands):
        if len(operands) == 1 and isinstance(operands[0], (list, tuple)):
            operands = operands[0]
        return torch.einsum(equation, *_cx(operands))

    def trace(a):
        return a.diagonal(dim1=-2, dim2=-1).sum(-1)

    tc = types.ModuleType("torch_complex")
    tc.tensor = types.ModuleType("torch_complex.tensor")
    tc.tensor.ComplexTensor = ComplexTensor
    tc.functional = types.ModuleType("torch_complex.functional")
    tc.functional.einsum, tc.functional.trace = einsum, trace
    tc.ComplexTensor = ComplexTensor
    sys.modules.update({"torch_complex": tc, "torch_complex.tensor": tc.tensor, "torch_complex.functional": tc.functional})
    try:
        import distutils.version  # noqa: F401
    except Exception:  # noqa: BLE001  (removed from Python 3.12; dnn_beamformer.py:1 compares torch versions with it)
        class LooseVersion(str):
            def _k(self):
                return [int(p) for p in self.split("+")[0].split(".")[:3] if p.isdigit()]

            def __ge__(self, other):
                return self._k() >= LooseVersion(other)._k()
        du = types.ModuleType("distutils")
        du.version = types.ModuleType("distutils.version")
        du.version.LooseVersion = LooseVersion
        sys.modules.update({"distutils": du, "distutils.version": du.version})


def ri(t):
    return torch.view_as_real(t.detach().resolve_conj()).numpy().copy()


def run_case(mods, model32, x32, ilens, double):
    """the reference's DNN_Beamformer.forward and the backward of sum |enhanced|^2 -> dict of float64 / float32 arrays"""
    bf_mod = mods["dnn_beamformer"]
    model = copy.deepcopy(model32)
    torch.set_default_dtype(torch.float64 if double else torch.float32)
    try:
        if double:
            model = model.double()
        x = x32.to(torch.complex128 if double else torch.complex64)
        seen = {}
        real_mvdr = bf_mod.get_mvdr_vector

        def spy(psd_s, psd_n, u):
            seen.update(psd_speech=psd_s.clone(), psd_noise=psd_n.clone(), u=u.clone())   # before `psd_n += eps * eye`
            seen["ws"] = real_mvdr(psd_s, psd_n, u)
            return seen["ws"]

        bf_mod.get_mvdr_vector = spy
        try:
            enhanced, _, mask_speech = model(x, torch.as_tensor(ilens))
        finally:
            bf_mod.get_mvdr_vector = real_mvdr
        loss = (enhanced.real ** 2 + enhanced.imag ** 2).sum()
        loss.backward()
        out = dict(psd_speech=ri(seen["psd_speech"]), psd_noise=ri(seen["psd_noise"]), u=seen["u"].detach().numpy().copy(),
                   ws=ri(seen["ws"]), enhanced=ri(enhanced), mask_speech=mask_speech.detach().contiguous().numpy().copy(),
                   loss=loss.detach().numpy().copy())
        for k, p in model.named_parameters():
            if p.grad is not None:
                out["grad/" + k] = p.grad.detach().numpy().copy()
        return out
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden"))
    a = ap.parse_args()
    install_complex()
    install_stubs()
    sys.path.insert(0, a.ref)
    torch.set_num_threads(4)
    from espnet.nets.pytorch_backend.frontends import dnn_beamformer
    from espnet.nets.pytorch_backend.frontends.frontend import Frontend
    mods = {"dnn_beamformer": dnn_beamformer}
    rec = {}
    fe = Frontend(idim=257, use_beamformer=True, blayers=1, bunits=8, bprojs=8, badim=8)
    rec["state_dict_keys"] = np.asarray(list(fe.state_dict().keys()))
    models = {}
    for name, (B, T, C, F, ilens, ref_channel) in CASES.items():
        g = torch.Generator().manual_seed(1000 + 10 * C + F)
        key = (C, F)
        x = torch.complex(torch.randn(B, T, C, F, generator=g), torch.randn(B, T, C, F, generator=g))
        # a spatially coherent source under the noise, so that speech and noise PSDs differ as they do on real arrays
        steer = torch.complex(torch.randn(C, F, generator=g), torch.randn(C, F, generator=g))
        src = torch.complex(torch.randn(B, T, 1, F, generator=g), torch.randn(B, T, 1, F, generator=g))
        x = (0.6 * x + src * steer).to(torch.complex64)
        for b, n in enumerate(ilens):
            x[b, n:] = 0                                                    # Stft.forward zeroes the padded frames
        if key not in models:
            torch.manual_seed(7 + 100 * C + F)
            models[key] = dnn_beamformer.DNN_Beamformer(F, "blstmp", LAYERS, UNITS, PROJS, 2, 0.0, ADIM)
        model = models[key]
        model.ref_channel = ref_channel
        model.train()
        r64 = run_case(mods, model, x, ilens, True)
        r32 = run_case(mods, model, x, ilens, False)
        p = name + "/"
        rec[p + "x"] = torch.view_as_real(x).numpy()
        rec[p + "ilens"] = np.asarray(ilens, dtype=np.int64)
        rec[p + "ref_channel"] = np.asarray(ref_channel, dtype=np.int64)
        for k, v in model.state_dict().items():
            rec[p + "sd/" + k] = v.detach().numpy()
        gmax = max(float(np.abs(v).max()) for k, v in r64.items() if k.startswith("grad/"))
        zero = [k[5:] for k, v in r64.items() if k.startswith("grad/") and float(np.abs(v).max()) <= 1e-12 * gmax]
        rec[p + "zero_grads"] = np.asarray(zero)
        for k, v in r64.items():
            if k[5:] in zero and k.startswith("grad/"):
                continue
            rec[p + k] = v
            den = float(np.abs(v).max())
            err = float(np.abs(r32[k].astype(np.float64) - v).max()) / den if den > 0 else 0.0
            rec[p + "err32/" + k] = np.asarray(err)
        A = torch.view_as_complex(torch.from_numpy(r64["psd_noise"]))
        cond = float(torch.linalg.cond(A).max())
        rec[p + "cond_psd_noise"] = np.asarray(cond)
        worst_g = max(float(rec[p + "err32/" + k]) for k in r64 if k.startswith("grad/") and k[5:] not in zero)
        print("%-7s B,T,C,F=%s ilens=%s  err32: enhanced %.2e ws %.2e u %.2e psd_n %.2e  worst grad %.2e  cond(psd_n) %.1f" % (
            name, (B, T, C, F), ilens, rec[p + "err32/enhanced"], rec[p + "err32/ws"], rec[p + "err32/u"],
            rec[p + "err32/psd_noise"], worst_g, cond), "zero grads:", zero, flush=True)
    save(os.path.join(a.out, "beamformer.npz"), **rec)


if __name__ == "__main__":
    main()
