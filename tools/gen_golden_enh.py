#!/usr/bin/env python3
"""Enhancement fixture, by RUNNING THE REFERENCE's espnet2/enh/espnet_model.py, nets/tf_mask_net.py, nets/beamformer_net.py
and espnet2/layers/stft.py (PyTorch CPU, float64):

  tests/golden/enh.npz   recorded inputs (float32 values) and float64 results only:
      istft/<case>/...     Stft.inverse on random spectra, the cases of tests/enh_cases.py
      label/...            _create_mask_label, all six types, S = 3, a mixture with exact-zero frames
      loss/<S>/<kind>/...  _permutation_loss with tf_mse_loss on masks / magnitudes / spectra and both SI-SNR criteria,
                           S = 1, 2, 3: the batch loss, the per-utterance permutation losses and the chosen permutation
      tfm/<case>/...       ESPnetEnhancementModel(TFMaskingNet): weights (seeded), batch, loss, permutation, si_snr and
                           every parameter gradient, for the four loss types in training and "spectrum" in eval mode
      bfn/<case>/...       ESPnetEnhancementModel(BeamformerNet("mvdr")) in training with mask_mse, the fixed reference
                           channel 0 and the attention reference: loss and parameter gradients

Stand-ins, all in this process: torch_complex on torch's native complex tensors (install_complex of
oracle/gen_golden_beamformer.py), typeguard (check_argument_types is True), distutils; torch.stft / torch.istft of this
torch want complex tensors, so they are wrapped (return_complex=True + view_as_real, view_as_complex); and Tensor.float()
is the identity while the reference runs, so that the run is float64 throughout (the reference calls .float() on its
ComplexTensor in predict_mask, which on a native complex tensor would drop the imaginary part).

Usage: python tools/gen_golden_enh.py --ref <reference checkout> [--out tests/golden]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_golden import install_stubs  # noqa: E402
from gen_golden_beamformer import install_complex  # noqa: E402

import enh_cases as K  # noqa: E402


def load_reference(ref):
    install_complex()
    install_stubs()
    tg = types.ModuleType("typeguard")
    tg.check_argument_types = lambda *a, **k: True
    tg.check_return_type = lambda *a, **k: True
    sys.modules["typeguard"] = tg
    real_stft, real_istft = torch.stft, torch.istft

    def stft(input, *a, **kw):
        kw.pop("return_complex", None)
        return torch.view_as_real(real_stft(input, *a, return_complex=True, **kw))

    def istft(input, *a, **kw):
        if kw.get("length") is not None:
            kw["length"] = int(kw["length"])
        return real_istft(torch.view_as_complex(input.contiguous()), *a, **kw)

    torch.stft = stft
    torch.functional.stft = stft
    torch.istft = istft
    torch.functional.istft = istft
    torch.Tensor.float = lambda self, *a, **k: self
    sys.path.insert(0, ref)
    from espnet2.enh.espnet_model import ESPnetEnhancementModel
    from espnet2.enh.nets.beamformer_net import BeamformerNet
    from espnet2.enh.nets.tf_mask_net import TFMaskingNet
    from espnet2.layers.stft import Stft
    return ESPnetEnhancementModel, TFMaskingNet, BeamformerNet, Stft


def cx(a):
    return torch.view_as_complex(torch.as_tensor(np.ascontiguousarray(a)).double())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    Model, TFMaskingNet, BeamformerNet, Stft = load_reference(args.ref)
    import seeded_weights as SW
    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(4)
    out = {}

    def pair_of(ref, inf, criterion):
        """[B, S, S]: the reference's criterion on every (reference, estimate) pair"""
        return torch.stack([torch.stack([criterion(r, e) for e in inf], dim=1) for r in ref], dim=1).detach().numpy()

    # ---- Stft.inverse ----------------------------------------------------------------------------------------------------
    for name, c in K.ISTFT_CASES.items():
        spec = K.istft_input(name)
        st = Stft(n_fft=c["n_fft"], win_length=c["win_length"], hop_length=c["hop"], center=c["center"],
                  normalized=c["normalized"], onesided=c["onesided"])
        ilens = None if c["length"] is None else torch.as_tensor([c["length"]] * spec.shape[0])
        wav, _ = st.inverse(torch.as_tensor(spec).double(), ilens)
        out["istft/%s/spec" % name], out["istft/%s/wav" % name] = spec, wav.numpy()

    # ---- labels and losses -----------------------------------------------------------------------------------------------
    model = Model(TFMaskingNet(n_fft=32, hop_length=8, layer=1, unit=8, num_spk=3))
    mix, refs = K.label_input()
    out["label/mix"], out["label/refs"] = mix, refs
    for t in K.LABELS:
        lab = model._create_mask_label(cx(mix), [cx(r) for r in refs], mask_type=t)
        out["label/" + t] = np.stack([v.double().numpy() for v in lab])
    crit = {"mse": Model.tf_mse_loss, "si_snr": Model.si_snr_loss, "si_snr_zeromean": Model.si_snr_loss_zeromean}
    for S in (1, 2, 3):
        for kind, (ref, inf, cname) in K.loss_inputs(S).items():
            out["loss/%d/%s/ref" % (S, kind)], out["loss/%d/%s/inf" % (S, kind)] = ref, inf
            cplx = kind in ("magnitude", "spectrum", "spectrum4d")
            r = [cx(v) if cplx else torch.as_tensor(v).double() for v in ref]
            e = [cx(v) if cplx else torch.as_tensor(v).double() for v in inf]
            if kind == "magnitude":
                r, e = [abs(v) for v in r], [abs(v) for v in e]
            loss, perm = Model._permutation_loss(r, e, crit[cname])
            out["loss/%d/%s/loss" % (S, kind)], out["loss/%d/%s/perm" % (S, kind)] = loss.numpy(), perm.numpy()
            out["loss/%d/%s/pair" % (S, kind)] = pair_of(r, e, crit[cname])

    # ---- models ------------------------------------------------------------------------------------------------------------
    def record(prefix, net, batch, lens, training):
        m = Model(net).double()
        m.train(training)
        real = Model._permutation_loss
        pairs = []

        def spy(ref, inf, criterion, perm=None):
            pairs.append(pair_of(ref, inf, criterion))
            loss, perm = real(ref, inf, criterion, perm)
            out.setdefault(prefix + "perm", perm.numpy())
            return loss, perm

        m._permutation_loss = spy
        loss, stats, weight = m(batch["speech_mix"].double(), torch.as_tensor(lens), **{k: v.double() for k, v in batch.items()
                                                                                       if k != "speech_mix"})
        out[prefix + "loss"] = loss.detach().numpy()
        out[prefix + "pair"] = pairs[0]
        if stats["si_snr"] is not None:
            out[prefix + "si_snr"] = stats["si_snr"].detach().numpy()
        if training:
            loss.backward()
            for k, p in net.named_parameters():
                if p.grad is not None:
                    out[prefix + "grad/" + k] = p.grad.numpy().copy()
        for k, v in net.state_dict().items():
            out[prefix + "sd/" + k] = v.detach().to(torch.float32).numpy()
        for k, v in batch.items():
            out[prefix + "in/" + k] = v.numpy()
        out[prefix + "lens"] = np.asarray(lens, np.int64)

    for name, c in K.TFM_CASES.items():
        net = SW.fill_parameters(TFMaskingNet(**c["conf"]), salt=c["salt"]).double()
        net.loss_type = c.get("loss_type", net.loss_type)          # TFMaskingNet's constructor refuses "si_snr"; the model takes it
        # the seeded values as float32 numbers, the precision the weights are stored and tested in
        net.load_state_dict({k: v.to(torch.float32).double() for k, v in net.state_dict().items()})
        batch, lens = K.tfm_batch(name)
        record("tfm/%s/" % name, net, batch, lens, c["training"])
    floor = []
    for name, c in K.BFN_CASES.items():
        net = SW.fill_parameters(BeamformerNet(**c["conf"]), salt=c["salt"]).double()
        net.load_state_dict({k: v.to(torch.float32).double() for k, v in net.state_dict().items()})
        batch, lens = K.bfn_batch(name)
        record("bfn/%s/" % name, net, batch, lens, True)
        net.train()
        _, _, masks = net(batch["speech_mix"].double(), torch.as_tensor(lens))
        floor.append(min(float(v[v > 0].min()) for v in masks.values()))
    # the reference's clamp(min=1e-6) of the masks sits in DNN_Beamformer.forward only; the masks stay far above it anyway
    print("smallest predicted beamformer mask: %.3g" % min(floor))
    assert min(floor) > 1e-6
    path = os.path.join(args.out, "enh.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
