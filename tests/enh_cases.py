"""Seeded inputs shared by tools/gen_golden_enh.py (which records the reference on them) and tests/test_enh.py,
tests/test_gpu_enh.py.  Everything is float32-valued; complex arrays carry a trailing (re, im) axis."""
import functools
import itertools

import numpy as np
import torch

LABELS = ("IBM", "IRM", "IAM", "PSM", "NPSM", "PSM^2")

# the inverse STFT: one frame; a length that is no multiple of the hop; a hop that does not divide n_fft; win_length < n_fft;
# center both ways; hop = n_fft / 4; 16 overlapping frames (the kernel's cap); normalized; two-sided; zeros up to `length`
ISTFT_CASES = {
    "hop_quarter": dict(n_fft=64, hop=16, win_length=None, center=True, normalized=False, onesided=True, T=9, length=None),
    "one_frame": dict(n_fft=32, hop=8, win_length=None, center=False, normalized=False, onesided=True, T=1, length=None),
    "one_frame_center": dict(n_fft=32, hop=8, win_length=None, center=True, normalized=False, onesided=True, T=1, length=10),
    "odd_hop": dict(n_fft=48, hop=20, win_length=None, center=True, normalized=False, onesided=True, T=7, length=101),
    "short_window": dict(n_fft=32, hop=8, win_length=24, center=True, normalized=False, onesided=True, T=6, length=37),
    "no_center": dict(n_fft=32, hop=8, win_length=None, center=False, normalized=False, onesided=True, T=5, length=None),
    "cap16": dict(n_fft=64, hop=4, win_length=None, center=True, normalized=False, onesided=True, T=20, length=70),
    "normalized": dict(n_fft=32, hop=8, win_length=None, center=True, normalized=True, onesided=True, T=4, length=None),
    "twosided": dict(n_fft=32, hop=8, win_length=None, center=True, normalized=False, onesided=False, T=4, length=21),
    "zeros_to_length": dict(n_fft=32, hop=8, win_length=None, center=True, normalized=False, onesided=True, T=5, length=60),
}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(fn):
    """the inputs are float32 numbers whatever the caller's default dtype is (the generator tool runs in float64)"""
    @functools.wraps(fn)
    def run(*a, **k):
        keep = torch.get_default_dtype()
        torch.set_default_dtype(torch.float32)
        try:
            return fn(*a, **k)
        finally:
            torch.set_default_dtype(keep)
    return run


@_f32
def istft_input(name, B=2):
    c = ISTFT_CASES[name]
    F = c["n_fft"] // 2 + 1 if c["onesided"] else c["n_fft"]
    return torch.randn(B, c["T"], F, 2, generator=_gen(100 + sorted(ISTFT_CASES).index(name))).numpy()


@_f32
def label_input(B=2, T=6, F=17, S=3):
    """(mix [B,T,F,2], refs [S,B,T,F,2]); utterance 1 ends in exact-zero frames, and one frame of the mixture is zero
    under non-zero references"""
    g = _gen(7)
    refs = torch.randn(S, B, T, F, 2, generator=g) * torch.tensor([1.0, 0.6, 0.3])[:, None, None, None, None]
    mix = refs.sum(0) + 0.2 * torch.randn(B, T, F, 2, generator=g)
    refs[:, 1, 4:] = 0
    mix[1, 4:] = 0
    mix[0, 2] = 0
    return mix.numpy(), refs.numpy()


def planted(S, B, b):
    """the permutation planted in utterance b"""
    perms = list(itertools.permutations(range(S)))
    return perms[(5 * b + 1) % len(perms)]


@_f32
def loss_inputs(S, B=3):
    """kind -> (ref [S,B,...], inf [S,B,...], criterion name): the estimates are the references under a permutation that
    differs per utterance, plus noise, so that the best permutation is well separated"""
    out = {}
    shapes = {"mask": ((5, 17), False, "mse"), "mask4d": ((3, 4, 9), False, "mse"), "magnitude": ((5, 17), True, "mse"),
              "spectrum": ((5, 17), True, "mse"), "spectrum4d": ((3, 4, 9), True, "mse"), "si_snr": ((203,), False, "si_snr"),
              "si_snr_zeromean": ((203,), False, "si_snr_zeromean")}
    for i, (kind, (inner, cplx, crit)) in enumerate(shapes.items()):
        g = _gen(1000 + 10 * S + i)
        shape = (S, B) + inner + ((2,) if cplx else ())
        ref = torch.rand(shape, generator=g) if kind.startswith("mask") else torch.randn(shape, generator=g)
        if kind.startswith("si_snr"):
            ref = ref + 0.3                                       # a mean for the zero-mean criterion to remove
        inf = torch.empty(shape)
        for b in range(B):
            for s, t in enumerate(planted(S, B, b)):
                inf[t, b] = ref[s, b]
        inf = inf + 0.3 * torch.randn(shape, generator=g)
        out[kind] = (ref.numpy(), inf.numpy(), crit)
    return out


# ---- models --------------------------------------------------------------------------------------------------------------
_TFM = dict(n_fft=32, hop_length=8, layer=2, unit=8)
TFM_CASES = {
    "mask_irm": dict(conf=dict(_TFM, num_spk=2, mask_type="IRM", loss_type="mask_mse"), lens=(200, 157), salt=301, training=True),
    "mask_psm_tanh_mvn": dict(conf=dict(_TFM, num_spk=2, nonlinear="tanh", utt_mvn=True, mask_type="PSM", loss_type="mask_mse"),
                              lens=(200, 157), salt=302, training=True),
    "magnitude": dict(conf=dict(_TFM, num_spk=2, loss_type="magnitude"), lens=(200, 200), salt=303, training=True),
    "spectrum_s3": dict(conf=dict(_TFM, num_spk=3, nonlinear="relu", loss_type="spectrum"), lens=(200, 157), salt=304,
                        training=True),
    "spectrum_eval": dict(conf=dict(_TFM, num_spk=2, loss_type="spectrum"), lens=(200, 157), salt=305, training=False),
    "si_snr": dict(conf=dict(_TFM, num_spk=2, loss_type="spectrum"), loss_type="si_snr", lens=(200, 157), salt=306, training=True),
}
_BFN = dict(n_fft=32, hop_length=8, blayers=1, bunits=8, bprojs=8, badim=8, mask_type="PSM^2", loss_type="mask_mse")
BFN_CASES = {
    "mvdr_ref0": dict(conf=dict(_BFN, ref_channel=0), lens=(200, 157), salt=311, C=3),
    "mvdr_attention": dict(conf=dict(_BFN, ref_channel=-1), lens=(200, 157), salt=312, C=3),
}


def _signals(n, B, L, C, g):
    """n smooth sources per utterance [n, B, L(, C)]"""
    shape = (n, B, L) + ((C,) if C else ())
    x = torch.randn(shape, generator=g)
    k = torch.tensor([0.25, 0.5, 0.25])
    flat = x.movedim(2, -1).reshape(-1, 1, L)
    sm = torch.nn.functional.conv1d(flat, k[None, None], padding=1).reshape(x.movedim(2, -1).shape).movedim(-1, 2)
    gains = torch.tensor([1.0, 0.7, 0.45])[:n].reshape((n,) + (1,) * (x.dim() - 1))
    return (0.5 * x + sm) * gains


@_f32
def tfm_batch(name):
    c = TFM_CASES[name]
    S, lens = c["conf"]["num_spk"], c["lens"]
    g = _gen(c["salt"])
    refs = _signals(S, len(lens), max(lens), 0, g)
    mix = refs.sum(0) + 0.05 * torch.randn(len(lens), max(lens), generator=g)
    for b, n in enumerate(lens):
        refs[:, b, n:] = 0
        mix[b, n:] = 0
    batch = {"speech_mix": mix}
    batch.update({"speech_ref%d" % (s + 1): refs[s] for s in range(S)})
    return batch, list(lens)


@_f32
def bfn_batch(name):
    c = BFN_CASES[name]
    lens, C = c["lens"], c["C"]
    g = _gen(c["salt"])
    src = _signals(2, len(lens), max(lens), C, g)
    mix = src.sum(0)
    for b, n in enumerate(lens):
        src[:, b, n:] = 0
        mix[b, n:] = 0
    return {"speech_mix": mix, "speech_ref1": src[0], "noise_ref1": src[1]}, list(lens)


def as_np(batch):
    return {k: np.asarray(v) for k, v in batch.items()}
