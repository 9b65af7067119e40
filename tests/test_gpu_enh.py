"""Speech enhancement training on the GPU: the kernels of csrc/enh.hip and ops.istft element-wise against the float64
restatement (tests/enh_restatement.py, pinned to the reference's recorded output by tests/test_enh.py), and
ESPnetEnhancementModel over TFMaskingNet and BeamformerNet against the fixture recorded from the reference.

Bound.  Every quantity is bounded by 4 times the error that the restatement itself makes when it runs in float32 on the CPU
on the same inputs (4x: this project's margin for a differently ordered evaluation), in the measure
max |a - ref| / max |ref|.  test_enh.py keeps that float32 error below 1e-3 and above 0, so the bound is never vacuous.  No
bound is taken from the kernels.  Every kernel output is pre-filled with NaN, and a second launch must give the same bits.
Observed ratios on an MI355X: see the docstrings."""
import itertools

import numpy as np
import pytest
import torch

import enh_cases as K
import enh_restatement as E
from conftest import load_golden
from test_gpu_beamformer import nan_like, within_4x, worst_of

gpu = pytest.mark.gpu
DEV = "cuda"
CHUNK = 4096                       # ops.ENH_CHUNK: inner sizes sit one below and one above one and two chunks
_CACHE = {}


def dtypes(double):
    return (torch.float64, torch.complex128) if double else (torch.float32, torch.complex64)


def cached(key, run):
    if key not in _CACHE:
        _CACHE[key] = (run(True), run(False))
    return _CACHE[key]


def nan64(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float64)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- inputs and their restated results -----------------------------------------------------------------------------------
def istft_case(name):
    c = K.ISTFT_CASES[name]
    spec = torch.from_numpy(K.istft_input(name))
    length = c["length"]
    n_out = length if length is not None else c["hop"] * (c["T"] - 1) + c["n_fft"] - (2 * (c["n_fft"] // 2) if c["center"] else 0)
    gw = torch.randn(spec.shape[0], n_out, generator=gen(11))

    def run(double):
        rdt, _ = dtypes(double)
        s = spec.to(rdt).clone().requires_grad_(True)
        wav = E.istft(torch.view_as_complex(s), c["n_fft"], c["hop"], c["win_length"], None, c["center"], c["normalized"],
                      c["onesided"], length)
        (wav * gw.to(rdt)).sum().backward()
        return dict(wav=wav.detach(), dspec=s.grad)
    return spec, gw, run


ROUND_TRIPS = {"hann": (64, 16, None), "hann_odd_hop": (48, 20, None), "hann_short_window": (32, 8, 24), "reference": (64, 16, None)}


def round_trip_case(name):
    """a waveform through the forward STFT (Hann analysis) and back: with the Hann synthesis window (the true inverse), and
    "reference": with the reference's rectangular one, which halves the signal at hop = n_fft / 4"""
    n_fft, hop, win_length = ROUND_TRIPS[name]
    x = torch.randn(2, 333, generator=gen(31))
    window = None if name == "reference" else "hann"

    def run(double):
        rdt, _ = dtypes(double)
        return dict(wav=E.istft(E.stft(x.to(rdt), n_fft, hop, win_length), n_fft, hop, win_length, window, length=333))
    return x, window, run


MASK_APPLY = [(S, act) for S in (1, 2, 3) for act in ("sigmoid", "relu", "tanh")]


def mask_apply_case(S, act, B=2, T=7, F=33):
    g = gen(20 + S)
    logits = torch.randn(S, B, T, F, generator=g)
    X = torch.randn(B, T, F, 2, generator=g)
    X[1, 5:] = 0                                                    # exact-zero frames
    gm, gp = torch.randn(S, B, T, F, generator=g), torch.randn(S, B, T, F, 2, generator=g)

    def run(double):
        rdt, _ = dtypes(double)
        z = logits.to(rdt).clone().requires_grad_(True)
        m, P = E.mask_apply(z, E.cx(X.to(rdt)), act)
        ((m * gm.to(rdt)).sum() + (E.ri(P) * gp.to(rdt)).sum()).backward()
        return dict(mask=m.detach(), P=E.ri(P.detach()), dlogits=z.grad)
    return logits, X, gm, gp, run


# inner shapes (T, [C,] F): one frame; n one below one chunk of 4096, one chunk exactly, one above; one below two chunks
# (8191 is prime: one bin per frame) and one above; 4-D with C = 1 and with C = 4 across a chunk boundary
TF_SHAPES = ((1, 9), (45, 91), (64, 64), (17, 241), (8191, 1), (3, 2731), (7, 1, 33), (8, 4, 129))
TF_KINDS = [("mask", lab) for lab in K.LABELS] + [("magnitude", None), ("spectrum", None), ("real", None)]


def tf_case(kind, label, S, shape, act="sigmoid", B=3):
    """references, a mixture with exact-zero frames (the tail of the shorter utterances), estimates that carry a planted
    permutation per utterance, and a cotangent per utterance"""
    g = gen(1000 * S + 10 * len(shape) + shape[0])
    T = shape[0]
    lens = [T, max(1, (2 * T) // 3), max(1, T // 2)]
    refs = torch.randn((S, B) + shape + (2,), generator=g) * torch.tensor([1.0, 0.6, 0.35])[:S].view((S,) + (1,) * (len(shape) + 2))
    mix = refs.sum(0) + 0.1 * torch.randn((B,) + shape + (2,), generator=g)
    for b, n in enumerate(lens):
        refs[:, b, n:] = 0
        mix[b, n:] = 0
    cot = torch.rand(B, generator=g) + 0.5
    if kind == "mask":
        lab = torch.stack(E.mask_label(E.cx(mix), [E.cx(r) for r in refs], label)).float()
        target = torch.logit(lab.clamp(0.05, 0.95)) if act == "sigmoid" else lab
    elif kind == "real":
        target = refs[..., 0].clone()
    else:
        target = refs.clone()
    est = torch.empty_like(target)
    for b in range(B):
        for s, t in enumerate(K.planted(S, B, b)):
            est[t, b] = target[s, b]
    est = est + 0.2 * torch.randn(est.shape, generator=g)
    if kind in ("magnitude", "spectrum"):
        est[:, 1, lens[1]:] = 0                                     # an estimate that is exactly zero: |P| at 0

    def run(double):
        rdt, _ = dtypes(double)
        e = est.to(rdt).clone().requires_grad_(True)
        if kind == "mask":
            ref = E.mask_label(E.cx(mix.to(rdt)), [E.cx(r.to(rdt)) for r in refs], label)
            inf, crit = list(E.ACTS[act](e)), E.tf_mse_loss
        elif kind == "real":
            ref, inf, crit = list(refs[..., 0].to(rdt)), list(e), E.tf_mse_loss
        else:
            ref, inf = [E.cx(r.to(rdt)) for r in refs], [torch.view_as_complex(v) for v in e]
            crit = E.mag_mse_loss if kind == "magnitude" else E.tf_mse_loss
        pair = E.pair_matrix(ref, inf, crit)
        loss, perm = E.permutation_loss(ref, inf, crit)
        if double:                                                  # rounding must not be able to flip a compared pick
            assert E.permutation_gap(ref, inf, crit) >= 1e-3, (kind, label, S, shape)
        (loss * cot.to(rdt)).sum().backward()
        return dict(pair=pair.detach(), loss=loss.detach(), perm=perm, dest=e.grad)
    return refs, mix, est, cot, run


SNR_LENGTHS = (203, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK + 1)
SNR_CASES = [(L, 0.3) for L in SNR_LENGTHS] + [(CHUNK + 1, 1e-3)]      # the last one: 60 dB


def snr_case(S, L, zeromean, noise=0.3, B=3):
    g = gen(7000 + 10 * S + L % 97)
    ref = torch.randn(S, B, L, generator=g) + 0.3
    est = torch.empty_like(ref)
    for b in range(B):
        for s, t in enumerate(K.planted(S, B, b)):
            est[t, b] = ref[s, b]
    est = est + noise * torch.randn(ref.shape, generator=g)
    ref[:, 1, (2 * L) // 3:] = 0                                    # unequal lengths: the sums run over the padding too
    cot = torch.rand(B, generator=g) + 0.5
    crit = E.si_snr_loss_zeromean if zeromean else E.si_snr_loss

    def run(double):
        rdt, _ = dtypes(double)
        e = est.to(rdt).clone().requires_grad_(True)
        r = list(ref.to(rdt))
        pair = E.pair_matrix(r, list(e), crit)
        loss, perm = E.permutation_loss(r, list(e), crit)
        if double:
            assert E.permutation_gap(r, list(e), crit) >= 1e-3, (S, L, zeromean, noise)
        (loss * cot.to(rdt)).sum().backward()
        return dict(pair=pair.detach(), loss=loss.detach(), perm=perm, dest=e.grad)
    return ref, est, cot, run


def model_run(golden, kind, name):
    import test_enh as TE

    def run(double):
        rdt = dtypes(double)[0]
        if kind == "tfm":
            out, sd = TE.restated_tfm(golden, name, rdt)
        else:
            c, p = K.BFN_CASES[name], "bfn/%s/" % name
            sd = {k[len("beamformer."):]: v for k, v in TE._sd(golden, p, rdt).items()}
            b = {k: torch.from_numpy(golden[p + "in/" + k]).to(rdt) for k in ("speech_mix", "speech_ref1", "noise_ref1")}
            out = E.beamformer_model(sd, b["speech_mix"], list(c["lens"]), b["speech_ref1"], b["noise_ref1"], c["conf"])
            out["loss"].backward()
        res = dict(loss=out["loss"].detach().reshape(1))
        if out.get("si_snr") is not None:
            res["si_snr"] = out["si_snr"].reshape(1)
        res.update({"grad/" + k: v.grad for k, v in sd.items() if v.grad is not None})
        return res
    return run


def restated_cases():
    """(key, run(double) -> dict of tensors) for every input of this file: test_enh.py holds the float32 restatement's
    error on them below 1e-3"""
    for name in K.ISTFT_CASES:
        yield "istft/" + name, istft_case(name)[-1]
    for name in ROUND_TRIPS:
        yield "round_trip/" + name, round_trip_case(name)[-1]
    for S, act in MASK_APPLY:
        yield "mask_apply/%d%s" % (S, act), mask_apply_case(S, act)[-1]
    for (kind, label), S, shape in itertools.product(TF_KINDS, (1, 2, 3), TF_SHAPES):
        yield "pair_%s/%s/%d/%s" % (kind, label, S, shape), tf_case(kind, label, S, shape)[-1]
    for S, (L, noise), zm in itertools.product((1, 2, 3), SNR_CASES, (True, False)):
        yield "sisnr/%d/%d/%s/%g" % (S, L, zm, noise), snr_case(S, L, zm, noise)[-1]
    golden = load_golden("enh.npz")
    for name in K.TFM_CASES:
        yield "tfm/" + name, model_run(golden, "tfm", name)
    for name in K.BFN_CASES:
        yield "bfn/" + name, model_run(golden, "bfn", name)


def same_bits(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- kernels -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", K.ISTFT_CASES)
def test_inverse_stft(name):
    """Stft.inverse (one GEMM + eamd_istft_ola) and its backward (eamd_istft_ola_bwd + one GEMM on overlapping rows):
    the waveform and the spectrum's gradient within 4x the float32 restatement's error; zeros from the end of the signal
    up to `length`; the imaginary parts of DC and Nyquist get exactly no gradient; the same bits on a second run.
    MI355X, error / float32-restatement error (the bound is 4): waveform <= 0.09, the kernel alone <= 0.13, spectrum
    gradient <= 0.06; largest errors 2.2e-7 (waveform) and 3.0e-7 (gradient) of the largest element."""
    from espnet_amd import ops
    from espnet_amd.espnet2.frontend import Stft
    c = K.ISTFT_CASES[name]
    spec, gw, run = istft_case(name)
    r64, r32 = cached("istft/" + name, run)
    st = Stft(c["n_fft"], c["win_length"], c["hop"], center=c["center"], normalized=c["normalized"], onesided=c["onesided"])
    B, T = spec.shape[:2]
    N, hop, length = c["n_fft"], c["hop"], gw.shape[1]

    def launch():
        s = spec.to(DEV).requires_grad_(True)
        wav, _ = st.inverse(s, None if c["length"] is None else [c["length"]] * B)
        wav.backward(gw.to(DEV))
        # the two kernels by themselves, into NaN
        inv, bwd, w, _ = st.inverse_basis(DEV)
        frames = (s.detach().view(B * T, -1) @ inv.t()).view(B, T, N)
        wav2 = ops.istft_ola(frames.contiguous(), w, hop, c["center"], length, out=nan_like(B, length))
        g = ops.istft_ola_bwd(gw.to(DEV), w, T, hop, c["center"], out=nan_like(B * ops.istft_rows(T, N, hop) * hop + N))
        return wav.detach(), s.grad, wav2, g
    got, again = launch(), launch()
    torch.cuda.synchronize()
    same_bits(got, again)
    wav, dspec, wav2, g = got
    assert torch.isfinite(g).all() and float(g[-N:].abs().max()) == 0.0
    report = []
    within_4x("wav", wav.cpu(), r64["wav"], r32["wav"], report)
    within_4x("wav (kernel alone)", wav2.cpu(), r64["wav"], r32["wav"], report)
    within_4x("dspec", dspec.cpu(), r64["dspec"], r32["dspec"], report)
    assert float(dspec[:, :, 0, 1].abs().max()) == 0.0
    if N % 2 == 0:
        assert float(dspec[:, :, N // 2, 1].abs().max()) == 0.0
    if name == "zeros_to_length":
        assert float(wav[:, 48:].abs().max()) == 0.0 and float(wav[:, :48].abs().min()) > 0
    print("[enh] istft %s: " % name + "; ".join(t for _, t in report))


@gpu
@pytest.mark.parametrize("name", ROUND_TRIPS)
def test_inverse_of_the_forward_stft(name):
    """Stft.inverse(Stft.forward(x), window="hann") gives x back (the true inverse, one argument away), and without a window,
    as the reference, 0.5 x at hop = n_fft / 4: against the float64 restatement's round trip, within 4x the float32 one's error"""
    from espnet_amd.espnet2.frontend import Stft
    n_fft, hop, win_length = ROUND_TRIPS[name]
    x, window, run = round_trip_case(name)
    r64, r32 = cached("round_trip/" + name, run)
    st = Stft(n_fft, win_length, hop)
    spec, _ = st(x.to(DEV))
    wav, _ = st.inverse(spec, [333, 333], window=window)
    torch.cuda.synchronize()
    report = []
    within_4x("wav", wav.cpu(), r64["wav"], r32["wav"], report)
    if window is None:
        assert E.err_vs(r64["wav"][:, 64:-64], 0.5 * x.double()[:, 64:-64]) < 1e-12      # what the device is held to, above
    else:
        assert E.err_vs(r64["wav"], x.double()) < 1e-12
    print("[enh] round trip %s: " % name + "; ".join(t for _, t in report))


@gpu
def test_inverse_stft_refuses_more_than_16_overlaps():
    from espnet_amd import _lib
    from espnet_amd.espnet2.frontend import Stft
    with pytest.raises(_lib.EamdError, match="64/3"):
        Stft(64, None, 3).inverse(torch.zeros(1, 30, 33, 2, device=DEV))
    L = _lib.lib()
    t = torch.zeros(4096, device=DEV)
    assert L.eamd_istft_ola(t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 4, 64, 3, 1, 40, None) == _lib.EAMD_EUNSUPPORTED


@gpu
@pytest.mark.parametrize("S,act", MASK_APPLY)
def test_mask_apply(S, act):
    """eamd_enh_mask_apply / _bwd: masks, masked spectra and the logit gradient, finite on exact-zero frames (where the
    spectra and their share of the gradient are exactly 0).
    MI355X, worst ratio: masks 2.4 (tanh, 7.3e-8 against 3.0e-8), 1.0 (sigmoid), relu exact; spectra 0.85; logit gradient 1.1."""
    from espnet_amd import ops
    logits, X, gm, gp, run = mask_apply_case(S, act)
    r64, r32 = cached("mask_apply/%d%s" % (S, act), run)
    a = ops.ENH_ACTS[act]

    def launch():
        m, P = ops.enh_mask_apply(logits.to(DEV), X.to(DEV), a, out=(nan_like(*logits.shape), nan_like(*logits.shape, 2)))
        dl = ops.enh_mask_apply_bwd(logits.to(DEV), X.to(DEV), gm.to(DEV), gp.to(DEV), a, out=nan_like(*logits.shape))
        m_only, none = ops.enh_mask_apply(logits.to(DEV), None, a, out=(nan_like(*logits.shape), None))
        dl_m = ops.enh_mask_apply_bwd(logits.to(DEV), None, gm.to(DEV), None, a, out=nan_like(*logits.shape))
        assert none is None
        return m, P, dl, m_only, dl_m
    got, again = launch(), launch()
    torch.cuda.synchronize()
    same_bits(got, again)
    m, P, dl, m_only, dl_m = got
    assert torch.equal(m, m_only) and float(P[:, 1, 5:].abs().max()) == 0.0 and torch.isfinite(dl_m).all()
    report = []
    within_4x("mask", m.cpu(), r64["mask"], r32["mask"], report)
    within_4x("P", P.cpu(), r64["P"], r32["P"], report)
    within_4x("dlogits", dl.cpu(), r64["dlogits"], r32["dlogits"], report)
    print("[enh] mask_apply S=%d %s: " % (S, act) + "; ".join(t for _, t in report))


def check_pick(pair, r64, forced_ok=True):
    """eamd_enh_pit_pick on a pair matrix from the device: the restated permutation, and the loss under a forced one"""
    from espnet_amd import ops
    B, S, _ = pair.shape
    loss, perm = ops.enh_pit_pick(pair, out=(nan_like(B), torch.full((B,), -1, device=DEV, dtype=torch.int64)))
    assert perm.cpu().tolist() == r64["perm"].tolist()
    nperm = len(list(itertools.permutations(range(S))))
    forced = torch.tensor([(k + 1) % nperm for k in r64["perm"].tolist()], device=DEV)
    lf, pf = ops.enh_pit_pick(pair, forced, out=(nan_like(B), torch.full((B,), -1, device=DEV, dtype=torch.int64)))
    want = E.permutation_losses(pair.cpu())[torch.arange(B), forced.cpu()]
    assert torch.equal(pf, forced) and float((lf.cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    return loss, perm


@gpu
@pytest.mark.parametrize("S", (1, 2, 3))
@pytest.mark.parametrize("kind,label", TF_KINDS, ids=[k if lab is None else lab for k, lab in TF_KINDS])
def test_pair_tf(kind, label, S):
    """eamd_enh_pair_tf, eamd_enh_pit_pick and eamd_enh_pair_tf_bwd over the inner shapes TF_SHAPES (one frame; 4095, 4096
    and 4097 around one chunk of 4096; 8191 and 8193 around two; 4-D with C = 1 and C = 4): the pair matrix, the loss and the estimate's gradient within
    4x the float32 restatement's error, the permutation equal; labels and gradients finite on exact-zero frames; the
    magnitude gradient exactly 0 where the estimate is 0; the same bits on a second launch.
    MI355X, worst ratio over the grid: 2.0 (IAM, S = 1, n = 9, the pair matrix: 7.8e-7 against 3.9e-7)."""
    from espnet_amd import ops
    mode = {"mask": ops.ENH_MASK, "magnitude": ops.ENH_MAG, "spectrum": ops.ENH_SPEC, "real": ops.ENH_REAL}[kind]
    lab = ops.ENH_LABELS[label] if label else 0
    act = ops.ENH_ACTS["sigmoid" if kind == "mask" else "none"]
    report = []
    for shape in TF_SHAPES:
        refs, mix, est, cot, run = tf_case(kind, label, S, shape)
        r64, r32 = cached("pair_%s/%s/%d/%s" % (kind, label, S, shape), run)
        ref_d = (refs[..., 0].contiguous() if kind == "real" else refs).to(DEV)
        mix_d = mix.to(DEV) if kind == "mask" else None
        est_d, B = est.to(DEV), est.shape[1]

        def launch():
            pair = ops.enh_pair_tf(est_d, ref_d, mix_d, mode, lab, act, out=nan64(B, S, S))
            loss, perm = check_pick(pair, r64)
            dest = ops.enh_pair_tf_bwd(est_d, ref_d, mix_d, perm, cot.to(DEV), mode, lab, act, out=nan_like(*est.shape))
            return pair, loss, dest
        got, again = launch(), launch()
        torch.cuda.synchronize()
        same_bits(got, again)
        pair, loss, dest = got
        tag = "%s n=%d " % (label or kind, int(np.prod(shape)))
        within_4x(tag + "pair", pair.cpu(), r64["pair"], r32["pair"], report)
        within_4x(tag + "loss", loss.cpu(), r64["loss"], r32["loss"], report)
        within_4x(tag + "dest", dest.cpu(), r64["dest"], r32["dest"], report)
        if kind == "magnitude":
            n1 = max(1, (2 * shape[0]) // 3)
            assert n1 == shape[0] or float(dest[:, 1, n1:].abs().max()) == 0.0
    print("[enh] pair_tf %s S=%d: " % (label or kind, S) + worst_of(report))
    print("[enh] pair_tf %s S=%d, C = 1: " % (label or kind, S) + worst_of([r for r in report if " n=231 " in r[1]]))


@gpu
@pytest.mark.parametrize("zeromean", (True, False), ids=("zeromean", "l2norm"))
@pytest.mark.parametrize("S", (1, 2, 3))
def test_pair_sisnr(S, zeromean):
    """eamd_enh_pair_sisnr (+ pick) and _bwd over L = 203, 4095, 4096, 4097, 8191, 8193 and, at 60 dB (noise 1e-3), L = 4097: both
    criteria from the fp64 sums in closed form, within 4x the float32 restatement's error (which at 60 dB is the
    cancellation the fp64 sums avoid); unequal lengths, the sums run over the padding.
    MI355X, worst ratio: 1.0 (a loss rounded to float32 where the float32 restatement rounds the same way), typically 0.5;
    with the pair matrix kept in float32 the S = 2 zero-mean loss at L = 203 was at 3.97, which is why it stays fp64."""
    from espnet_amd import ops
    mode = ops.ENH_SNR_ZEROMEAN if zeromean else ops.ENH_SNR_L2NORM
    report = []
    for L, noise in SNR_CASES:
        ref, est, cot, run = snr_case(S, L, zeromean, noise)
        r64, r32 = cached("sisnr/%d/%d/%s/%g" % (S, L, zeromean, noise), run)
        B = ref.shape[1]
        NV = 4 * S + S * S

        def launch():
            pair, sums = ops.enh_pair_sisnr(est.to(DEV), ref.to(DEV), mode,
                                            out=(nan64(B, S, S), nan64(B, NV)))
            loss, perm = check_pick(pair, r64)
            dest = ops.enh_pair_sisnr_bwd(est.to(DEV), ref.to(DEV), sums, perm, cot.to(DEV), mode, out=nan_like(S, B, L))
            return pair, sums, loss, dest
        got, again = launch(), launch()
        torch.cuda.synchronize()
        same_bits(got, again)
        pair, sums, loss, dest = got
        assert torch.isfinite(sums).all()
        tag = "L=%d noise=%g " % (L, noise)
        within_4x(tag + "pair", pair.cpu(), r64["pair"], r32["pair"], report)
        within_4x(tag + "loss", loss.cpu(), r64["loss"], r32["loss"], report)
        within_4x(tag + "dest", dest.cpu(), r64["dest"], r32["dest"], report)
    print("[enh] pair_sisnr S=%d %s: " % (S, "zeromean" if zeromean else "l2norm") + worst_of(report))


@gpu
def test_unsupported_speaker_counts_are_refused():
    from espnet_amd import _lib, ops
    with pytest.raises(_lib.EamdError, match="speakers"):
        ops.enh_pit_pick(torch.zeros(2, 4, 4, device=DEV, dtype=torch.float64))
    with pytest.raises(_lib.EamdError, match="speakers"):
        ops.enh_pair_sisnr(torch.zeros(4, 2, 50, device=DEV), torch.zeros(4, 2, 50, device=DEV))


# ---- models --------------------------------------------------------------------------------------------------------------
def _model_check(tag, m, loss, stats, golden, p, r32, prefix=""):
    report = []
    ref = {k: torch.from_numpy(np.asarray(v)).reshape(-1) if k in ("loss", "si_snr") else torch.from_numpy(v)
           for k, v in ((k[len(p):], v) for k, v in golden.items() if k.startswith(p)) if k in ("loss", "si_snr") or k.startswith("grad/")}
    within_4x("loss", loss.detach().reshape(1).cpu(), ref["loss"], r32["loss"], report)
    if "si_snr" in ref:
        within_4x("si_snr", stats["si_snr"].reshape(1).cpu(), ref["si_snr"], r32["si_snr"], report)
    else:
        assert stats["si_snr"] is None or m.loss_type == "si_snr"
    grads = {k[5:]: v for k, v in ref.items() if k.startswith("grad/")}
    gmax = max([float(v.abs().max()) for v in grads.values()] or [0.0])
    for k, par in m.enh_model.named_parameters():
        if k not in grads or float(grads[k].abs().max()) <= 1e-12 * gmax:
            assert par.grad is None or float(par.grad.abs().max()) <= 1e-6 * gmax, k
            continue
        assert par.grad is not None, k
        within_4x("d" + k, par.grad.cpu(), grads[k], r32["grad/" + k[len(prefix):]], report)
    print("[enh] %s: " % tag + worst_of(report))


@gpu
@pytest.mark.parametrize("name", K.TFM_CASES)
def test_tf_masking_model_against_the_reference(name):
    """ESPnetEnhancementModel(TFMaskingNet), the weights and batch of the fixture: loss, the chosen permutation, the
    eval-mode SI-SNR statistic (through Stft.inverse under the TF loss's permutation) and every parameter gradient
    against the reference's float64 record, within 4x the float32 restatement's error.
    MI355X, worst ratio: 2.6 (rnn.l_last.bias of spectrum_s3, 8.5e-8 against 3.3e-8), 1.8 (a recurrent bias, same case), 1.2
    (magnitude); losses 0.05 to 0.8, the eval-mode SI-SNR statistic 0.27."""
    from espnet_amd.espnet2.enh import ESPnetEnhancementModel, TFMaskingNet
    golden = load_golden("enh.npz")
    c, p = K.TFM_CASES[name], "tfm/%s/" % name
    _, r32 = cached("tfm/" + name, model_run(golden, "tfm", name))
    net = TFMaskingNet(**c["conf"])
    net.load_state_dict({k[len(p) + 3:]: torch.from_numpy(v) for k, v in golden.items() if k.startswith(p + "sd/")})
    net.loss_type = c.get("loss_type", net.loss_type)
    m = ESPnetEnhancementModel(net).to(DEV).train(c["training"])
    batch = {k[len(p) + 3:]: torch.from_numpy(v).to(DEV) for k, v in golden.items() if k.startswith(p + "in/")}
    loss, stats, weight = m(batch.pop("speech_mix"), torch.tensor(c["lens"]), **batch)
    if c["training"]:
        loss.backward()
    torch.cuda.synchronize()
    assert int(weight) == len(c["lens"]) and m.last_perm.cpu().tolist() == golden[p + "perm"].tolist()
    assert float(stats["loss"]) == float(loss.detach())
    _model_check("TFMaskingNet " + name, m, loss, stats, golden, p, r32)


@gpu
@pytest.mark.parametrize("name", K.BFN_CASES)
def test_beamformer_model_against_the_reference(name):
    """ESPnetEnhancementModel(BeamformerNet("mvdr")), training with mask_mse on PSM^2 labels: the speech-mask plus the
    noise-mask term and the mask estimator's gradients against the reference's float64 record; in eval mode the beamformer
    runs, the statistic is finite, the enhanced spectrum is bit for bit that of DNN_Beamformer.forward on the same spectrum
    and the masks are those of DNN_Beamformer.predict_mask.
    MI355X, worst ratio: 1.0 (loss, attention reference), 0.7 (mask.linears.1.weight, fixed reference channel)."""
    from espnet_amd.espnet2.enh import BeamformerNet, ESPnetEnhancementModel
    golden = load_golden("enh.npz")
    c, p = K.BFN_CASES[name], "bfn/%s/" % name
    _, r32 = cached("bfn/" + name, model_run(golden, "bfn", name))
    net = BeamformerNet(**c["conf"])
    missing = net.load_state_dict({k[len(p) + 3:]: torch.from_numpy(v) for k, v in golden.items() if k.startswith(p + "sd/")},
                                  strict=False)
    assert not missing.unexpected_keys and all(k.startswith("beamformer.ref.") for k in missing.missing_keys)
    m = ESPnetEnhancementModel(net).to(DEV).train()
    batch = {k[len(p) + 3:]: torch.from_numpy(v).to(DEV) for k, v in golden.items() if k.startswith(p + "in/")}
    mix = batch.pop("speech_mix")
    loss, stats, weight = m(mix, torch.tensor(c["lens"]), **batch)
    loss.backward()
    torch.cuda.synchronize()
    _model_check("BeamformerNet " + name, m, loss, stats, golden, p, r32, prefix="beamformer.")
    m.eval()
    with torch.no_grad():
        loss_e, stats_e, _ = m(mix, torch.tensor(c["lens"]), **batch)
        enhanced, flens, masks = net(mix, torch.tensor(c["lens"]))
        wav, _, _ = net.forward_rawwav(mix, torch.tensor(c["lens"]))
        spec, fl = net.stft(mix, torch.tensor(c["lens"]))
        direct = net.beamformer(spec, fl)[0]
        pm, _ = net.beamformer.predict_mask(spec, fl)
    assert torch.isfinite(stats_e["si_snr"]) and torch.isfinite(loss_e)
    assert torch.equal(enhanced, direct)                            # the same kernels on the same spectrum: the same bits
    assert len(pm) == 2 and torch.equal(pm[0], masks["spk1"]) and torch.equal(pm[1], masks["noise1"])
    assert enhanced.shape == (2, 26, 17, 2) and wav.shape == (2, 200) and list(masks) == ["spk1", "noise1"]
    assert masks["spk1"].shape == (2, 26, 3, 17) and flens.tolist() == [26, 20]


@gpu
def test_predict_mask_pads_to_the_input_length():
    """DNN_Beamformer.predict_mask and BeamformerNet.forward in training mode on a batch whose longest utterance is shorter
    than the input (Tm = 19 < T = 26 frames): (B, T, C, F) masks, equal to each other, sigmoid of the restated mask
    estimator's logits up to Tm within 4x the float32 restatement's error, exact zeros from Tm on; no logits are handed on"""
    import beamformer_restatement as R
    from espnet_amd.espnet2.enh import BeamformerNet
    golden = load_golden("enh.npz")
    name = "mvdr_attention"
    c, p = K.BFN_CASES[name], "bfn/%s/" % name
    net = BeamformerNet(**c["conf"])
    net.load_state_dict({k[len(p) + 3:]: torch.from_numpy(v) for k, v in golden.items() if k.startswith(p + "sd/")})
    net = net.to(DEV).train()
    mix = torch.from_numpy(golden[p + "in/speech_mix"])
    lens = [150, 100]
    none, flens, masks = net(mix.to(DEV), torch.tensor(lens))
    spec, fl = net.stft(mix.to(DEV), torch.tensor(lens))
    pm, _ = net.beamformer.predict_mask(spec, fl)
    torch.cuda.synchronize()
    assert none is None and flens.tolist() == [19, 13] and masks.logits is None and list(masks) == ["spk1", "noise1"]
    assert pm[0].shape == (2, 26, 3, 17) and torch.equal(pm[0], masks["spk1"]) and torch.equal(pm[1], masks["noise1"])
    assert float(pm[0][:, 19:].abs().max()) == 0.0 and float(pm[1][:, 19:].abs().max()) == 0.0
    report = []

    def run(double):
        rdt, cdt = dtypes(double)
        sd = {k[len(p) + 3 + len("beamformer."):]: torch.from_numpy(v).to(rdt) for k, v in golden.items() if k.startswith(p + "sd/")}
        z = R.mask_logits(sd, E.cx(spec.cpu()).to(cdt), fl.tolist())
        return torch.stack([R.masks_full(z[s], 26) for s in range(2)])
    r64, r32 = run(True), run(False)
    within_4x("masks", torch.stack(pm).cpu(), r64, r32, report)
    print("[enh] predict_mask: " + "; ".join(t for _, t in report))
