"""Speech enhancement training on the CPU: tests/enh_restatement.py, the yardstick of csrc/enh.hip and espnet2/enh.py, against
the fixture recorded from the reference (tools/gen_golden_enh.py: Stft.inverse, the six mask labels, the permutation losses
and ESPnetEnhancementModel over TFMaskingNet and BeamformerNet, float64), its closed forms against float64 autograd, the
conditions that keep the GPU tests' bound and permutation comparisons meaningful, the C ABI's argument checks and the
public surface.  No GPU.

The tests of the inverse round trip, the 0.5 x quirk, the SI-SNR closed form, gradcheck and the magnitude gradient at zero
run tests/enh_restatement.py alone, against torch: they pin the yardstick, not the product, and would pass without the
feature's product code (the files they need are new with it).  The product is held to that yardstick in
tests/test_gpu_enh.py, the round trip through Stft.forward and Stft.inverse(window="hann") included."""
import itertools

import numpy as np
import pytest
import torch

import enh_cases as K
import enh_restatement as E
from conftest import load_golden

F64, C128 = torch.float64, torch.complex128


@pytest.fixture(scope="module")
def golden():
    return load_golden("enh.npz")


def num(v):
    """a one-element tensor or array -> float"""
    return float(np.asarray(v.detach() if torch.is_tensor(v) else v).reshape(-1)[0])


def c128(a):
    return E.cx(np.asarray(a, dtype=np.float64))


def gap_of(pair):
    """(second best - best) / |best| permutation loss of a recorded pair matrix [B,S,S], the smallest over the batch"""
    losses = E.permutation_losses(torch.as_tensor(pair))
    top = torch.sort(losses, dim=1).values
    return float(((top[:, 1] - top[:, 0]) / top[:, 0].abs()).min())


# ---- inverse STFT --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.ISTFT_CASES)
def test_inverse_stft_equals_the_reference(golden, name):
    """Stft.inverse of the reference (torch.istft without a window) in float64: 1e-10 relative.  Observed: 2e-15 or better."""
    c = K.ISTFT_CASES[name]
    spec = c128(golden["istft/%s/spec" % name])
    assert np.array_equal(golden["istft/%s/spec" % name], K.istft_input(name))
    got = E.istft(spec, c["n_fft"], c["hop"], c["win_length"], None, c["center"], c["normalized"], c["onesided"], c["length"])
    ref = torch.from_numpy(golden["istft/%s/wav" % name])
    assert got.shape == ref.shape
    e = E.err_vs(got, ref)
    print("[enh] istft %s vs the reference: %.1e" % (name, e))
    assert e < 1e-10


@pytest.mark.parametrize("n_fft,hop,win_length", [(64, 16, None), (48, 20, None), (32, 8, 24), (64, 4, None)])
def test_inverse_with_the_analysis_window_inverts_the_forward(n_fft, hop, win_length):
    x = torch.randn(2, 333, generator=torch.Generator().manual_seed(1), dtype=F64)
    spec = E.stft(x, n_fft, hop, win_length)
    back = E.istft(spec, n_fft, hop, win_length, "hann", length=333)
    assert E.err_vs(back, x) < 1e-12


def test_the_reference_inverse_halves_the_signal_at_hop_quarter():
    """no window is passed to istft: Hann analysis, rectangular synthesis, hop = n_fft / 4 -> 0.5 x (away from the edges the
    Hann windows of four frames sum to 2 and the rectangular envelope to 4)"""
    x = torch.randn(2, 320, generator=torch.Generator().manual_seed(2), dtype=F64)
    back = E.istft(E.stft(x, 64, 16), 64, 16, length=320)
    assert E.err_vs(back[:, 64:-64], 0.5 * x[:, 64:-64]) < 1e-12


def test_a_window_that_leaves_samples_uncovered_is_refused():
    spec = torch.zeros(1, 4, 17, dtype=C128)
    with pytest.raises(RuntimeError, match="window overlap add min"):
        E.istft(spec, 32, 16, 8)                                  # 8 ones in 32, hop 16: gaps
    from espnet_amd import _lib, ops
    with pytest.raises(RuntimeError, match="window overlap add min"):
        ops.istft_check(E.full_window(8, 32, None).numpy(), 4, 32, 16, True, 40)
    with pytest.raises(_lib.EamdError, match="64/3"):             # more than 16 overlapping frames
        ops.istft_check(np.ones(64), 30, 64, 3, True, 40)
    assert ops.istft_check(np.ones(64), 20, 64, 4, True, 70) == 70


def test_inverse_basis_of_the_module_is_the_restated_transform():
    """Stft.inverse_basis (host side of ops.istft) against the restatement's frames: rectangular window, every layout"""
    from espnet_amd.espnet2.frontend import Stft
    for name in ("hop_quarter", "short_window", "normalized", "twosided", "odd_hop"):
        c = K.ISTFT_CASES[name]
        st = Stft(c["n_fft"], c["win_length"], c["hop"], center=c["center"], normalized=c["normalized"], onesided=c["onesided"])
        inv, bwd, w, w_host = st.inverse_basis("cpu")
        spec = torch.from_numpy(K.istft_input(name))[:, :1].double()         # one frame
        frames = spec.reshape(2, -1) @ inv.double().T
        full = E.full_window(st.win_length, c["n_fft"], None)
        assert torch.equal(w.double(), full) and np.array_equal(w_host, full.numpy())
        assert inv.shape == (c["n_fft"], 2 * st.n_freq) and torch.allclose(bwd.double(), inv.double().T * full, atol=1e-7)
        # one frame, no centre: istft = frames * w / w^2 where w != 0
        ref = E.istft(E.cx(spec), c["n_fft"], c["hop"], c["n_fft"], None, False, c["normalized"], c["onesided"])
        assert E.err_vs(frames, ref) < 1e-6
    assert st.inverse_basis("cpu", "hann")[2].sum() > 0 and st.inverse_basis("cpu", "hann")[2][0] == 0


# ---- labels and criteria -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_type", K.LABELS)
def test_mask_labels_equal_the_reference(golden, mask_type):
    mix, refs = c128(golden["label/mix"]), [c128(r) for r in golden["label/refs"]]
    got = torch.stack(E.mask_label(mix, refs, mask_type))
    ref = torch.from_numpy(golden["label/" + mask_type]).double()
    assert torch.isfinite(got).all()                                 # the exact-zero frames included
    assert E.err_vs(got, ref) < 1e-10
    if mask_type == "NPSM":
        assert float(ref.min()) < 0                                  # clamped to [-1, 1], not [0, 1]: the reference's quirk


def _loss_case(golden, S, kind):
    p = "loss/%d/%s/" % (S, kind)
    cplx = golden[p + "ref"].shape[-1] == 2 and kind in ("magnitude", "spectrum", "spectrum4d")
    conv = (lambda a: c128(a)) if cplx else (lambda a: torch.from_numpy(a).double())
    ref, inf = [conv(v) for v in golden[p + "ref"]], [conv(v) for v in golden[p + "inf"]]
    crit = {"magnitude": E.mag_mse_loss, "si_snr": E.si_snr_loss, "si_snr_zeromean": E.si_snr_loss_zeromean}.get(kind, E.tf_mse_loss)
    return p, ref, inf, crit


@pytest.mark.parametrize("kind", ["mask", "mask4d", "magnitude", "spectrum", "spectrum4d", "si_snr", "si_snr_zeromean"])
@pytest.mark.parametrize("S", (1, 2, 3))
def test_permutation_losses_equal_the_reference(golden, S, kind):
    """pair matrix, batch loss and permutation: 1e-10, permutations equal; the golden's best and second-best permutation
    losses are at least 1e-3 apart (relative), so rounding cannot flip a pick"""
    p, ref, inf, crit = _loss_case(golden, S, kind)
    if S > 1:
        assert gap_of(golden[p + "pair"]) >= 1e-3
    pair = E.pair_matrix(ref, inf, crit)
    loss, perm = E.permutation_loss(ref, inf, crit)
    assert E.err_vs(pair, torch.from_numpy(golden[p + "pair"])) < 1e-10
    assert abs(num(loss.mean()) - num(golden[p + "loss"])) <= 1e-10 * abs(num(golden[p + "loss"]))
    assert perm.tolist() == golden[p + "perm"].tolist()
    B = len(perm)
    perms = list(itertools.permutations(range(S)))
    assert [perms[k] for k in perm.tolist()] == [K.planted(S, B, b) for b in range(B)]


@pytest.mark.parametrize("zeromean", (True, False))
def test_si_snr_closed_form(zeromean):
    """the criterion from the five sums, and d loss / d e = a e + b r + c, against the direct formula and its autograd"""
    g = torch.Generator().manual_seed(3)
    r = torch.randn(3, 157, generator=g, dtype=F64) + 0.2
    e = (r + 0.1 * torch.randn(3, 157, generator=g, dtype=F64)).requires_grad_(True)
    direct = (E.si_snr_loss_zeromean if zeromean else E.si_snr_loss)(r, e)
    direct.sum().backward()
    loss, a, b, c = E.si_snr_closed_form(E.si_snr_sums(r, e.detach()), 157, zeromean)
    assert E.err_vs(loss, direct.detach()) < 1e-10
    assert E.err_vs(a[:, None] * e.detach() + b[:, None] * r + c[:, None], e.grad) < 1e-9


def test_restated_gradients_pass_gradcheck():
    g = torch.Generator().manual_seed(4)
    spec = torch.randn(1, 3, 9, generator=g, dtype=C128)
    assert torch.autograd.gradcheck(lambda s: E.istft(torch.view_as_complex(s), 16, 4, length=10), (E.ri(spec).requires_grad_(True),))
    mix = torch.randn(2, 3, 5, generator=g, dtype=C128)
    refs = [torch.randn(2, 3, 5, generator=g, dtype=C128) for _ in range(2)]
    logits = torch.randn(2, 2, 3, 5, generator=g, dtype=F64).requires_grad_(True)
    for act in ("sigmoid", "tanh"):
        for mt in ("IRM", "PSM"):
            f = lambda z: E.permutation_loss(E.mask_label(mix, refs, mt), list(E.ACTS[act](z)), E.tf_mse_loss)[0]  # noqa: E731
            assert torch.autograd.gradcheck(f, (logits,))
        for crit in (E.tf_mse_loss, E.mag_mse_loss):
            f = lambda z: E.permutation_loss(refs, list(E.mask_apply(z, mix, act)[1]), crit)[0]  # noqa: E731
            assert torch.autograd.gradcheck(f, (logits,))
    # the closed form of the mask application's backward
    gm, gp = torch.randn(2, 2, 3, 5, generator=g, dtype=F64), torch.randn(2, 2, 3, 5, generator=g, dtype=C128)
    for act in ("sigmoid", "relu", "tanh", "none"):
        z = logits.detach().clone().requires_grad_(True)
        m, P = E.mask_apply(z, mix, act)
        ((m * gm).sum() + (P.real * gp.real + P.imag * gp.imag).sum()).backward()
        assert E.err_vs(E.mask_apply_bwd(z.detach(), mix, act, gm, gp), z.grad) < 1e-12


def test_magnitude_gradient_is_zero_where_the_estimate_is_zero():
    """the departure: |P| at P = 0 (every padded frame) takes gradient 0; the reference's formula gives NaN there"""
    ref = torch.randn(1, 2, 3, dtype=C128)
    inf = torch.zeros(1, 2, 3, 2, dtype=F64, requires_grad=True)
    E.mag_mse_loss(ref, torch.view_as_complex(inf)).sum().backward()
    assert float(inf.grad.abs().max()) == 0.0
    inf2 = torch.zeros(1, 2, 3, 2, dtype=F64, requires_grad=True)
    E.mag_mse_loss(ref, torch.view_as_complex(inf2), zero_grad_at_zero=False).sum().backward()
    assert torch.isnan(inf2.grad).all()


# ---- models --------------------------------------------------------------------------------------------------------------
def _sd(golden, prefix, dtype=F64):
    return {k[len(prefix) + 3:]: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in golden.items()
            if k.startswith(prefix + "sd/")}


def restated_tfm(golden, name, dtype=F64):
    c, p = K.TFM_CASES[name], "tfm/%s/" % name
    sd = _sd(golden, p, dtype)
    wav = torch.from_numpy(golden[p + "in/speech_mix"]).to(dtype)
    refs = [torch.from_numpy(golden[p + "in/speech_ref%d" % (s + 1)]).to(dtype) for s in range(c["conf"]["num_spk"])]
    conf = dict(c["conf"], loss_type=c.get("loss_type", c["conf"]["loss_type"]))
    out = E.tf_masking_model(sd, wav, list(c["lens"]), refs, conf, c["training"])
    if c["training"]:
        out["loss"].backward()
    return out, sd


@pytest.mark.parametrize("name", K.TFM_CASES)
def test_tf_masking_model_equals_the_reference(golden, name):
    """loss, permutation, the eval-mode SI-SNR statistic and every parameter gradient of
    ESPnetEnhancementModel(TFMaskingNet): 1e-10 of the largest gradient"""
    p = "tfm/%s/" % name
    assert {k: v.tolist() for k, v in K.as_np(K.tfm_batch(name)[0]).items()} == \
        {k[len(p) + 3:]: v.tolist() for k, v in golden.items() if k.startswith(p + "in/")}
    assert gap_of(golden[p + "pair"]) >= 1e-3
    out, sd = restated_tfm(golden, name)
    assert abs(num(out["loss"]) - num(golden[p + "loss"])) <= 1e-10 * abs(num(golden[p + "loss"]))
    assert out["perm"].tolist() == golden[p + "perm"].tolist()
    if p + "si_snr" in golden:
        assert abs(num(out["si_snr"]) - num(golden[p + "si_snr"])) <= 1e-10 * abs(num(golden[p + "si_snr"]))
    grads = {k[len(p) + 5:]: v for k, v in golden.items() if k.startswith(p + "grad/")}
    assert bool(grads) == K.TFM_CASES[name]["training"]
    if grads:
        gmax = max(float(np.abs(v).max()) for v in grads.values())
        for k, v in grads.items():
            assert float((sd[k].grad - torch.from_numpy(v)).abs().max()) <= 1e-10 * gmax, k


@pytest.mark.parametrize("name", K.BFN_CASES)
def test_beamformer_model_equals_the_reference(golden, name):
    """ESPnetEnhancementModel(BeamformerNet) in training with mask_mse: the speech-mask and the noise-mask term and the
    mask estimator's gradients (the beamformer itself does not run there, as in the reference)"""
    c, p = K.BFN_CASES[name], "bfn/%s/" % name
    sd = {k[len("beamformer."):]: v for k, v in _sd(golden, p).items()}
    b = {k: torch.from_numpy(golden[p + "in/" + k]).double() for k in ("speech_mix", "speech_ref1", "noise_ref1")}
    out = E.beamformer_model(sd, b["speech_mix"], list(c["lens"]), b["speech_ref1"], b["noise_ref1"], c["conf"])
    out["loss"].backward()
    assert abs(num(out["loss"]) - num(golden[p + "loss"])) <= 1e-10 * abs(num(golden[p + "loss"]))
    grads = {k[len(p) + 5 + len("beamformer."):]: v for k, v in golden.items() if k.startswith(p + "grad/")}
    assert grads and all(k.startswith("mask.") for k in grads)
    gmax = max(float(np.abs(v).max()) for v in grads.values())
    for k, v in grads.items():
        assert float((sd[k].grad - torch.from_numpy(v)).abs().max()) <= 1e-10 * gmax, k


# ---- what keeps the GPU bound meaningful -------------------------------------------------------------------------------
def test_float32_restatement_errors_on_the_gpu_test_inputs():
    """the float32 restatement against the float64 one on the inputs of tests/test_gpu_enh.py: below 1e-3 (and above 0), so
    that '4x the float32 restatement's error' is a real bound.  Observed: istft 3.4e-6 (waveform) and 5.5e-6
    (spectrum gradient), mask application <= 2.0e-7, pair matrices 1.1e-6 (mask), 2.7e-7 (magnitude), 1.5e-7 (spectrum),
    5.5e-7 (SI-SNR), estimate gradients <= 2.3e-6 and 1.0e-4 for SI-SNR at 60 dB, model losses <= 3.2e-7, model
    gradients <= 5.0e-6."""
    import test_gpu_enh as G
    worst = {}
    for key, run in G.restated_cases():
        r64, r32 = run(True), run(False)
        for k in r64:
            if r64[k].dtype == torch.int64:
                continue
            e = E.err_vs(r32[k].to(r64[k].dtype), r64[k])
            worst[key.split("/")[0] + ":" + k] = max(worst.get(key.split("/")[0] + ":" + k, 0.0), e)
            assert e < 1e-3, (key, k, e)
    print("[enh] float32 restatement error: " + ", ".join("%s %.1e" % kv for kv in sorted(worst.items())))
    assert min(worst.values()) > 0


# ---- the C ABI and the public surface ----------------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from espnet_amd import _lib
    L = _lib.lib()
    a = 0x10000                                                       # made-up addresses: no row may be a valid call
    assert L.eamd_istft_ola(None, a, a, 1, 4, 32, 8, 1, 40, None) == -1
    assert L.eamd_istft_ola(a, a, a, 1, 4, 64, 3, 1, 40, None) == -2        # more than 16 overlapping frames
    assert L.eamd_istft_ola(a, a, a, 1, 4, 32, 0, 1, 40, None) == -1
    assert L.eamd_istft_ola_bwd(a, a, None, 1, 4, 32, 8, 1, 40, 7, None) == -1
    assert L.eamd_istft_ola_bwd(a, a, a, 1, 4, 32, 8, 1, 40, 6, None) == -1  # rows that do not cover the frames
    assert L.eamd_istft_ola_bwd(a, a, a, 1, 4, 64, 3, 1, 40, 30, None) == -2
    assert L.eamd_enh_mask_apply(None, a, a, a, 2, 100, 0, None) == -1
    assert L.eamd_enh_mask_apply(a, None, a, a, 2, 100, 0, None) == -1       # a spectrum without the mixture
    assert L.eamd_enh_mask_apply(a, a, a, a, 2, 100, 4, None) == -1          # no such activation
    assert L.eamd_enh_mask_apply_bwd(a, a, None, None, a, 2, 100, 0, None) == -1
    assert L.eamd_enh_pair_tf(a, None, a, a, a, 2, 3, 100, 1, 0, 0, 0, None) == -1
    assert L.eamd_enh_pair_tf(a, a, None, a, a, 2, 3, 100, 1, 0, 0, 0, None) == -1   # MASK mode needs the mixture
    assert L.eamd_enh_pair_tf(a, a, a, a, a, 4, 3, 100, 1, 0, 0, 0, None) == -2      # S = 4
    assert L.eamd_enh_pair_tf(a, a, a, a, a, 2, 3, 5000, 1, 0, 0, 0, None) == -1     # nchunk != ceil(n / 4096)
    assert L.eamd_enh_pair_tf(a, a, a, a, a, 2, 3, 100, 1, 0, 6, 0, None) == -1      # no such label
    assert L.eamd_enh_pair_tf_bwd(a, a, a, None, a, a, 2, 3, 100, 0, 0, 0, None) == -1
    assert L.eamd_enh_pair_sisnr(a, a, a, None, a, 2, 3, 100, 1, 0, None) == -1
    assert L.eamd_enh_pair_sisnr(a, a, a, a, a, 0, 3, 100, 1, 0, None) == -2
    assert L.eamd_enh_pair_sisnr(a, a, a, a, a, 2, 3, 100, 1, 2, None) == -1         # no such criterion
    assert L.eamd_enh_pair_sisnr_bwd(a, a, None, a, a, a, 2, 3, 100, 0, None) == -1
    assert L.eamd_enh_pit_pick(None, None, a, a, 3, 2, None) == -1
    assert L.eamd_enh_pit_pick(a, None, a, a, 3, 4, None) == -2
    assert L.eamd_enh_pit_pick(a, None, a, a, 3, 0, None) == -2


def test_public_surface():
    from espnet_amd.espnet2.enh import BeamformerNet, ESPnetEnhancementModel, TFMaskingNet
    small = dict(n_fft=32, hop_length=8)
    m = TFMaskingNet(layer=1, unit=8, **small)
    assert (m.num_spk, m.num_bin, m.mask_type, m.loss_type) == (2, 17, "IRM", "mask_mse")
    assert {"rnn.nbrnn.weight_ih_l0", "rnn.l_last.weight", "linear.0.weight", "linear.1.bias"} <= set(m.state_dict())
    with pytest.raises(ValueError, match="si_snr"):
        TFMaskingNet(loss_type="si_snr", layer=1, unit=8, **small)
    with pytest.raises(ValueError, match="crelu"):
        TFMaskingNet(nonlinear="crelu", layer=1, unit=8, **small)
    e = ESPnetEnhancementModel(m)
    assert (e.num_spk, e.mask_type, e.loss_type, e.ref_channel) == (2, "IRM", "mask_mse", -1)
    bf = dict(blayers=1, bunits=8, bprojs=8, badim=8, **small)
    with pytest.raises(ValueError, match=r"IPM\^2"):                   # BeamformerNet's own default; the reference trips at the first batch
        ESPnetEnhancementModel(BeamformerNet(**bf))
    b = BeamformerNet(mask_type="PSM^2", beamformer_type="wpd", taps=2, delay=2, **bf)
    assert (b.beamformer.beamformer_type, b.beamformer.btaps, b.beamformer.bdelay) == ("wpd", 2, 2)
    assert ESPnetEnhancementModel(b).num_noise_type == 1
    assert {"beamformer.mask.linears.1.weight", "beamformer.ref.gvec.bias"} <= set(b.state_dict())
    for kw, what in ((dict(use_wpe=True), "DNN_WPE"), (dict(num_spk=2), "bnmask"), (dict(use_noise_mask=False), "bnmask"),
                     (dict(bnonlinear="relu"), "sigmoid"), (dict(normalize_input=True), "normalize_input")):
        with pytest.raises(NotImplementedError, match=what):
            BeamformerNet(mask_type="PSM^2", **dict(bf, **kw))
    with pytest.raises(ValueError, match="Unsupported loss type"):
        BeamformerNet(loss_type="magnitude", **bf)
    with pytest.raises(NotImplementedError, match="dereverb_ref"):
        e(torch.zeros(1, 100), None, speech_ref1=torch.zeros(1, 100), speech_ref2=torch.zeros(1, 100), dereverb_ref=torch.zeros(1, 100))
    feats = e.collect_feats(torch.zeros(2, 100), torch.tensor([80, 60]))
    assert feats["feats"].shape == (2, 80) and feats["feats_lengths"].tolist() == [80, 60]


def test_product_path_has_no_cpu_fallback_for_enhancement():
    from espnet_amd import _lib
    from espnet_amd.espnet2.enh import ESPnetEnhancementModel
    with pytest.raises(_lib.EamdError):
        ESPnetEnhancementModel.si_snr_loss(torch.randn(2, 50), torch.randn(2, 50))
