"""Jointly trained speech-enhancement front-end of the RNN E2E, without a GPU: the float64 restatement of the espnet1
feature transform (tests/feature_transform_restatement.py) against the reference's float64 run recorded in
tests/golden/frontend_e2e.npz, the construction, input forms, draw order and refusals of E2E(use_frontend=True), and the
host-side argument checks of the new entry points."""
import argparse
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import feature_transform_restatement as R
from conftest import ROOT, load_golden

FT_TAGS = ["s%d_m%dv%d_d%d" % (s, m, v, d) for s in (0, 1) for m in (0, 1) for v in (0, 1) for d in (3, 4)]
E2E_CASES = ("blstmp_bf", "blstmp_pass", "vggblstmp_bf")


@pytest.fixture(scope="module")
def golden():
    return load_golden("frontend_e2e.npz")


def e2e_args(g, **kw):
    return argparse.Namespace(**dict(json.loads(str(g["e2e/args_json"])), **kw))


def ft_inputs(g, tag, dtype=torch.float64):
    """-> (complex input, melmat, ilens, bias, scale, norm_means, norm_vars) of one ft/* case"""
    s, m, v, d = (int(c) for c in re.match(r"s(\d)_m(\d)v(\d)_d(\d)", tag).groups())
    x = R.cx(g["ft/x%d" % d]).to(torch.complex128 if dtype == torch.float64 else torch.complex64)
    bias, scale = R.stats_bias_scale(g["ft/stats"], dtype) if s else (None, None)
    return x, torch.from_numpy(g["ft/melmat"]).to(dtype), g["ft/ilens"].tolist(), bias, scale, bool(m), bool(v)


def ft_restated(g, tag, dtype=torch.float64):
    x, melmat, ilens, bias, scale, nm, nv = ft_inputs(g, tag, dtype)
    x.requires_grad_(not nv)
    h = R.feature_transform(x, melmat, ilens, bias, scale, True, nm, nv)
    gx = None
    if not nv:
        (h * torch.from_numpy(g["ft/w"]).to(dtype)).sum().backward()
        gx = R.ri(x.grad)
    return h.detach(), gx


@pytest.mark.parametrize("tag", FT_TAGS)
def test_restatement_reproduces_the_reference_in_float64(golden, tag):
    """outputs on ALL frames, the padded ones included, and the gradient with respect to the complex input: 1e-9"""
    h, gx = ft_restated(golden, tag)
    want = torch.from_numpy(golden["ft/%s/out" % tag])
    assert h.shape == want.shape and R.err_vs(h, want) < 1e-9, R.err_vs(h, want)
    if gx is not None:
        wg = torch.from_numpy(golden["ft/%s/gx" % tag])
        assert gx.shape == wg.shape and R.err_vs(gx, wg) < 1e-9, R.err_vs(gx, wg)
    else:
        assert "ft/%s/gx" % tag not in golden


def test_padded_frames_are_part_of_the_recorded_output(golden):
    """the quirk is pinned: the padded frames enter the utterance mean and leave the layer non-zero, so zeroing them - in
    the output, or in front of the utterance MVN - does not give what the reference computed"""
    for tag in ("s0_m1v0_d3", "s1_m1v0_d3", "s1_m0v1_d4"):
        x, melmat, ilens, bias, scale, nm, nv = ft_inputs(golden, tag)
        want = torch.from_numpy(golden["ft/%s/out" % tag])
        short = int(np.argmin(ilens))
        assert float(want[short, ilens[short]:].abs().min()) > 1e-3                                   # not zero padded
        h = R.logmel(x if x.dim() == 3 else x[:, :, 0], melmat, ilens)
        if bias is not None:
            h = R.global_mvn(h, bias, scale).masked_fill(R.pad_mask(ilens, h.shape[1])[:, :, None], 0.0)   # what an in-place fill would do
            got = R.utterance_mvn(h, ilens, nm, nv)
            assert R.err_vs(got[short, :ilens[short]], want[short, :ilens[short]]) > 1e-2, tag
        z = want.clone()
        z[short, ilens[short]:] = 0
        assert R.err_vs(z, want) > 1e-2


def test_fixture_bars_and_mel_matrix(golden):
    """every recorded quantity comes with the reference's own float32 error, inside the generator's bars; the product's
    mel matrix is the recorded one"""
    from espnet_amd.espnet2.frontend import mel_filterbank
    for tag in FT_TAGS:
        assert 0.0 <= float(golden["ft/%s/err32/out" % tag]) < 1e-5
    for case in E2E_CASES:
        p = "e2e/%s/" % case
        zero = set(golden[p + "zero_grads"].tolist())
        assert zero <= {"att.0.gvec.bias", "frontend.beamformer.ref.gvec.bias"}
        for k in ("loss", "loss_ctc", "loss_att"):
            assert float(golden[p + "err32/" + k]) <= 2.5e-6
        errs = {k: float(v) for k, v in golden.items() if k.startswith(p + "err32/grad/")}
        assert errs and max(errs.values()) <= 1.25e-4
        assert all(int(n) >= 4 * golden["e2e/xs"].shape[2] for n in golden["e2e/ilens"])
    assert int(golden["e2e/blstmp_bf/draws"][0]) == 1 and int(golden["e2e/blstmp_pass/draws"][0]) == 0
    mel = mel_filterbank(16000, 32, 8, 0.0, None, False).T
    assert np.abs(mel - golden["ft/melmat"]).max() <= 1e-6 * np.abs(golden["ft/melmat"]).max()


@pytest.mark.parametrize("case", E2E_CASES)
def test_e2e_with_frontend_constructs_without_a_gpu(golden, case):
    """parameter and buffer names and their order equal the reference's; the encoder is built on n_mels features"""
    from espnet_amd.nets.e2e_asr import E2E
    etype = "vggblstmp" if case.startswith("vgg") else "blstmp"
    m = E2E(17, int(golden["e2e/odim"]), e2e_args(golden, etype=etype))
    assert list(m.state_dict().keys()) == golden["e2e/%s/state_dict_keys" % case].tolist()
    assert m.frontend.beamformer.mask.linears[0].weight.shape == (17, 8)
    assert m.feature_transform.logmel.melmat.shape == (17, 8)
    seeded = set(golden["e2e/%s/seeded_keys" % case].tolist())
    for k, v in m.state_dict().items():
        if k not in seeded:
            assert tuple(golden["e2e/%s/sd/%s" % (case, k)].shape) == tuple(v.shape), k
    plain = E2E(17, 7, e2e_args(golden, use_frontend=False))
    assert plain.frontend is None and not hasattr(plain, "feature_transform")
    assert list(plain.state_dict().keys()) == [k for k in E2E(17, 7, e2e_args(golden)).state_dict() if not k.startswith(("frontend.", "feature_transform."))]


def test_input_forms():
    """complex64 tensor, float tensor with a trailing (re, im) axis, complex numpy array, dict with real and imag"""
    from espnet_amd.nets.e2e_asr import to_spectrum
    g = torch.Generator().manual_seed(0)
    c = torch.complex(torch.randn(2, 5, 3, 4, generator=g), torch.randn(2, 5, 3, 4, generator=g))
    want = torch.view_as_real(c)
    for form in (c, want.clone(), c.numpy(), dict(real=c.real.numpy(), imag=c.imag.numpy()), dict(real=c.real, imag=c.imag),
                 c.to(torch.complex128)):
        got = to_spectrum(form)
        assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, want)
    with pytest.raises(ValueError):
        to_spectrum(torch.zeros(2, 5, 3, 4))
    with pytest.raises(ValueError):
        to_spectrum(dict(real=c.real))


def test_training_mode_draws_as_the_reference_does(golden):
    """frontend.py:101-109 then feature_transform.py:54-62: one numpy.random.randint(2) per call chooses between
    pass-through and beamforming, and on pass-through one randint(C) chooses the channel; eval: beamformer, no draw"""
    from espnet_amd.nets.e2e_asr import E2E
    m = E2E(17, 7, e2e_args(golden, apply_uttmvn=False)).train()
    C = 3
    calls, seen = [], []
    m.frontend.beamformer.forward = lambda h, ilens: (calls.append(1), (h[:, :, 0] + 100.0, ilens, None))[1]
    m.feature_transform.logmel.from_spectrum = lambda spec, lens: (seen.append(float(spec[0, 0, 0, 0])), spec[..., 0])[1]
    x = torch.zeros(2, 6, C, 17, 2)
    for c in range(C):
        x[:, :, c] = float(c)
    np.random.seed(3)
    want = []
    for _ in range(10):
        d = int(np.random.randint(2))
        want.append((d, None if d else int(np.random.randint(C))))
    assert {d for d, _ in want} == {0, 1}
    np.random.seed(3)
    for d, ch in want:
        before = len(calls)
        h, hlens = m._features(x, [6, 6])
        assert (len(calls) - before == 1) == bool(d)
        assert seen[-1] == (100.0 if d else float(ch))
        assert h.shape == (2, 6, 17) and [int(v) for v in hlens] == [6, 6]
    m.eval()
    state = np.random.get_state()[1].copy()
    m._features(x, [6, 6])
    assert seen[-1] == 100.0 and np.array_equal(np.random.get_state()[1], state)      # eval: beamformer, nothing drawn
    m.frontend.use_beamformer = False                                                 # eval pass-through: channel 0
    m._features(x, [6, 6])
    assert seen[-1] == 0.0


def test_refusals(golden, tmp_path):
    from espnet_amd.nets.e2e_asr import E2E
    from espnet_amd.nets.frontends.feature_transform import FeatureTransform, LogMel, utterance_mvn
    with pytest.raises(NotImplementedError, match="WPE"):
        E2E(17, 7, e2e_args(golden, use_wpe=True))
    with pytest.raises(NotImplementedError, match="bnmask"):
        E2E(17, 7, e2e_args(golden, bnmask=3))
    with pytest.raises(NotImplementedError):
        LogMel(n_fft=32, n_mels=8, norm=None)
    x = torch.zeros(2, 6, 17, 2, requires_grad=True)
    ft = FeatureTransform(n_fft=32, n_mels=8, uttmvn_norm_vars=True)
    with pytest.raises(RuntimeError, match="reference's own backward"):               # before any kernel: no GPU needed
        ft(x, [6, 4])
    with pytest.raises(RuntimeError, match="reference's own backward"):
        utterance_mvn(torch.zeros(2, 6, 8, requires_grad=True), [6, 4], norm_vars=True)
    for args in ((x.detach(), [6, 4]), (torch.zeros(2, 6, 3, 17, 2), [6, 4])):        # no gradient asked: accepted, then needs the GPU
        with pytest.raises(Exception) as ei:
            ft(*args)
        assert not isinstance(ei.value, (RuntimeError, NotImplementedError)) or "reference's own backward" not in str(ei.value)
    with torch.no_grad(), pytest.raises(Exception) as ei:
        ft(x, [6, 4])
    assert "reference's own backward" not in str(ei.value)
    with pytest.raises(RuntimeError, match="Frontend"):
        E2E(17, 7, e2e_args(golden, use_frontend=False)).enhance([np.zeros((5, 3, 17), np.complex64)])
    np.save(tmp_path / "stats.npy", golden["ft/stats"])
    gm = FeatureTransform(n_fft=32, n_mels=8, stats_file=str(tmp_path / "stats.npy"))
    assert list(gm.state_dict().keys()) == ["logmel.melmat", "global_mvn.bias", "global_mvn.scale"]
    bias, scale = R.stats_bias_scale(golden["ft/stats"], torch.float32)
    assert torch.equal(gm.global_mvn.bias, bias) and torch.equal(gm.global_mvn.scale, scale)


def test_entry_points_reject_bad_arguments_without_a_device():
    from espnet_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = ctypes.c_float
    assert lib.eamd_ft_logmel_fwd(None, None, None, None, None, None, 2, 5, 17, 8, None) < 0
    assert lib.eamd_ft_logmel_bwd(None, None, None, None, None, None, None, None, None, 2, 5, 17, 8, None) < 0
    assert lib.eamd_ft_mvn_fwd(None, None, None, None, None, None, 1, 1, 0, f(1e-20), 2, 5, 8, None) < 0
    assert lib.eamd_ft_mvn_bwd(None, None, None, None, None, 1, 2, 5, 8, None) < 0
    assert lib.eamd_conv3x3_c1_bwd_x(None, None, None, 2, 5, 8, 64, 0, None) < 0
    for B, T, F, M in ((0, 5, 17, 8), (2, 0, 17, 8), (2, 5, 0, 8), (2, 5, 17, 0), (-1, 5, 17, 8)):
        assert lib.eamd_ft_logmel_fwd(p, p, p, p, p, p, B, T, F, M, None) == -1
        assert lib.eamd_ft_logmel_bwd(p, p, p, p, p, p, p, p, p, B, T, F, M, None) == -1
        assert lib.eamd_ft_mvn_fwd(p, p, p, p, p, p, 1, 1, 0, f(1e-20), B, T, M, None) == -1 or F == 0
        assert lib.eamd_ft_mvn_bwd(p, p, p, p, p, 1, B, T, M, None) == -1 or F == 0
        assert lib.eamd_conv3x3_c1_bwd_x(p, p, p, B, T, F, 64, 0, None) == -1 or M == 0
    assert lib.eamd_conv3x3_c1_bwd_x(p, p, p, 2, 5, 8, 0, 0, None) == -1
    # one of bias / scale alone, and utterance statistics without lengths or workspace
    assert lib.eamd_ft_mvn_fwd(p, p, p, p, None, p, 1, 1, 0, f(1e-20), 2, 5, 8, None) == -1
    assert lib.eamd_ft_mvn_fwd(p, p, None, None, None, p, 1, 1, 0, f(1e-20), 2, 5, 8, None) == -1
    assert lib.eamd_ft_mvn_fwd(p, p, p, None, None, None, 1, 1, 0, f(1e-20), 2, 5, 8, None) == -1
    assert lib.eamd_ft_mvn_bwd(p, p, None, None, p, 1, 2, 5, 8, None) == -1
    # LDS requests that depend on F, M, C: refused as unsupported before any launch
    assert lib.eamd_ft_logmel_fwd(p, p, p, p, p, p, 2, 5, 4097, 8, None) == _lib.EAMD_EUNSUPPORTED
    assert lib.eamd_ft_logmel_bwd(p, p, p, p, p, p, p, p, p, 2, 5, 4000, 97, None) == _lib.EAMD_EUNSUPPORTED
    assert lib.eamd_conv3x3_c1_bwd_x(p, p, p, 2, 5, 400, 64, 0, None) == _lib.EAMD_EUNSUPPORTED
    assert lib.eamd_conv3x3_c1_bwd_x(p, p, p, 2, 5, 8, 6, 0, None) == _lib.EAMD_EUNSUPPORTED


def test_header_library_and_binding_agree():
    from espnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "espnet_amd.h")).read()
    declared = sorted(set(re.findall(r"\b(eamd_[a-z0-9_]+)\s*\(", header)))
    lib = _lib.lib()
    for s in ("eamd_ft_logmel_fwd", "eamd_ft_logmel_bwd", "eamd_ft_mvn_fwd", "eamd_ft_mvn_bwd", "eamd_conv3x3_c1_bwd_x"):
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
    assert sorted(_lib.SYMBOLS) == declared
    assert lib.eamd_abi_version() == 1
