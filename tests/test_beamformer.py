"""MVDR beamforming front-end without a GPU: the float64 restatement (tests/beamformer_restatement.py) against the
reference's float64 run recorded in tests/golden/beamformer.npz, the construction and refusals of the public surface,
and the host-side argument checks of the new entry points."""
import ctypes

import numpy as np
import pytest
import torch

import beamformer_restatement as R
from conftest import load_golden

CASES = ("c3", "c2ref0", "c8")
CONF = dict(use_beamformer=True, blayers=1, bunits=8, bprojs=8, badim=8)


@pytest.fixture(scope="module")
def golden():
    return load_golden("beamformer.npz")


def case_of(g, name, dtype=torch.float64):
    """-> (x complex [B,T,C,F], ilens, ref_channel, state_dict as leaves that require grad)"""
    p = name + "/"
    x = R.cx(g[p + "x"]).to(torch.complex128 if dtype == torch.float64 else torch.complex64)
    sd = {k[len(p) + 3:]: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in g.items() if k.startswith(p + "sd/")}
    return x, [int(v) for v in g[p + "ilens"]], int(g[p + "ref_channel"]), sd


def recorded(g, name):
    """the reference's float64 results in the restatement's layouts"""
    p = name + "/"
    out = {k: R.cx(g[p + k]) for k in ("psd_speech", "psd_noise", "ws", "enhanced")}
    out["u"] = torch.from_numpy(g[p + "u"])
    out["mask_speech"] = torch.from_numpy(g[p + "mask_speech"])
    grads = {k[len(p) + 5:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(p + "grad/")}
    return out, grads


def restated(g, name, dtype=torch.float64):
    x, ilens, ref_channel, sd = case_of(g, name, dtype)
    out = R.dnn_beamformer(sd, x, ilens, ref_channel)
    (out["enhanced"].real ** 2 + out["enhanced"].imag ** 2).sum().backward()
    return out, {k: v.grad for k, v in sd.items() if v.grad is not None}


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_in_float64(golden, name):
    """1e-9 relative: both sides are float64, the noise PSDs' condition numbers reach about 240"""
    want, want_g = recorded(golden, name)
    got, got_g = restated(golden, name)
    for k, v in want.items():
        assert got[k].shape == v.shape, k
        assert R.err_vs(got[k].detach(), v) < 1e-9, (k, R.err_vs(got[k].detach(), v))
    zero = set(golden[name + "/zero_grads"].tolist())
    assert set(want_g) | zero == set(got_g) and want_g
    gmax = max(float(v.abs().max()) for v in want_g.values())
    for k, v in want_g.items():
        assert R.err_vs(got_g[k], v) < 1e-9, (k, R.err_vs(got_g[k], v))
    for k in zero:                                          # identically zero: rounding noise on both sides
        assert float(got_g[k].abs().max()) <= 1e-12 * gmax, k


def test_fixture_records_the_reference_s_own_float32_error(golden):
    """every recorded quantity comes with err32, and the restatement run in float32 errs at the same order"""
    for name in CASES:
        want, want_g = recorded(golden, name)
        for k in list(want) + ["grad/" + k for k in want_g]:
            e = float(golden[name + "/err32/" + k])
            assert 0.0 <= e < 1e-3, (name, k, e)
        got32, _ = restated(golden, name, torch.float32)
        for k in ("ws", "enhanced"):
            e = R.err_vs(got32[k].detach().to(torch.complex128), want[k])
            assert e < 16 * float(golden[name + "/err32/" + k]), (name, k, e)


def test_padded_frames_enter_the_normaliser(golden):
    """frames between an utterance's length and Tm carry sigmoid(bias) masks (the reference's masked_fill without the
    underscore) and count in n; zeroing them changes the recorded PSD"""
    x, ilens, _, sd = case_of(golden, "c3")
    want, _ = recorded(golden, "c3")
    with torch.no_grad():
        z = R.mask_logits(sd, x, ilens)
        short = int(np.argmin(ilens))
        pad = torch.sigmoid(z[0, short, :, ilens[short]:])
        assert pad.shape[1] > 0 and float((pad - pad[:, :1]).abs().max()) < 1e-12      # one constant row per channel
        assert R.err_vs(R.psd_matrices(x, z)[0], want["psd_speech"]) < 1e-9
        z2 = z.clone()
        z2[:, short, :, ilens[short]:] = -1e9                                           # masks of the padding -> 0
        assert R.err_vs(R.psd_matrices(x, z2)[0][short], want["psd_speech"][short]) > 1e-2


def test_default_frontend_builds_the_beamformer_without_a_gpu(golden):
    from espnet_amd.espnet2.frontend import DefaultFrontend
    fe = DefaultFrontend(frontend_conf=dict(CONF))
    assert list(fe.frontend.state_dict().keys()) == golden["state_dict_keys"].tolist()
    assert fe.frontend.beamformer.mask.linears[0].weight.shape == (257, 8)
    for conf in (None, dict(use_beamformer=False, use_wpe=False), {}):
        assert DefaultFrontend(frontend_conf=conf).frontend is None


def test_module_state_dict_matches_the_fixture_weights(golden):
    """the 2-layer fixture weights load key for key and shape for shape"""
    from espnet_amd.nets.frontends.dnn_beamformer import DNN_Beamformer
    _, _, _, sd = case_of(golden, "c8", torch.float32)
    m = DNN_Beamformer(17, "blstmp", 2, 8, 8, 2, 0.0, 8)
    m.load_state_dict({k: v.detach() for k, v in sd.items()}, strict=True)


def test_refusals():
    from espnet_amd.espnet2.frontend import DefaultFrontend
    from espnet_amd.nets.frontends.dnn_beamformer import DNN_Beamformer
    from espnet_amd.nets.frontends.frontend import Frontend
    with pytest.raises(NotImplementedError, match="WPE") as ei:
        DefaultFrontend(frontend_conf=dict(use_wpe=True))
    assert "beamformer" not in str(ei.value).lower()
    with pytest.raises(NotImplementedError, match="WPE"):
        Frontend(idim=17, use_wpe=True, use_beamformer=True)
    with pytest.raises(NotImplementedError, match="bnmask"):
        DefaultFrontend(frontend_conf=dict(CONF, bnmask=3))
    with pytest.raises(ValueError, match="beamformer_type"):
        DNN_Beamformer(17, blayers=1, bunits=4, bprojs=4, badim=4, beamformer_type="gev")
    fe = DefaultFrontend(frontend_conf=dict(CONF)).train()
    wav = torch.zeros(1, 2000, 2)
    with pytest.raises(NotImplementedError, match="jointly"):           # before any kernel: no GPU needed
        fe(wav, [2000])
    fe.frontend.requires_grad_(False)
    with pytest.raises(Exception) as ei:                                # frozen: accepted, and then needs the GPU
        fe(wav, [2000])
    assert not isinstance(ei.value, NotImplementedError)


def test_training_mode_draws_as_the_reference_does():
    """frontend.py:101-109: one numpy.random.randint(2) per call chooses between pass-through and beamforming"""
    from espnet_amd.nets.frontends.frontend import Frontend
    fe = Frontend(idim=5, use_beamformer=True, blayers=1, bunits=4, bprojs=4, badim=4).train()
    calls = []
    fe.beamformer.forward = lambda h, ilens: (calls.append(1), (h[:, :, 0], ilens, None))[1]
    x = torch.zeros(2, 6, 3, 5, 2)
    np.random.seed(3)
    draws = [int(np.random.randint(2)) for _ in range(8)]
    np.random.seed(3)
    for d in draws:
        before = len(calls)
        h, _, _ = fe(x, [6, 6])
        assert (len(calls) - before == 1) == bool(d) and h.dim() == (4 if d else 5)
    fe.eval()
    assert fe(x, [6, 6])[0].dim() == 4


def test_entry_points_reject_bad_arguments_without_a_device():
    from espnet_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.eamd_bf_psd(None, None, None, None, None, None, 2, 1, 4, 4, 2, 3, None) < 0
    assert lib.eamd_bf_psd_bwd(None, None, None, None, None, None, None, None, 2, 1, 4, 4, 2, 3, None) < 0
    assert lib.eamd_bf_mvdr(None, None, None, None, 1, 3, 2, None) < 0
    assert lib.eamd_bf_mvdr_bwd(None, None, None, None, None, None, None, None, 1, 3, 2, None) < 0
    assert lib.eamd_bf_apply(None, None, None, 1, 4, 2, 3, None) < 0
    assert lib.eamd_bf_apply_bwd(None, None, None, None, 1, 4, 2, 3, None) < 0
    for C in (1, 9):
        assert lib.eamd_bf_psd(p, p, p, p, p, p, 2, 1, 4, 4, C, 3, None) < 0
        assert lib.eamd_bf_psd_bwd(p, p, p, p, p, p, p, p, 2, 1, 4, 4, C, 3, None) < 0
        assert lib.eamd_bf_mvdr(p, p, p, p, 1, 3, C, None) < 0
        assert lib.eamd_bf_mvdr_bwd(p, p, p, p, p, p, p, p, 1, 3, C, None) < 0
        assert lib.eamd_bf_apply(p, p, p, 1, 4, C, 3, None) < 0
        assert lib.eamd_bf_apply_bwd(p, p, p, p, 1, 4, C, 3, None) < 0
        assert lib.eamd_bf_workspace_bytes(0, 2, 1, 4, C, 3) < 0
    # non-positive sizes, and a mask longer than the spectrum
    assert lib.eamd_bf_psd(p, p, p, p, p, p, 2, 0, 4, 4, 2, 3, None) < 0
    assert lib.eamd_bf_psd(p, p, p, p, p, p, 2, 1, 4, 5, 2, 3, None) < 0
    assert lib.eamd_bf_apply(p, p, p, 1, 0, 2, 3, None) < 0
    # workspace sizes: chunk partials of C*C + 1 planes (PSD) and 2 C planes (filter gradient)
    from espnet_amd import ops
    assert lib.eamd_bf_workspace_bytes(ops.BF_PSD, 2, 3, ops.BF_TCHUNK + 1, 4, 5) == 4 * 2 * 2 * 3 * 17 * 5
    assert lib.eamd_bf_workspace_bytes(ops.BF_APPLY_BWD, 1, 3, ops.BF_TCHUNK, 4, 5) == 4 * 1 * 3 * 8 * 5
