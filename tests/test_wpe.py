"""WPE dereverberation without a GPU.  The reference delegates the algorithm to a package that is not available, so the
float64 restatement (tests/wpe_restatement.py) is pinned here by the properties that define WPE - a second restatement in
plain loops, the normal equations, optimality of the weighted prediction error, batch independence, its closed-form
backward against autograd - and then the construction, refusals and draw order of the public surface."""
import ctypes

import numpy as np
import pytest
import torch

import wpe_restatement as W
from conftest import load_golden, seeded_weights

F = 5
IDS = ["C%dK%dD%d" % c[:3] for c in W.CASES]


def inputs(case, F=F, dtype=torch.complex128, seed=0):
    C, K, D, T, ilens = case
    y, z = W.synth(C, T, ilens, F, seed)
    rdt = torch.float64 if dtype == torch.complex128 else torch.float32
    return y.to(dtype), z.to(rdt)


def run(case, dtype, inverse_power=True, F=F):
    """restatement in `dtype` -> x, G, gpower and the logit gradient of L = Re <gx, x> for a seeded gx"""
    C, K, D, T, ilens = case
    y, z = inputs(case, F, dtype)
    z.requires_grad_(True)
    power = W.masked_power(y, z)
    power.retain_grad()
    x, G = W.one_iteration(y, power, ilens, K, D, inverse_power=inverse_power, return_filter=True)
    g = torch.Generator().manual_seed(5)
    gx = torch.complex(torch.randn(x.shape, generator=g), torch.randn(x.shape, generator=g)).to(dtype)
    (gx.conj() * x).real.sum().backward()
    return dict(x=x.detach(), G=G.detach(), gpower=power.grad, dz=z.grad, power=power.detach(), gx=gx, y=y)


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_vectorised_restatement_equals_the_loops(case):
    C, K, D, T, ilens = case
    y, z = inputs(case, F=2)
    power = W.masked_power(y, z)
    x, G = W.one_iteration(y, power, ilens, K, D, return_filter=True)
    xl, Gl = W.one_iteration_loops(y, power, ilens, K, D)
    assert W.err_vs(x, xl) < 1e-10 and W.err_vs(G, Gl) < 1e-10
    for b, n in enumerate(ilens):
        if n < T:
            assert float(x[b, n:].abs().max()) == 0.0


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_normal_equations_and_optimality(case):
    """R G = P at float64 rounding (cond(R) <= about 1.5e4); the weighted prediction error has zero gradient at G and is
    not lower at G + delta"""
    C, K, D, T, ilens = case
    y, z = inputs(case)
    power = W.masked_power(y, z)
    _, G = W.one_iteration(y, power, ilens, K, D, return_filter=True)
    g = torch.Generator().manual_seed(1)
    for b, n in enumerate(ilens):
        h, R, P = W.correlations(y[b, :n], power[b, :n], K, D)
        Gb = G[b].reshape(F, C * K, C)
        assert float(torch.linalg.cond(R).max()) < 1e5
        assert float(torch.linalg.norm(R @ Gb - P) / torch.linalg.norm(P)) < 1e-11
        Gv = Gb.clone().requires_grad_(True)
        cost = W.weighted_cost(y[b, :n], power[b, :n], Gv, K, D)
        (grad,) = torch.autograd.grad(cost, Gv)
        scale = float(torch.linalg.norm(P))
        assert float(torch.linalg.norm(grad)) < 1e-9 * scale
        for _ in range(3):
            delta = 1e-3 * torch.complex(torch.randn(Gb.shape, generator=g, dtype=torch.float64),
                                         torch.randn(Gb.shape, generator=g, dtype=torch.float64))
            assert float(W.weighted_cost(y[b, :n], power[b, :n], Gb + delta, K, D)) > float(cost)


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_an_utterance_in_a_batch_equals_the_utterance_alone(case):
    C, K, D, T, ilens = case
    y, z = inputs(case)
    power = W.masked_power(y, z)
    x = W.one_iteration(y, power, ilens, K, D)
    for b, n in enumerate(ilens):
        alone = W.one_iteration(y[b:b + 1, :n], power[b:b + 1, :n], [n], K, D)
        assert W.err_vs(x[b:b + 1, :n], alone) < 1e-12 and float(x[b, n:].abs().max() if n < T else 0.0) == 0.0


@pytest.mark.parametrize("inverse_power", (True, False))
@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_closed_form_backward_equals_autograd(case, inverse_power):
    C, K, D, T, ilens = case
    r = run(case, torch.complex128, inverse_power)
    got = W.one_iteration_backward(r["y"], r["power"], ilens, K, D, r["gx"], inverse_power=inverse_power)
    assert W.err_vs(got, r["gpower"]) < 1e-11
    # the logit gradient of the power step: gpower |y_c|^2 / C sigmoid'(z)
    y, z = inputs(case)
    s = torch.sigmoid(z[0])
    dz = (got[:, :, None, :] * (y.real ** 2 + y.imag ** 2) / C).permute(0, 2, 1, 3) * s * (1 - s)
    assert W.err_vs(dz[None], r["dz"]) < 1e-11


def test_two_iterations_without_a_mask():
    C, K, D, T, ilens = W.CASES[1]
    y, _ = inputs(W.CASES[1])
    out = W.dnn_wpe({}, y, ilens, K, D, iterations=2, use_dnn_mask=False)
    p0 = (y.real ** 2 + y.imag ** 2).mean(2)
    x1 = W.one_iteration(y, p0, ilens, K, D)
    x2 = W.one_iteration(y, (x1.real ** 2 + x1.imag ** 2).mean(2), ilens, K, D)
    assert out["mask"] is None and torch.equal(out["enhanced"], x2) and W.err_vs(x1, x2) > 1e-3
    # dereverberation: the late reverberation's share of the energy drops
    assert float(x2.abs().pow(2).sum()) < float(y.abs().pow(2).sum())


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_float32_restatement_errs_below_1e_3(case):
    """the condition that keeps the GPU tests' bound (4x this error) from being vacuous: x, G and the logit gradient of the
    restatement in float32 are within 1e-3 of float64 in max |a - ref| / max |ref|"""
    r64, r32 = run(case, torch.complex128), run(case, torch.complex64)
    for k in ("x", "G", "dz", "gpower"):
        e = W.err_vs(r32[k].to(r64[k].dtype), r64[k])
        print("[wpe] %s float32 restatement error %s %.2e" % (IDS[W.CASES.index(case)], k, e))
        assert 0 < e and (e <= 1e-3 or k == "gpower"), (k, e)


# ---- the public surface ------------------------------------------------------------------------------------------------
def test_dnn_wpe_state_dict_and_seeded_weights():
    """mask_est.* = the beamformer's mask.* keys without its second Linear, re-prefixed"""
    from espnet_amd.nets.frontends.dnn_wpe import DNN_WPE
    keys = load_golden("beamformer.npz")["state_dict_keys"].tolist()
    want = ["mask_est." + k[len("beamformer.mask."):] for k in keys
            if k.startswith("beamformer.mask.") and not k.startswith("beamformer.mask.linears.1.")]
    m = DNN_WPE(widim=257, wlayers=1, wunits=8, wprojs=8)
    assert want and list(m.state_dict().keys()) == want
    assert (m.taps, m.delay, m.iterations, m.use_dnn_mask, m.inverse_power, m.normalization) == (5, 3, 1, True, True, False)
    seeded_weights().fill_parameters(m, salt=41)
    assert all(torch.isfinite(p).all() and float(p.abs().max()) > 0 for p in m.parameters())
    plain = DNN_WPE(use_dnn_mask=False, iterations=2)
    assert not list(plain.state_dict().keys()) and plain.predict_mask(torch.zeros(1, 40, 2, 3, 2), [40]) == (None, [40])


def test_new_refusals():
    from espnet_amd.nets.frontends.dnn_wpe import DNN_WPE
    from espnet_amd.nets.frontends.wpe import wpe_one_iteration
    with pytest.raises(NotImplementedError, match="normalization"):
        DNN_WPE(widim=17, wlayers=1, wunits=4, wprojs=4, normalization=True)
    with pytest.raises(ValueError, match="delay"):
        DNN_WPE(widim=17, wlayers=1, wunits=4, wprojs=4, delay=-1)
    Y, p = torch.zeros(2, 120, 9, 3, 2), torch.ones(2, 120, 3)
    with pytest.raises(ValueError, match="64"):                       # before any launch: no GPU needed
        wpe_one_iteration(Y, p, [120, 120], taps=8)
    with pytest.raises(ValueError, match="delay"):
        wpe_one_iteration(Y[:, :, :2], p, [120, 120], taps=5, delay=-1)
    with pytest.raises(ValueError, match="too short"):                # 27 - 7 = 20 usable frames >= 10 unknowns, 16 - 7 = 9 not
        wpe_one_iteration(Y[:, :27, :2], p[:, :27], [27, 16], taps=5, delay=3)
    with pytest.raises(ValueError, match="too short"):
        DNN_WPE(use_dnn_mask=False)(Y[:, :16, :2], [16, 16])
    with pytest.raises(Exception) as ei:                              # long enough: accepted, and then needs the GPU
        wpe_one_iteration(Y[:, :27, :2], p[:, :27], [27, 17], taps=5, delay=3)
    assert not isinstance(ei.value, ValueError)


def test_constructor_switches_still_refuse_wpe():
    import argparse
    import json
    from espnet_amd.espnet2.frontend import DefaultFrontend
    from espnet_amd.nets.e2e_asr import E2E
    from espnet_amd.nets.frontends.frontend import Frontend
    with pytest.raises(NotImplementedError, match="WPE"):
        Frontend(idim=17, use_wpe=True)
    with pytest.raises(NotImplementedError, match="WPE"):
        DefaultFrontend(frontend_conf=dict(use_wpe=True))
    args = json.loads(str(load_golden("frontend_e2e.npz")["e2e/args_json"]))
    with pytest.raises(NotImplementedError, match="WPE"):
        E2E(17, 7, argparse.Namespace(**dict(args, use_wpe=True)))


def _frontend(use_beamformer=True):
    from espnet_amd.nets.frontends.dnn_wpe import DNN_WPE
    from espnet_amd.nets.frontends.frontend import Frontend
    fe = Frontend(idim=5, use_beamformer=use_beamformer, blayers=1, bunits=4, bprojs=4, badim=4)
    wpe = DNN_WPE(widim=5, wlayers=1, wunits=4, wprojs=4, taps=2, delay=1)
    return fe, wpe


def test_attach_wpe_draws_and_order(monkeypatch):
    """training: one numpy.random.randint over [(pass), (WPE), (beamformer)] per call, WPE or the beamformer, never both;
    eval: WPE, then the beamformer on its output, nothing drawn"""
    from espnet_amd.nets.frontends.dnn_wpe import DNN_WPE
    fe, wpe = _frontend()
    assert fe.use_wpe is False and fe.wpe is None
    with pytest.raises(TypeError):
        fe.attach_wpe(torch.nn.Identity())
    assert fe.attach_wpe(wpe) is fe and fe.use_wpe is True and fe.wpe is wpe
    assert [k for k in fe.state_dict() if k.startswith("wpe.mask_est.")]
    calls = []
    monkeypatch.setattr(DNN_WPE, "forward", lambda self, h, ilens: (calls.append("wpe"), (h + 1.0, ilens, "wmask"))[1])
    fe.beamformer.forward = lambda h, ilens: (calls.append("bf"), (h[:, :, 0] + 10.0, ilens, "bmask"))[1]
    x = torch.zeros(2, 6, 3, 5, 2)
    fe.train()
    np.random.seed(4)
    draws = [int(np.random.randint(3)) for _ in range(12)]
    assert set(draws) == {0, 1, 2}
    np.random.seed(4)
    for d in draws:
        del calls[:]
        h, _, mask = fe(x, [6, 6])
        assert calls == [[], ["wpe"], ["bf"]][d] and mask == [None, "wmask", "bmask"][d]
        assert h.dim() == (4 if d == 2 else 5) and float(h.flatten()[0]) == [0.0, 1.0, 10.0][d]
    fe.eval()
    del calls[:]
    state = np.random.get_state()[1].copy()
    h, _, mask = fe(x, [6, 6])
    assert calls == ["wpe", "bf"] and mask == "bmask" and h.dim() == 4 and float(h.flatten()[0]) == 11.0
    assert np.array_equal(np.random.get_state()[1], state)
    # WPE alone (no beamformer built): eval returns the dereverberated channels
    fe2, wpe2 = _frontend(use_beamformer=False)
    fe2.attach_wpe(wpe2).eval()
    h, _, mask = fe2(x, [6, 6])
    assert h.dim() == 5 and mask == "wmask"


def test_without_wpe_the_draws_are_unchanged():
    """no WPE attached: one numpy.random.randint(2) per call, as before this module existed"""
    fe, _ = _frontend()
    fe.train()
    calls = []
    fe.beamformer.forward = lambda h, ilens: (calls.append(1), (h[:, :, 0], ilens, None))[1]
    x = torch.zeros(2, 6, 3, 5, 2)
    np.random.seed(3)
    draws = [int(np.random.randint(2)) for _ in range(8)]
    after = np.random.get_state()[1].copy()
    np.random.seed(3)
    for d in draws:
        before = len(calls)
        fe(x, [6, 6])
        assert (len(calls) - before == 1) == bool(d)
    assert np.array_equal(np.random.get_state()[1], after)


def test_entry_points_reject_bad_arguments_without_a_device():
    from espnet_amd import _lib, ops
    lib = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.eamd_wpe_power(None, None, None, 1, 4, 4, 2, 3, None) < 0
    assert lib.eamd_wpe_power_bwd(None, None, None, None, 1, 4, 4, 2, 3, None) < 0
    assert lib.eamd_wpe_taps(None, None, None, None, None, None, 1, 40, 2, 3, 5, 3, 1e-10, 1, 1, None) < 0
    assert lib.eamd_wpe_filter(None, None, None, None, 1, 40, 2, 3, 5, 3, None) < 0
    assert lib.eamd_wpe_bwd(None, None, None, None, None, None, None, None, 1, 40, 2, 3, 5, 3, 1e-10, 1, 1, None) < 0
    # more than 64 unknowns, a negative delay, no taps, a chunk count outside 1..T, a mask longer than the spectrum
    assert lib.eamd_wpe_taps(p, p, None, p, None, p, 1, 400, 9, 3, 8, 3, 1e-10, 1, 1, None) == _lib.EAMD_EUNSUPPORTED
    assert lib.eamd_wpe_filter(p, p, None, p, 1, 400, 9, 3, 8, 3, None) == _lib.EAMD_EUNSUPPORTED
    assert lib.eamd_wpe_bwd(p, p, p, p, None, p, p, p, 1, 400, 9, 3, 8, 3, 1e-10, 1, 1, None) == _lib.EAMD_EUNSUPPORTED
    assert lib.eamd_wpe_taps(p, p, None, p, None, p, 1, 40, 2, 3, 5, -1, 1e-10, 1, 1, None) < 0
    assert lib.eamd_wpe_taps(p, p, None, p, None, p, 1, 40, 2, 3, 0, 3, 1e-10, 1, 1, None) < 0
    assert lib.eamd_wpe_taps(p, p, None, p, None, p, 1, 40, 2, 3, 5, 3, 1e-10, 1, 0, None) < 0
    assert lib.eamd_wpe_taps(p, p, None, p, None, p, 1, 40, 2, 3, 5, 3, 1e-10, 1, 41, None) < 0
    assert lib.eamd_wpe_filter(p, p, None, p, 0, 40, 2, 3, 5, 3, None) < 0
    assert lib.eamd_wpe_power(p, p, p, 1, 4, 5, 2, 3, None) < 0
    # the chunk count is a function of the shape alone, at least 64 frames per chunk
    assert ops.wpe_nchunk(2, 130, 8, 65, 8) == 3 and ops.wpe_nchunk(2, 40, 1, 5, 5) == 1
    assert ops.wpe_nchunk(8, 1000, 8, 257, 5) == ops.wpe_nchunk(8, 1000, 8, 257, 5)
    assert (ops.WPE_FTILE, ops.WPE_MAX_UNKNOWNS) == (32, 64)
