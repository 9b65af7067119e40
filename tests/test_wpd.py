"""The WPD convolutional beamformer on the CPU: tests/wpd_restatement.py, the yardstick of the kernels of csrc/wpd.hip,
against the fixture recorded from the reference's conv_beamformer.py (tools/gen_golden_wpd.py), its closed-form backward
against float64 autograd, the length convention, the conditioning that keeps the GPU tests' bound meaningful, and the
public surface of DNN_Beamformer / Frontend.  No GPU."""
import argparse

import pytest
import torch

import wpd_restatement as W
from conftest import load_golden

F = 5
C128 = torch.complex128


def _case64(ci, F=F, seed=0):
    C, K, D, T, ilens = W.CASES[ci]
    y, z, phi, u = W.inputs(ci, F, seed=seed)
    return y.to(C128), W.masked_power(y, z).float().double(), phi.to(C128), u.double()


@pytest.fixture(scope="module")
def golden():
    return load_golden("wpd.npz")


@pytest.mark.parametrize("ci", range(len(W.CASES)), ids=W.IDS)
def test_restatement_equals_the_reference(golden, ci):
    """ws and enhanced of the reference's get_covariances -> get_WPD_filter_v2 -> perform_WPD_filtering, recorded in
    float64 (a full-length utterance from the batch, a shorter one from the reference run on it alone): 1e-10 relative.
    Observed: 5e-13 or better."""
    C, K, D, T, ilens = W.CASES[ci]
    k = W.IDS[ci]
    y, phi = W.cx(golden[k + "/y"]).to(C128), W.cx(golden[k + "/phi"]).to(C128)
    power, u = torch.from_numpy(golden[k + "/power"]).double(), torch.from_numpy(golden[k + "/u"]).double()
    assert tuple(golden[k + "/ilens"]) == ilens
    r = W.wpd(y, power, phi, u, ilens, K, D)
    e_ws, e_en = W.err_vs(r["h"], W.cx(golden[k + "/ws"])), W.err_vs(r["e"], W.cx(golden[k + "/enhanced"]))
    print("[wpd] %s vs the reference: ws %.1e enhanced %.1e" % (k, e_ws, e_en))
    assert e_ws < 1e-10 and e_en < 1e-10


@pytest.mark.parametrize("inverse_power", (True, False), ids=("inverse", "as_given"))
@pytest.mark.parametrize("ci", range(len(W.CASES)), ids=W.IDS)
def test_closed_form_backward_equals_autograd(ci, inverse_power):
    """gu, gPhi and gpower of L = Re <ge, e>: the formulas the kernels implement against float64 autograd, 1e-10 relative"""
    C, K, D, T, ilens = W.CASES[ci]
    y, power, phi, u = _case64(ci)
    if not inverse_power:
        power = power + 0.05
    g = torch.Generator().manual_seed(3)
    ge = torch.complex(torch.randn(len(ilens), T, F, generator=g, dtype=torch.float64),
                       torch.randn(len(ilens), T, F, generator=g, dtype=torch.float64))
    power, phi, u = power.requires_grad_(True), phi.requires_grad_(True), u.requires_grad_(True)
    e = W.wpd(y, power, phi, u, ilens, K, D, inverse_power=inverse_power)["e"]
    (ge.conj() * e).real.sum().backward()
    got = W.wpd_backward(y, power.detach(), phi.detach(), u.detach(), ilens, K, D, ge, inverse_power=inverse_power)
    for name, ref in (("gu", u.grad), ("gphi", phi.grad), ("gpower", power.grad)):
        if C == 1 and name == "gphi":      # a 1 x 1 Phi cancels from h = X Phi u / (X[0] Phi + 1e-15): both are rounding noise
            assert float(ref.abs().max()) < 1e-10 and float(got[name].abs().max()) < 1e-10
            continue
        assert float(ref.abs().max()) > 0
        assert W.err_vs(got[name], ref) < 1e-10, name
    assert D + K - 1 == 0 or float(got["gpower"][:, :D + K - 1].abs().max()) == 0.0
    for b, n in enumerate(ilens):
        assert float(got["gpower"][b, n:].abs().max() if n < T else 0.0) == 0.0


@pytest.mark.parametrize("ci", range(len(W.CASES)), ids=W.IDS)
def test_an_utterance_in_a_batch_equals_the_utterance_alone(ci):
    C, K, D, T, ilens = W.CASES[ci]
    y, power, phi, u = _case64(ci)
    r = W.wpd(y, power, phi, u, ilens, K, D)
    for b, n in enumerate(ilens):
        alone = W.wpd(y[b:b + 1, :n], power[b:b + 1, :n], phi[b:b + 1], u[b:b + 1], (n,), K, D)
        assert torch.equal(alone["h"][0], r["h"][b]) and torch.equal(alone["e"][0], r["e"][b, :n])
        assert float(r["e"][b, n:].abs().max() if n < T else 0.0) == 0.0


@pytest.mark.parametrize("ci", range(len(W.CASES)), ids=W.IDS)
def test_conditioning_keeps_the_gpu_bound_meaningful(ci):
    """cond(Rf) < 1e5 and the float32 restatement within 1e-3 of the float64 one on every case, so that '4x the float32
    restatement's error' (tests/test_gpu_wpd.py) is a real bound.  Observed: cond <= 1.3e4, float32 error <= 1e-4."""
    C, K, D, T, ilens = W.CASES[ci]
    for Fq in (1, 5):
        y, z, phi, u = W.inputs(ci, Fq)
        power = W.masked_power(y, z).float()
        r64 = W.wpd(y.to(C128), power.double(), phi.to(C128), u.double(), ilens, K, D)
        r32 = W.wpd(y, power, phi, u, ilens, K, D)
        cond = float(torch.linalg.cond(r64["Rf"]).max())
        errs = {k: W.err_vs(r32[k].to(C128), r64[k]) for k in ("Rf", "h", "e")}
        print("[wpd] %s F=%d: cond %.1e, float32 error " % (W.IDS[ci], Fq, cond) + " ".join("%s %.1e" % kv for kv in errs.items()))
        assert cond < 1e5
        assert all(0 < v < 1e-3 for v in errs.values()), errs


# ---- public surface ----------------------------------------------------------------------------------------------------
def _bf(**kw):
    from espnet_amd.nets.frontends.dnn_beamformer import DNN_Beamformer
    return DNN_Beamformer(9, "blstmp", 1, 8, 8, badim=8, **kw)


def test_wpd_and_mpdr_construct():
    """fails on the parent commit, where every type but "mvdr" is refused"""
    for t in ("wpd", "mpdr"):
        m = _bf(beamformer_type=t)
        assert m.beamformer_type == t and (m.btaps, m.bdelay) == (5, 3) and m.eps == 1e-6
    m = _bf(beamformer_type="wpd", btaps=2, bdelay=4)
    assert (m.btaps, m.bdelay) == (2, 4)


def test_other_types_still_raise():
    with pytest.raises(ValueError, match="gev"):
        _bf(beamformer_type="gev")
    with pytest.raises(NotImplementedError):
        _bf(beamformer_type="wpd", bnmask=3)


def test_no_taps_force_a_delay_of_one():
    assert _bf(beamformer_type="wpd", btaps=0, bdelay=3).bdelay == 1


def test_default_module_keeps_its_state_dict():
    keys = set(_bf().state_dict())
    assert keys == set(_bf(beamformer_type="wpd").state_dict()) == set(_bf(beamformer_type="mpdr").state_dict())
    assert _bf().beamformer_type == "mvdr"
    assert {"mask.linears.0.weight", "mask.linears.1.weight", "ref.mlp_psd.weight", "ref.gvec.bias"} <= keys
    assert all(k.split(".")[0] in ("mask", "ref") for k in keys)


def test_too_many_unknowns_raise_at_forward():
    """(btaps + 1) * C = 72 > 64: refused by name on the host, before the mask estimator or any kernel runs"""
    m = _bf(beamformer_type="wpd", btaps=8)
    with pytest.raises(ValueError, match=r"\(btaps \+ 1\) \* C = 64"):
        m(torch.zeros(1, 30, 8, 9, 2), [30])


def test_frontend_passes_the_type_through():
    from espnet_amd.nets.frontends.frontend import Frontend, frontend_for
    fe = Frontend(idim=9, use_beamformer=True, blayers=1, bunits=8, bprojs=8, badim=8, beamformer_type="wpd", btaps=3, bdelay=2)
    assert (fe.beamformer.beamformer_type, fe.beamformer.btaps, fe.beamformer.bdelay) == ("wpd", 3, 2)
    old = dict(use_wpe=False, wtype="blstmp", wlayers=1, wunits=8, wprojs=8, wdropout_rate=0.0, wpe_taps=5, wpe_delay=3,
               use_dnn_mask_for_wpe=True, use_beamformer=True, btype="blstmp", blayers=1, bunits=8, bprojs=8, bnmask=2,
               badim=8, ref_channel=-1, bdropout_rate=0.0)
    assert frontend_for(argparse.Namespace(**old), 9).beamformer.beamformer_type == "mvdr"     # an old argument namespace
    fe = frontend_for(argparse.Namespace(beamformer_type="mpdr", btaps=0, bdelay=3, **old), 9)
    assert (fe.beamformer.beamformer_type, fe.beamformer.bdelay) == ("mpdr", 1)
