"""The WPD convolutional beamformer on the GPU: the kernels of csrc/wpd.hip element-wise against the float64 restatement
(tests/wpd_restatement.py, pinned to the reference's recorded output by tests/test_wpd.py), DNN_Beamformer("wpd" / "mpdr")
against the restated module, and the chains through Frontend and the RNN E2E.

Bound.  Everything here depends on the conditioning of Rf (cond <= about 2.4e4 on this data), so every quantity is bounded
by 4 times the error that the restatement itself makes when it runs in float32 on the CPU on the same inputs (4x: this
project's margin for a differently ordered evaluation), in the measure max |a - ref| / max |ref|.  test_wpd.py keeps that
float32 error below 1e-3, so the bound is never vacuous.  No bound is taken from the kernels.  The kernels accumulate and
solve in fp64; observed on an MI355X: see the docstrings and DESIGN.md section 4."""
import argparse
import json

import numpy as np
import pytest
import torch

import beamformer_restatement as R
import wpd_restatement as W
from conftest import load_golden, seeded_weights
from test_gpu_beamformer import nan_like, within_4x, worst_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
FS = (1, 63, 65)                 # one bin, and one below / one above two 32-bin tiles
_REF = {}


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def nan64(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float64)


def reference(ci, F):
    """the restatement in float64 and float32 on the live bins of case ci (bin F // 2 is identically zero for F > 1),
    computed once -> (y, z, phi, u, ge on all F bins, live bin list, r64, r32); r*: power, Rf, h, e and gu, gphi, gpower,
    dz of L = Re <ge, e>"""
    if (ci, F) not in _REF:
        C, K, D, T, ilens = W.CASES[ci]
        y, z, phi, u = W.inputs(ci, F, zero_bin=True)
        live = [f for f in range(F) if F == 1 or f != F // 2]
        g = torch.Generator().manual_seed(5)
        ge = torch.complex(torch.randn(len(ilens), T, F, generator=g), torch.randn(len(ilens), T, F, generator=g))

        def run(cdt, rdt):
            zz = z[..., live].to(rdt).requires_grad_(True)
            yy = y[..., live].to(cdt)
            pp, uu = phi[:, live].to(cdt).requires_grad_(True), u.to(rdt).requires_grad_(True)
            power = W.masked_power(yy, zz)
            power.retain_grad()
            r = W.wpd(yy, power, pp, uu, ilens, K, D)
            (ge[..., live].to(cdt).conj() * r["e"]).real.sum().backward()
            return dict(power=power.detach(), Rf=r["Rf"].detach(), h=r["h"].detach(), e=r["e"].detach(), gu=uu.grad,
                        gphi=pp.grad, gpower=power.grad, dz=zz.grad)
        _REF[(ci, F)] = (y, z, phi, u, ge, live, run(torch.complex128, torch.float64), run(torch.complex64, torch.float32))
    return _REF[(ci, F)]


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("ci", range(len(W.CASES)), ids=W.IDS)
def test_kernels_against_the_restatement(ci, F):
    """Rf, h, e, gu, gPhi, gpower and the logit gradient of L = Re <ge, e>, every output pre-filled with NaN: within 4x the
    float32 restatement's own error; a second launch gives the same bits; the zero bin gives exact zeros in every output
    and gradient; e and gpower are exactly zero past each length and gpower before t0.  T = 130 runs three time chunks,
    the others one or two.  With C = 1 a 1 x 1 Phi cancels from h, so gPhi is rounding noise on both sides (it passes, and
    says nothing).
    MI355X, worst error / fp32-restatement error over the grid (the bound is 4): Rf 0.66, h 0.25, e 0.32, gu 0.17, gPhi 0.21,
    gpower 0.34, logit gradient 0.60 (all on the well-conditioned C = 1 and C = 4 cases, where the float32 restatement itself
    is within 3e-7; with C = 8 every ratio is below 0.01); largest absolute errors 5.3e-8, 8.1e-8, 2.8e-7, 8.0e-7, 4.6e-7,
    2.6e-7 and 2.9e-7 of the largest element."""
    from espnet_amd import ops
    C, K, D, T, ilens = W.CASES[ci]
    B, N = len(ilens), C * (K + 1)
    y, z, phi, u, ge, live, r64, r32 = reference(ci, F)
    yd, zd, phid, ud, ged, lens = R.ri(y).to(DEV), z.to(DEV), R.ri(phi).to(DEV), u.to(DEV), R.ri(ge).to(DEV), i32(ilens)

    def launch():
        power = ops.wpe_power(yd, zd, out=nan_like(B, T, F))
        Rf = ops.wpd_cov(yd, power, lens, K, D, W.EPS, out=nan64(B, F, N, N, 2))
        h, fac, xk = ops.wpd_vector(Rf, phid, ud, out=(nan_like(B, F, N, 2), nan64(B, F, N, N, 2), nan64(B, F, N, C, 2)))
        e = ops.wpd_apply(h, yd, lens, K, D, out=nan_like(B, T, F, 2))
        gh = ops.wpd_apply_bwd(ged, yd, lens, K, D, out=nan_like(B, F, N, 2))
        gphi, gu, gRf = ops.wpd_vector_bwd(fac, xk, phid, ud, gh, out=(nan_like(B, F, C, C, 2), nan_like(B, C), nan64(B, F, N, N, 2)))
        gpower = ops.wpd_cov_bwd(yd, gRf, power, lens, K, D, W.EPS, out=nan_like(B, T, F))
        dz = ops.wpe_power_bwd(yd, zd, gpower, out=nan_like(1, B, C, T, F))
        return dict(power=power, Rf=Rf, h=h, fac=fac, xk=xk, e=e, gh=gh, gphi=gphi, gu=gu, gRf=gRf, gpower=gpower, dz=dz)
    got, again = launch(), launch()
    torch.cuda.synchronize()
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, again[k]), k
    Rc = R.cx(got["Rf"].cpu())
    assert torch.equal(Rc, Rc.conj().transpose(-1, -2))                             # exactly Hermitian
    if F > 1:
        zb = F // 2
        for k in ("power", "e", "gpower", "dz"):
            v = got[k][..., zb, :] if k == "e" else got[k][..., zb]
            assert float(v.abs().max()) == 0.0, k
        for k in ("Rf", "h", "gh", "gphi", "gRf", "xk"):
            assert float(got[k][:, zb].abs().max()) == 0.0, k
    for b, n in enumerate(ilens):
        if n < T:
            assert float(got["e"][b, n:].abs().max()) == 0.0 and float(got["gpower"][b, n:].abs().max()) == 0.0
    if D + K - 1 > 0:
        assert float(got["gpower"][:, :D + K - 1].abs().max()) == 0.0
    report = []
    within_4x("Rf", Rc[:, live], r64["Rf"], r32["Rf"], report)
    within_4x("h", R.cx(got["h"].cpu())[:, live], r64["h"], r32["h"], report)
    within_4x("e", R.cx(got["e"].cpu())[..., live], r64["e"], r32["e"], report)
    within_4x("gu", got["gu"].cpu(), r64["gu"], r32["gu"], report)
    within_4x("gphi", R.cx(got["gphi"].cpu())[:, live], r64["gphi"], r32["gphi"], report)
    within_4x("gpower", got["gpower"].cpu()[..., live], r64["gpower"], r32["gpower"], report)
    within_4x("dz", got["dz"].cpu()[..., live], r64["dz"], r32["dz"], report)
    print("[wpd] kernels %s F=%d: " % (W.IDS[ci], F) + "; ".join(t for _, t in report))


def test_weights_as_given_and_no_lengths():
    """inverse_power=False (the weights are given) and lens=None (every utterance fills the batch), forward and backward,
    on the C = 2 case"""
    from espnet_amd import ops
    ci = 1
    C, K, D, T, _ = W.CASES[ci]
    F, ilens = 9, (T, T)
    y, z, phi, u = W.inputs(ci, F, seed=3)                            # the second utterance ends in zero frames
    g = torch.Generator().manual_seed(6)
    ge = torch.complex(torch.randn(2, T, F, generator=g), torch.randn(2, T, F, generator=g))

    def run(cdt, rdt):
        w = (W.masked_power(y.to(cdt), z.to(rdt)) + 0.05).requires_grad_(True)
        r = W.wpd(y.to(cdt), w, phi.to(cdt), u.to(rdt), ilens, K, D, inverse_power=False)
        (ge.to(cdt).conj() * r["e"]).real.sum().backward()
        return r["e"].detach(), w.grad
    r64, r32 = run(torch.complex128, torch.float64), run(torch.complex64, torch.float32)
    yd, phid, ud = R.ri(y).to(DEV), R.ri(phi).to(DEV), u.to(DEV)
    w = (W.masked_power(y, z) + 0.05).to(DEV)
    Rf = ops.wpd_cov(yd, w, None, K, D, inverse_power=False)
    h, fac, xk = ops.wpd_vector(Rf, phid, ud)
    e = ops.wpd_apply(h, yd, None, K, D, out=nan_like(2, T, F, 2))
    gh = ops.wpd_apply_bwd(R.ri(ge).to(DEV), yd, None, K, D)
    _, _, gRf = ops.wpd_vector_bwd(fac, xk, phid, ud, gh)
    gw = ops.wpd_cov_bwd(yd, gRf, w, None, K, D, inverse_power=False, out=nan_like(2, T, F))
    report = []
    within_4x("e", R.cx(e.cpu()), r64[0], r32[0], report)
    within_4x("gw", gw.cpu(), r64[1], r32[1], report)
    print("[wpd] weights as given: " + "; ".join(t for _, t in report))


# ---- module ------------------------------------------------------------------------------------------------------------
MODULES = {"wpd_c3_attention": (2, "wpd", -1), "wpd_c8_ref0": (4, "wpd", 0), "mpdr_c3": (2, "mpdr", -1)}


@pytest.mark.parametrize("name", MODULES)
def test_dnn_beamformer_against_the_restated_module(name):
    """2-layer, 8-unit blstmp estimator, seeded weights: enhanced, the returned mask, ws and every parameter gradient of
    L = sum |enhanced|^2 against float64 autograd of the restated module, within 4x its own float32 error.  Under "wpd"
    and "mpdr" the noise mask is not used: its output layer gets a zero gradient or none.
    MI355X, worst ratio: wpd C = 3 3.6 (the attention reference's mlp_psd.weight, 8.6e-7 against 2.4e-7; the kernels' own gu
    is at 0.5 there, and the same module as "mvdr" on the same data has 1.1e-6 on that parameter: the error is made between
    u and the attention reference's parameters, which the three types share), enhanced 0.26; wpd C = 8 1.02 (the returned
    mask, one sigmoid at float32 rounding on both sides), ws 0.02; mpdr 1.7 (again the attention reference)."""
    from espnet_amd.nets.frontends.dnn_beamformer import DNN_Beamformer
    ci, btype, ref_channel = MODULES[name]
    C, K, D, T, ilens = W.CASES[ci]
    F = 9
    m = DNN_Beamformer(F, "blstmp", 2, 8, 8, badim=8, ref_channel=ref_channel, beamformer_type=btype, btaps=K, bdelay=D)
    m = seeded_weights().fill_parameters(m, salt=60 + ci)
    y, _ = W.synth(C, T, ilens, F, seed=1)

    def run(cdt, rdt):
        sd = {k: v.detach().to(rdt).requires_grad_(True) for k, v in m.state_dict().items()}
        out = W.dnn_beamformer(sd, y.to(cdt), ilens, btype, K, D, ref_channel)
        (out["enhanced"].real ** 2 + out["enhanced"].imag ** 2).sum().backward()
        return out["enhanced"].detach(), out["mask_speech"], out["ws"].detach(), {k: v.grad for k, v in sd.items()}
    r64, r32 = run(torch.complex128, torch.float64), run(torch.complex64, torch.float32)
    m = m.to(DEV).train()
    yd = R.ri(y).to(DEV)
    enhanced, olens, mask, parts = m(yd, list(ilens), return_all=True)
    (enhanced ** 2).sum().backward()
    torch.cuda.synchronize()
    assert enhanced.shape == (len(ilens), T, F, 2) and mask.shape == yd.shape[:4] and list(olens) == list(ilens)
    assert ("Rf" in parts) == (btype == "wpd") and ("psd_n" in parts) == (btype == "mpdr")
    report = []
    within_4x("enhanced", R.cx(enhanced.detach().cpu()), r64[0], r32[0], report)
    within_4x("mask", mask.cpu(), r64[1], r32[1], report)
    within_4x("ws", R.cx(parts["ws"].detach().cpu()), r64[2], r32[2], report)
    gmax = max(float(v.abs().max()) for v in r64[3].values() if v is not None)
    for k, p in m.named_parameters():
        if k == "ref.gvec.bias":        # in front of the softmax over channels, which is shift invariant: identically zero;
            # float64 gives rounding noise, no yardstick - a sum of B C rounded terms, as in test_gpu_beamformer.py
            print("[wpd] %s d%s: %.2e, largest gradient %.2e" % (name, k, 0.0 if p.grad is None else float(p.grad.abs().max()), gmax))
            assert p.grad is None or float(p.grad.abs().max()) <= 1e-6 * gmax, k
            continue
        if k.startswith("mask.linears.1."):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            assert r64[3][k] is None or float(r64[3][k].abs().max()) == 0.0, k
            continue
        if r64[3][k] is None:                                       # the attention reference with a fixed channel
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        within_4x("d" + k, p.grad.cpu(), r64[3][k], r32[3][k], report)
    print("[wpd] DNN_Beamformer %s: " % name + worst_of(report))


# ---- chains ------------------------------------------------------------------------------------------------------------
def test_eval_frontend_with_the_wpd_beamformer():
    """Frontend(beamformer_type="wpd"), eval: the restated chain, within 4x the float32 chain's own error (MI355X: 0.08
    enhanced, 0.96 mask)"""
    from espnet_amd.nets.frontends.frontend import Frontend
    C, K, D, T, ilens = W.CASES[2]
    F = 9
    fe = Frontend(idim=F, use_beamformer=True, blayers=1, bunits=8, bprojs=8, badim=8, beamformer_type="wpd", btaps=K, bdelay=D)
    fe = seeded_weights().fill_parameters(fe, salt=67)
    y, _ = W.synth(C, T, ilens, F, seed=4)

    def run(cdt, rdt):
        sd = {k[len("beamformer."):]: v.detach().to(rdt) for k, v in fe.state_dict().items()}
        with torch.no_grad():
            out = W.dnn_beamformer(sd, y.to(cdt), ilens, "wpd", K, D)
        return out["enhanced"], out["mask_speech"]
    r64, r32 = run(torch.complex128, torch.float64), run(torch.complex64, torch.float32)
    fe = fe.to(DEV).eval()
    with torch.no_grad():
        h, _, mask = fe(R.ri(y).to(DEV), list(ilens))
    assert h.shape == (len(ilens), T, F, 2)
    report = []
    within_4x("enhanced", R.cx(h.cpu()), r64[0], r32[0], report)
    within_4x("mask_speech", mask.cpu(), r64[1], r32[1], report)
    print("[wpd] Frontend(wpd): " + "; ".join(t for _, t in report))


def test_rnn_e2e_trains_the_mask_estimator_through_wpd():
    """E2E(use_frontend=True, beamformer_type="wpd"), one training step with the draw forced to the beamformer: the loss
    is finite and the mask estimator's recurrent layers and speech-mask output receive finite, non-zero gradients"""
    from espnet_amd.nets.e2e_asr import E2E
    g = load_golden("frontend_e2e.npz")
    conf = json.loads(str(g["e2e/args_json"]))
    conf.update(beamformer_type="wpd", btaps=2, bdelay=2)
    args = argparse.Namespace(**conf)
    m = E2E(17, int(g["e2e/odim"]), args)
    assert m.frontend.beamformer.beamformer_type == "wpd"
    m = seeded_weights().fill_parameters(m, salt=68)
    m.feature_transform.logmel.set_ranges()
    m = m.to(DEV).train()
    xs, ilens, ys = torch.from_numpy(g["e2e/xs"]).to(DEV), g["e2e/ilens"].tolist(), torch.from_numpy(g["e2e/ys"]).to(DEV)
    seed = next(s for s in range(100) if np.random.RandomState(s).randint(2) == 1)
    np.random.seed(seed)
    loss = m(xs, ilens, ys)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    seen = 0
    for k, p in m.frontend.beamformer.mask.named_parameters():
        if k.startswith("linears.1."):
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
        seen += 1
    assert seen > 0
