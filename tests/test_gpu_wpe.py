"""WPE dereverberation on the GPU: the kernels of csrc/wpe.hip element-wise against the float64 restatement
(tests/wpe_restatement.py, pinned on the CPU by tests/test_wpe.py), DNN_WPE against the restated module, and the chains
through Frontend, the RNN E2E and DefaultFrontend.

Bound.  Everything here depends on the conditioning of R (cond <= about 1.5e4 on this data), so every quantity is bounded
by 4 times the error that the restatement itself makes when it runs in float32 on the CPU on the same inputs (4x: this
project's margin for a differently ordered evaluation), in the measure max |a - ref| / max |ref|.  test_wpe.py keeps that
float32 error below 1e-3, so the bound is never vacuous.  No bound is taken from the kernels.  The kernels accumulate and
solve in fp64; observed on an MI355X: see the docstrings and DESIGN.md section 4."""
import argparse
import json

import numpy as np
import pytest
import torch

import beamformer_restatement as R
import wpe_restatement as W
from conftest import load_golden, seeded_weights
from test_gpu_beamformer import nan_like, within_4x, worst_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
FS = (1, 63, 65)                 # one bin, and one below / one above two 32-bin tiles
IDS = ["C%dK%dD%d" % c[:3] for c in W.CASES]
_REF = {}


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def reference(ci, F):
    """the restatement in float64 and float32 on the live bins of case ci (bin F // 2 is identically zero for F > 1),
    computed once -> (y, z, gx on all F bins, live bin list, r64, r32); r*: x, G, power, gpower, dz of L = Re <gx, x>"""
    if (ci, F) not in _REF:
        C, K, D, T, ilens = W.CASES[ci]
        y, z = W.synth(C, T, ilens, F, zero_bin=True)
        live = [f for f in range(F) if F == 1 or f != F // 2]
        g = torch.Generator().manual_seed(5)
        gx = torch.complex(torch.randn(y.shape, generator=g), torch.randn(y.shape, generator=g)).to(torch.complex64)

        def run(cdt, rdt):
            zz = z[..., live].to(rdt).requires_grad_(True)
            yy = y[..., live].to(cdt)
            power = W.masked_power(yy, zz)
            power.retain_grad()
            x, G = W.one_iteration(yy, power, ilens, K, D, return_filter=True)
            (gx[..., live].to(cdt).conj() * x).real.sum().backward()
            return dict(x=x.detach(), G=G.detach(), power=power.detach(), gpower=power.grad, dz=zz.grad)
        _REF[(ci, F)] = (y, z, gx, live, run(torch.complex128, torch.float64), run(torch.complex64, torch.float32))
    return _REF[(ci, F)]


def filter_of(G, K, C):
    """the kernels' G [B, K*C, C, F, 2] -> complex [B, F, K, C, C]"""
    B, _, _, F, _ = G.shape
    return R.cx(G.view(B, K, C, C, F, 2).permute(0, 4, 1, 2, 3, 5).cpu())


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("ci", range(len(W.CASES)), ids=IDS)
def test_kernels_against_the_restatement(ci, F):
    """power, G, x, gpower and the logit gradient of L = Re <gx, x>, every output pre-filled with NaN: within 4x the float32
    restatement's own error; a second launch gives the same bits; the zero bin gives exact zeros in every output and
    gradient; x is exactly zero past each length.  T = 130 runs three time chunks, the others one.
    MI355X, worst error / fp32-restatement error over the grid (the bound is 4): G 0.08, x 0.15, gpower 0.19, logit gradient
    0.15; largest absolute errors 7.3e-8, 2.2e-7, 4.5e-6 and 4.2e-7 of the largest element."""
    from espnet_amd import ops
    C, K, D, T, ilens = W.CASES[ci]
    B, N = len(ilens), C * K
    y, z, gx, live, r64, r32 = reference(ci, F)
    yd, zd, gxd, lens = R.ri(y).to(DEV), z.to(DEV), R.ri(gx).to(DEV), i32(ilens)

    def launch():
        power = ops.wpe_power(yd, zd, out=nan_like(B, T, F))
        G, fac = ops.wpe_taps(yd, power, lens, K, D, out=(nan_like(B, N, C, F, 2), nan_like(B, F, N, N, 2).double()))
        x = ops.wpe_filter(yd, G, lens, K, D, out=nan_like(B, T, C, F, 2))
        gpower = ops.wpe_bwd(yd, x, gxd, power, lens, fac, K, D, out=nan_like(B, T, F))
        dz = ops.wpe_power_bwd(yd, zd, gpower, out=nan_like(1, B, C, T, F))
        return dict(power=power, G=G, fac=fac, x=x, gpower=gpower, dz=dz)
    got, again = launch(), launch()
    torch.cuda.synchronize()
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, again[k]), k
    if F > 1:
        zb = F // 2
        for k, v in (("power", got["power"][..., zb]), ("G", got["G"][..., zb, :]), ("x", got["x"][..., zb, :]),
                     ("gpower", got["gpower"][..., zb]), ("dz", got["dz"][..., zb])):
            assert float(v.abs().max()) == 0.0, k
    for b, n in enumerate(ilens):
        if n < T:
            assert float(got["x"][b, n:].abs().max()) == 0.0 and float(got["gpower"][b, n:].abs().max()) == 0.0
    assert float(got["gpower"][:, :D + K - 1].abs().max()) == 0.0
    report = []
    within_4x("G", filter_of(got["G"], K, C)[:, live], r64["G"], r32["G"], report)
    within_4x("x", R.cx(got["x"].cpu())[..., live], r64["x"], r32["x"], report)
    within_4x("gpower", got["gpower"].cpu()[..., live], r64["gpower"], r32["gpower"], report)
    within_4x("dz", got["dz"].cpu()[..., live], r64["dz"], r32["dz"], report)
    print("[wpe] kernels %s F=%d: " % (IDS[ci], F) + "; ".join(t for _, t in report))


def test_power_as_given_and_no_lengths():
    """inverse_power=False (the weights are the power itself) and lens=None (every utterance fills the batch), forward
    and backward, on the C = 2 case"""
    from espnet_amd import ops
    C, K, D, T, _ = W.CASES[1]
    F, ilens = 9, (T, T)
    y, z = W.synth(C, T, ilens, F, seed=3)
    g = torch.Generator().manual_seed(6)
    gx = torch.complex(torch.randn(y.shape, generator=g), torch.randn(y.shape, generator=g)).to(torch.complex64)

    def run(cdt, rdt):
        power = (W.masked_power(y.to(cdt), z.to(rdt)) + 0.05).requires_grad_(True)
        x = W.one_iteration(y.to(cdt), power, ilens, K, D, inverse_power=False)
        (gx.to(cdt).conj() * x).real.sum().backward()
        return x.detach(), power.grad
    r64, r32 = run(torch.complex128, torch.float64), run(torch.complex64, torch.float32)
    yd = R.ri(y).to(DEV)
    power = (W.masked_power(y, z) + 0.05).to(DEV)
    G, fac = ops.wpe_taps(yd, power, None, K, D, inverse_power=False)
    x = ops.wpe_filter(yd, G, None, K, D, out=nan_like(*yd.shape))
    gpower = ops.wpe_bwd(yd, x, R.ri(gx).to(DEV), power, None, fac, K, D, inverse_power=False, out=nan_like(*power.shape))
    report = []
    within_4x("x", R.cx(x.cpu()), r64[0], r32[0], report)
    within_4x("gpower", gpower.cpu(), r64[1], r32[1], report)
    print("[wpe] power as given: " + "; ".join(t for _, t in report))


# ---- module ------------------------------------------------------------------------------------------------------------
def _module(ci, F, **kw):
    from espnet_amd.nets.frontends.dnn_wpe import DNN_WPE
    C, K, D, T, ilens = W.CASES[ci]
    m = DNN_WPE("blstmp", F, 2, 8, 8, 0.0, taps=K, delay=D, **kw)
    return seeded_weights().fill_parameters(m, salt=40 + ci)


@pytest.mark.parametrize("ci", (1, 3), ids=("C2", "C8"))
def test_dnn_wpe_against_the_restated_module(ci):
    """2-layer, 8-unit blstmp estimator: enhanced, the returned mask, predict_mask and every parameter gradient of
    L = sum |enhanced|^2 against float64 autograd of the restated module, within 4x its own float32 error.
    MI355X: the returned mask 1.07 of that error (1.15e-7 against 1.08e-7, one sigmoid at float32 rounding on both sides),
    the worst parameter gradient 0.17, enhanced below that."""
    C, K, D, T, ilens = W.CASES[ci]
    F = 9
    m = _module(ci, F)
    y, _ = W.synth(C, T, ilens, F, seed=1)

    def run(cdt, rdt):
        sd = {k: v.detach().to(rdt).requires_grad_(True) for k, v in m.state_dict().items()}
        out = W.dnn_wpe(sd, y.to(cdt), ilens, K, D)
        (out["enhanced"].real ** 2 + out["enhanced"].imag ** 2).sum().backward()
        return out["enhanced"].detach(), out["mask"], {k: v.grad for k, v in sd.items()}
    r64, r32 = run(torch.complex128, torch.float64), run(torch.complex64, torch.float32)
    m = m.to(DEV).train()
    yd = R.ri(y).to(DEV)
    enhanced, olens, mask = m(yd, list(ilens))
    (enhanced ** 2).sum().backward()
    torch.cuda.synchronize()
    assert enhanced.shape == yd.shape and mask.shape == yd.shape[:4] and list(olens) == list(ilens) and not mask.requires_grad
    report = []
    within_4x("enhanced", R.cx(enhanced.detach().cpu()), r64[0], r32[0], report)
    within_4x("mask", mask.cpu(), r64[1], r32[1], report)
    pm, _ = m.predict_mask(yd, list(ilens))
    assert torch.equal(pm, mask)
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert set(grads) == set(r64[2]) and all(g is not None for g in grads.values())
    for k, g in grads.items():
        within_4x("d" + k, g.cpu(), r64[2][k], r32[2][k], report)
    print("[wpe] DNN_WPE %s: " % IDS[ci] + worst_of(report))


def test_two_iterations_without_a_mask():
    """iterations=2, use_dnn_mask=False (what the reference's Frontend builds for use_dnn_mask_for_wpe=False): forward"""
    ci, F = 1, 9
    C, K, D, T, ilens = W.CASES[ci]
    m = _module(ci, F, use_dnn_mask=False, iterations=2).to(DEV).eval()
    y, _ = W.synth(C, T, ilens, F, seed=2)
    r64 = W.dnn_wpe({}, y.to(torch.complex128), ilens, K, D, iterations=2, use_dnn_mask=False)["enhanced"]
    r32 = W.dnn_wpe({}, y, ilens, K, D, iterations=2, use_dnn_mask=False)["enhanced"]
    with torch.no_grad():
        enhanced, _, mask = m(R.ri(y).to(DEV), list(ilens))
    report = []
    assert mask is None and m.predict_mask(R.ri(y).to(DEV), list(ilens))[0] is None
    within_4x("enhanced", R.cx(enhanced.cpu()), r64, r32, report)
    print("[wpe] two iterations: " + report[0][1])


# ---- chains ------------------------------------------------------------------------------------------------------------
def test_eval_frontend_runs_wpe_then_the_beamformer():
    """Frontend with both stages, eval: the beamformer's output on the dereverberated spectrum = the restatement of WPE
    followed by tests/beamformer_restatement.py, within 4x the float32 chain's own error (MI355X: 0.35 enhanced, 0.79 mask)"""
    from espnet_amd.nets.frontends.dnn_wpe import DNN_WPE
    from espnet_amd.nets.frontends.frontend import Frontend
    C, K, D, T, ilens = W.CASES[2]
    F = 9
    fe = Frontend(idim=F, use_beamformer=True, blayers=1, bunits=8, bprojs=8, badim=8)
    fe.attach_wpe(DNN_WPE(widim=F, wlayers=1, wunits=8, wprojs=8, taps=K, delay=D))
    fe = seeded_weights().fill_parameters(fe, salt=47)
    y, _ = W.synth(C, T, ilens, F, seed=4)

    def run(cdt, rdt):
        sd = {k: v.detach().to(rdt) for k, v in fe.state_dict().items()}
        with torch.no_grad():
            mid = W.dnn_wpe({k[4:]: v for k, v in sd.items() if k.startswith("wpe.")}, y.to(cdt), ilens, K, D)["enhanced"]
            out = R.dnn_beamformer({k[len("beamformer."):]: v for k, v in sd.items() if k.startswith("beamformer.")}, mid, ilens)
        return out["enhanced"], out["mask_speech"]
    r64, r32 = run(torch.complex128, torch.float64), run(torch.complex64, torch.float32)
    fe = fe.to(DEV).eval()
    with torch.no_grad():
        h, _, mask = fe(R.ri(y).to(DEV), list(ilens))
    assert h.shape == (len(ilens), T, F, 2)
    report = []
    within_4x("enhanced", R.cx(h.cpu()), r64[0], r32[0], report)
    within_4x("mask_speech", mask.cpu(), r64[1], r32[1], report)
    print("[wpe] WPE -> MVDR: " + "; ".join(t for _, t in report))


def test_rnn_e2e_trains_the_wpe_mask_estimator():
    """E2E(use_frontend=True) with a DNN_WPE attached, training, the draw forced to WPE: the 5-D output goes through the
    feature transform's channel pick with its gradient, and the WPE mask estimator's parameters receive finite, non-zero
    gradients; the beamformer, which did not run, receives none"""
    from espnet_amd.nets.e2e_asr import E2E
    from espnet_amd.nets.frontends.dnn_wpe import DNN_WPE
    g = load_golden("frontend_e2e.npz")
    args = argparse.Namespace(**json.loads(str(g["e2e/args_json"])))
    m = E2E(17, int(g["e2e/odim"]), args)
    m.frontend.attach_wpe(DNN_WPE(widim=17, wlayers=1, wunits=8, wprojs=8, taps=args.wpe_taps, delay=args.wpe_delay))
    m = seeded_weights().fill_parameters(m, salt=48)
    m.feature_transform.logmel.set_ranges()
    m = m.to(DEV).train()
    xs, ilens, ys = torch.from_numpy(g["e2e/xs"]).to(DEV), g["e2e/ilens"].tolist(), torch.from_numpy(g["e2e/ys"]).to(DEV)
    seed = next(s for s in range(100) if np.random.RandomState(s).randint(3) == 1)
    np.random.seed(seed)
    loss = m(xs, ilens, ys)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    wpe = dict(m.frontend.wpe.named_parameters())
    assert wpe
    for k, p in wpe.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in m.frontend.beamformer.parameters())


def test_default_frontend_with_wpe_attached():
    """eval, frozen front-end, (B, L, C) waveform: WPE and then the beamformer in front of the log-mel features"""
    from espnet_amd.espnet2.frontend import DefaultFrontend
    from espnet_amd.nets.frontends.dnn_wpe import DNN_WPE
    from test_gpu_beamformer import CONF, _wave
    kw = dict(n_fft=64, hop_length=16, n_mels=12, fs=8000)
    fe = DefaultFrontend(frontend_conf=dict(CONF), **kw)
    fe.frontend.attach_wpe(DNN_WPE(widim=33, wlayers=1, wunits=8, wprojs=8, taps=3, delay=2))
    fe = seeded_weights().fill_parameters(fe, salt=49).to(DEV).eval()
    fe.frontend.requires_grad_(False)
    wav, lens = _wave()
    feats, flens = fe(wav.to(DEV), lens)
    assert feats.shape == (2, int(flens.max()), 12) and flens.tolist() == [51, 38] and torch.isfinite(feats).all()
    fe.frontend.use_wpe = False
    plain, _ = fe(wav.to(DEV), lens)
    assert float((plain - feats).abs().max()) > 1e-3                  # the dereverberation stage did run
