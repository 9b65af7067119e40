"""MVDR beamforming front-end on the GPU: the kernels of csrc/beamformer.hip element-wise against the float64 restatement
(tests/beamformer_restatement.py), the modules against the reference's float64 run (tests/golden/beamformer.npz), and
DefaultFrontend / ESPnetASRModel with an enabled frontend_conf.

Bounds.  PSD and filter application are sums of products: the a-priori bound (n + 8) 2^-24 sum |terms| per element.  The
MVDR solve and every backward kernel depend on the conditioning of the data: they are bounded by 4 times the error that
the restatement itself makes when it runs in float32 on the CPU on the same inputs (4x: this project's margin for a
differently ordered fp32 evaluation), in the fixture's measure max |a - ref| / max |ref|.  No bound is taken from the
kernels.  Observed on an MI355X: see the docstrings."""
import numpy as np
import pytest
import torch

import beamformer_restatement as R
from conftest import load_golden, seeded_weights
from test_beamformer import CASES, case_of, recorded

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
CS, FS = (2, 3, 8), (1, 63, 65, 257)
TS = ((64, 64), (65, 65), (70, 50))             # (T, Tm) with 64-frame chunks: one chunk exactly, one frame more, ragged Tm < T
B, S = 2, 2
_DATA = {}


def data(C, F, T, Tm, zero_bin=True):
    """seeded spectrum x [B,T,C,F] complex64 (a coherent source under noise; utterance 1 is 7 frames shorter than Tm, its
    padded frames zero; every utterance keeps >= 4 C frames), logits z [S,B,C,Tm,F] whose padded frames of utterance 1 are
    one constant row per (mask, channel), as the estimator's bias makes them; zero_bin: bin F // 2 is identically zero (F > 1)"""
    key = (C, F, T, Tm, zero_bin)
    if key not in _DATA:
        g = torch.Generator().manual_seed(C * 1000 + F * 10 + T)
        rn = lambda *s: torch.complex(torch.randn(*s, generator=g), torch.randn(*s, generator=g))  # noqa: E731
        x = 0.6 * rn(B, T, C, F) + rn(B, T, 1, F) * rn(C, F)
        lens = [Tm, Tm - 7]
        assert min(lens) >= 4 * C
        for b, n in enumerate(lens):
            x[b, n:] = 0
        z = 1.5 * torch.randn(S, B, C, Tm, F, generator=g)
        z[:, 1, :, lens[1]:] = z[:, 1, :, lens[1]:lens[1] + 1].clone()
        if zero_bin and F > 1:
            x[..., F // 2] = 0
        _DATA[key] = (x.to(torch.complex64), z.float(), lens)
    return _DATA[key]


def dev_ri(t):
    return R.ri(t).to(DEV)


def nan_like(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def rel(a, ref):
    return R.err_vs(a.detach().cpu().to(ref.dtype), ref)


def worst_of(report):
    return "worst " + "; ".join(t for _, t in sorted(report, reverse=True)[:2])


def within_4x(name, got, ref64, ref32, report):
    """max |got - ref64| <= 4 max |ref32 - ref64| in the measure max-abs-difference over max |ref64|"""
    e, e32 = rel(got, ref64), R.err_vs(ref32.to(ref64.dtype), ref64)
    report.append((e / e32 if e32 > 0 else float(e > 0), "%s: %.2e vs the fp32 restatement's %.2e" % (name, e, e32)))
    assert torch.isfinite(got).all(), name
    assert e <= 4 * e32, (name, e, e32)


# ---- kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CS)
def test_psd_forward(C):
    """psd, feat and the normaliser against float64, all F and T configurations.  Bound per element:
    (Tm + 8) 2^-24 sum_t (m[t] / n) |x_tc| |x_te|, the feature's the row sum of it plus 4 ulp of the row.  The zero bin
    is exactly 0.  Two launches give the same bits.  MI355X: worst error / bound 0.02 (psd), 0.02 (feat)."""
    from espnet_amd import ops
    worst = [0.0, 0.0]
    for F in FS:
        for T, Tm in TS:
            x, z, _ = data(C, F, T, Tm)
            x64, z64 = x.to(torch.complex128), z.double()
            ref = R.psd_matrices(x64, z64)
            m = R.masks_of(z64, T)
            n = m.sum(dim=2) + R.EPS
            bound = (Tm + 8) * U * torch.einsum("sbtf,btcf,btef->sbfce", m / n[:, :, None], x64.abs(), x64.abs())
            out = (nan_like(S, B, F, C, C, 2), nan_like(B, C, F), nan_like(S, B, F))
            psd, feat, nrm = ops.bf_psd(dev_ri(x), z.to(DEV), out=out)
            again = ops.bf_psd(dev_ri(x), z.to(DEV), out=tuple(nan_like(*o.shape) for o in out))
            torch.cuda.synchronize()
            for a, b in zip(out, again):
                assert torch.equal(a, b)
            got = R.cx(psd.cpu().double())
            err = (got - ref).abs()
            assert torch.isfinite(psd).all() and bool((err <= bound).all()), (F, T, float((err / bound.clamp_min(1e-300)).max()))
            worst[0] = max(worst[0], float((err / bound.clamp_min(1e-300))[bound > 0].max()))
            zb = slice(F // 2, F // 2 + 1) if F > 1 else slice(0, 0)
            assert torch.equal(psd[:, :, zb], torch.zeros_like(psd[:, :, zb]))
            assert torch.equal(psd[..., 0], psd[..., 0].transpose(-1, -2)) and torch.equal(psd[..., 1], -psd[..., 1].transpose(-1, -2))
            assert float(((nrm.cpu().double() - n) / n).abs().max()) <= (Tm + 8) * U
            fref = R.psd_feature(ref[0])
            off = 1.0 - torch.eye(C, dtype=torch.float64)
            fb = ((bound[0] * off).sum(-1) + 4 * U * (ref[0].abs() * off).sum(-1)).transpose(1, 2) / (C - 1)
            ferr = (feat.cpu().double() - fref).abs()
            assert torch.isfinite(feat).all() and bool((ferr <= fb).all()), (F, T)
            assert torch.equal(feat[:, :, zb], torch.zeros_like(feat[:, :, zb]))
            if bool((fb > 0).any()):
                worst[1] = max(worst[1], float((ferr / fb.clamp_min(1e-300))[fb > 0].max()))
    print("[beamformer] psd forward C=%d: worst error / bound psd %.3f feat %.3f" % (C, worst[0], worst[1]))


@pytest.mark.parametrize("C", CS)
def test_psd_backward(C):
    """dz for L = Re <G, psd> + <g, feat> with random G, g against float64 autograd, within 4x the float32 restatement's
    own error; a zero bin gives finite gradients.  MI355X: see the printed lines (observed <= 1.2x)."""
    from espnet_amd import ops
    report = []
    for F in FS:
        for T, Tm in TS:
            x, z, _ = data(C, F, T, Tm, zero_bin=False)
            g = torch.Generator().manual_seed(F + T)
            G = torch.complex(torch.randn(S, B, F, C, C, generator=g), torch.randn(S, B, F, C, C, generator=g)).to(torch.complex64)
            gf = torch.randn(B, C, F, generator=g)

            def grad(cdt, rdt):
                zz = z.to(rdt).requires_grad_(True)
                psd = R.psd_matrices(x.to(cdt), zz)
                L = (G.to(cdt).conj() * psd).real.sum() + (gf.to(rdt) * R.psd_feature(psd[0])).sum()
                return torch.autograd.grad(L, zz)[0]
            ref64, ref32 = grad(torch.complex128, torch.float64), grad(torch.complex64, torch.float32)
            xd, zd = dev_ri(x), z.to(DEV)
            psd, feat, nrm = ops.bf_psd(xd, zd)
            dz = ops.bf_psd_bwd(xd, zd, psd, nrm, dev_ri(G), gf.to(DEV), out=nan_like(*z.shape))
            within_4x("dz F=%d T=%d/%d" % (F, T, Tm), dz, ref64, ref32, report)
    x, z, _ = data(C, 65, 70, 50, zero_bin=True)
    xd, zd = dev_ri(x), z.to(DEV)
    psd, feat, nrm = ops.bf_psd(xd, zd)
    dz = ops.bf_psd_bwd(xd, zd, psd, nrm, torch.ones_like(psd), torch.ones_like(feat), out=nan_like(*z.shape))
    assert torch.isfinite(dz).all()
    print("[beamformer] psd backward C=%d: " % C + worst_of(report))


def _psd_pair(C, F):
    """float32-valued Hermitian (psd_s, psd_n) [B,F,C,C] complex64 from the T = 70 data, and a reference vector u [B,C]"""
    x, z, _ = data(C, F, 70, 50)
    psd = R.psd_matrices(x.to(torch.complex128), z.double()).to(torch.complex64)
    g = torch.Generator().manual_seed(C + F)
    u = torch.softmax(2.0 * torch.randn(B, C, generator=g), dim=-1)
    gw = torch.complex(torch.randn(B, F, C, generator=g), torch.randn(B, F, C, generator=g)).to(torch.complex64)
    return psd[0], psd[1], u, gw


@pytest.mark.parametrize("C", CS)
def test_mvdr_forward_and_backward(C):
    """w, and the gradients of L = Re <gw, w> at psd_s, psd_n and u, against float64 (torch.linalg.inv, autograd) within 4x
    the float32 restatement's own error on the same float32 PSDs; the all-zero bin gives w = 0 exactly."""
    from espnet_amd import ops
    report = []
    for F in FS:
        ps, pn, u, gw = _psd_pair(C, F)

        def run(cdt, rdt):
            a, b, c = ps.to(cdt).requires_grad_(True), pn.to(cdt).requires_grad_(True), u.to(rdt).requires_grad_(True)
            w = R.mvdr_vector(a, b, c)
            return (w.detach(),) + torch.autograd.grad((gw.to(cdt).conj() * w).real.sum(), (a, b, c))
        r64, r32 = run(torch.complex128, torch.float64), run(torch.complex64, torch.float32)
        zb = [F // 2] if F > 1 else []
        live = [f for f in range(F) if f not in zb]                 # the zero bin: A = 1e-15 I, checked exactly below
        psd_s, psd_n, ud = dev_ri(ps), dev_ri(pn), u.to(DEV)
        w = ops.bf_mvdr(psd_s, psd_n, ud, out=nan_like(B, F, C, 2))
        assert torch.isfinite(w).all() and torch.equal(w[:, zb], torch.zeros_like(w[:, zb]))
        gs, gn, gu = ops.bf_mvdr_bwd(psd_s, psd_n, ud, dev_ri(gw), out=(nan_like(B, F, C, C, 2), nan_like(B, F, C, C, 2), nan_like(B, C)))
        assert torch.isfinite(gs).all() and torch.isfinite(gn).all() and torch.isfinite(gu).all()
        sel = lambda t: t[:, live]  # noqa: E731
        within_4x("w F=%d" % F, R.cx(sel(w).cpu()), sel(r64[0]), sel(r32[0]), report)
        within_4x("gpsd_s F=%d" % F, R.cx(sel(gs).cpu()), sel(r64[1]), sel(r32[1]), report)
        within_4x("gpsd_n F=%d" % F, R.cx(sel(gn).cpu()), sel(r64[2]), sel(r32[2]), report)

        def gu_of(cdt, rdt):                                          # gu sums over the bins: restate it over the live ones
            a, b, c = ps[:, live].to(cdt), pn[:, live].to(cdt), u.to(rdt).requires_grad_(True)
            return torch.autograd.grad((gw[:, live].to(cdt).conj() * R.mvdr_vector(a, b, c)).real.sum(), c)[0]
        gz = ops.bf_mvdr_bwd(psd_s[:, live].contiguous(), psd_n[:, live].contiguous(), ud, dev_ri(gw[:, live]))[2]
        within_4x("gu F=%d" % F, gz.cpu(), gu_of(torch.complex128, torch.float64), gu_of(torch.complex64, torch.float32), report)
    print("[beamformer] mvdr C=%d: " % C + worst_of(report))


@pytest.mark.parametrize("C", CS)
def test_apply_forward_and_backward(C):
    """y against float64 with the bound (2 C + 8) 2^-24 sum_c |w_c| |x_c| per element (zero bin and padded frames: exactly 0);
    the filter gradient sum_t conj(gy) x within 4x the float32 restatement's error, bit-equal on a second launch."""
    from espnet_amd import ops
    report, worst = [], 0.0
    for F in FS:
        for T, Tm in TS:
            x, _, lens = data(C, F, T, Tm)
            g = torch.Generator().manual_seed(F * 7 + T)
            w = torch.complex(torch.randn(B, F, C, generator=g), torch.randn(B, F, C, generator=g)).to(torch.complex64)
            gy = torch.complex(torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)).to(torch.complex64)
            x64, w64 = x.to(torch.complex128), w.to(torch.complex128)
            ref = R.apply_vector(w64, x64)
            bound = (2 * C + 8) * U * torch.einsum("bfc,btcf->btf", w64.abs(), x64.abs())
            xd = dev_ri(x)
            y = ops.bf_apply(dev_ri(w), xd, out=nan_like(B, T, F, 2))
            err = (R.cx(y.cpu().double()) - ref).abs()
            assert torch.isfinite(y).all() and bool((err <= bound).all()), (F, T)
            worst = max(worst, float((err / bound.clamp_min(1e-300))[bound > 0].max()))
            zb = slice(F // 2, F // 2 + 1) if F > 1 else slice(0, 0)
            assert torch.equal(y[:, :, zb], torch.zeros_like(y[:, :, zb])) and float(y[1, lens[1]:].abs().max()) == 0.0
            gref = lambda cdt: torch.einsum("btf,btcf->bfc", gy.to(cdt).conj(), x.to(cdt))  # noqa: E731
            gw = ops.bf_apply_bwd(dev_ri(gy), xd, out=nan_like(B, F, C, 2))
            gw2 = ops.bf_apply_bwd(dev_ri(gy), xd, out=nan_like(B, F, C, 2))
            assert torch.equal(gw, gw2)
            within_4x("gw F=%d T=%d" % (F, T), R.cx(gw.cpu()), gref(torch.complex128), gref(torch.complex64), report)
    print("[beamformer] apply C=%d: worst forward error / bound %.3f; " % (C, worst) + worst_of(report))


def test_unsupported_channel_counts_raise():
    from espnet_amd import _lib, ops
    for C in (1, 9):
        x = torch.zeros(1, 4, C, 3, 2, device=DEV)
        with pytest.raises(_lib.EamdError):
            ops.bf_apply(torch.zeros(1, 3, C, 2, device=DEV), x)
        with pytest.raises(_lib.EamdError):
            ops.bf_psd(x, torch.zeros(2, 1, C, 4, 3, device=DEV))


# ---- modules -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_golden("beamformer.npz")


def _module(golden, name):
    from espnet_amd.nets.frontends.dnn_beamformer import DNN_Beamformer
    x, ilens, ref_channel, sd = case_of(golden, name, torch.float32)
    F = x.shape[-1]
    m = DNN_Beamformer(F, "blstmp", 2, 8, 8, 2, 0.0, 8, ref_channel=ref_channel)
    m.load_state_dict({k: v.detach() for k, v in sd.items()}, strict=True)
    return m.to(DEV), R.ri(x).to(DEV), ilens


@pytest.mark.parametrize("name", CASES)
def test_dnn_beamformer_against_the_reference(golden, name):
    """DNN_Beamformer with the fixture's weights (attention reference: c3, c8; ref_channel = 0: c2ref0): enhanced, ws, u,
    mask_speech and the parameter gradients of sum |enhanced|^2 within 4x the reference's own float32 error
    err32/<name>; the gradient of the bias in front of the channel softmax, identically zero, stays at rounding level."""
    m, x, ilens = _module(golden, name)
    want, want_g = recorded(golden, name)
    m.train()
    enhanced, olens, mask_speech, mid = m(x, ilens, return_all=True)
    (enhanced ** 2).sum().backward()
    torch.cuda.synchronize()
    assert enhanced.shape == x.shape[:2] + (x.shape[3], 2) and mask_speech.shape == x.shape[:4] and list(olens) == list(ilens)
    got = dict(enhanced=R.cx(enhanced.detach().cpu()), ws=R.cx(mid["ws"].detach().cpu()), u=mid["u"].detach().cpu(),
               mask_speech=mask_speech.cpu())
    lines, bad = [], []
    for k, v in got.items():
        e, e32 = R.err_vs(v.to(want[k].dtype), want[k]), float(golden["%s/err32/%s" % (name, k)])
        lines.append("%s %.2e / %.2e" % (k, e, e32))
        if not (torch.isfinite(torch.view_as_real(v) if v.is_complex() else v).all() and e <= 4 * e32):
            bad.append(k)
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    zero = set(golden[name + "/zero_grads"].tolist())
    assert set(want_g) | zero == set(grads), sorted(set(grads) ^ (set(want_g) | zero))
    gmax = max(float(v.abs().max()) for v in want_g.values())
    for k, v in want_g.items():
        e, e32 = R.err_vs(grads[k].double(), v), float(golden["%s/err32/grad/%s" % (name, k)])
        lines.append("d%s %.2e / %.2e" % (k, e, e32))
        if not (torch.isfinite(grads[k]).all() and e <= 4 * e32):
            bad.append("grad/" + k)
    for k in zero:      # a sum of B C terms of the size of the other gradients' terms, each rounded to 2^-24
        assert float(grads[k].abs().max()) <= 1e-6 * gmax, k
    print("[beamformer] %s error / reference's own fp32 error: " % name + "; ".join(lines))
    assert not bad, bad


# ---- model -------------------------------------------------------------------------------------------------------------
CONF = dict(use_beamformer=True, blayers=1, bunits=8, bprojs=8, badim=8)


def _wave(Bw=2, L=800, C=3):
    g = torch.Generator().manual_seed(11)
    src = torch.randn(Bw, L, 1, generator=g)
    wav = 0.5 * torch.randn(Bw, L, C, generator=g) + src * torch.tensor([1.0, -0.7, 0.4])[:C]
    lens = [L, L - 200]
    wav[1, lens[1]:] = 0
    return wav, lens


def test_default_frontend_with_beamformer():
    """eval mode, (B, L, C) waveform: DefaultFrontend(frontend_conf) = LogMel of the restatement's enhanced power spectrum
    (torch.stft in float64 -> float64 beamformer with the module's weights) to 1e-3 absolute in the log domain"""
    from espnet_amd.espnet2.frontend import DefaultFrontend
    kw = dict(n_fft=64, hop_length=16, n_mels=12, fs=8000)
    fe = seeded_weights().fill_parameters(DefaultFrontend(frontend_conf=dict(CONF), **kw), salt=31).to(DEV).eval()
    wav, lens = _wave()
    feats, flens = fe(wav.to(DEV), lens)
    Bw, L, C = wav.shape
    st = torch.stft(wav.double().transpose(1, 2).reshape(Bw * C, L), 64, 16, 64, torch.hann_window(64, dtype=torch.float64),
                    center=True, pad_mode="reflect", return_complex=True)                      # (B*C, F, T)
    x = st.view(Bw, C, st.shape[1], st.shape[2]).permute(0, 3, 1, 2).contiguous()             # (B, T, C, F)
    assert flens.tolist() == [int(v) for v in fe.stft.olens(torch.as_tensor(lens))] and x.shape[1] == int(flens.max())
    for b, n in enumerate(flens.tolist()):
        x[b, n:] = 0
    sd = {k: v.detach().cpu().double() for k, v in fe.frontend.beamformer.state_dict().items()}
    with torch.no_grad():
        enh = R.dnn_beamformer(sd, x, flens.tolist(), -1)["enhanced"]
        power = (enh.real ** 2 + enh.imag ** 2).float().to(DEV)
        want, _ = fe.logmel(power, flens)
    err = float((feats - want).abs().max())
    print("[beamformer] DefaultFrontend + MVDR: log-mel max abs err %.2e (range %.1f..%.1f)" % (err, float(want.min()), float(want.max())))
    assert feats.shape == want.shape == (Bw, int(flens.max()), 12) and torch.isfinite(feats).all() and err < 1e-3
    # the channels matter: channel 0 alone gives other features
    plain, _ = DefaultFrontend(**kw).to(DEV).eval()(wav.to(DEV), lens)
    assert float((plain - feats).abs().max()) > 1e-2
    # training mode with the front-end frozen: beamformed or passed through by the reference's draw, finite either way
    fe.train()
    fe.frontend.requires_grad_(False)
    np.random.seed(0)
    outs = [fe(wav.to(DEV), lens)[0] for _ in range(4)]
    assert all(torch.isfinite(o).all() and o.shape == feats.shape for o in outs)
    assert any(torch.equal(o, feats) for o in outs) and any(not torch.equal(o, feats) for o in outs)


def test_espnet2_model_encodes_multichannel_input():
    from espnet_amd.espnet2 import CTC, ConformerEncoder, ESPnetASRModel, TransformerDecoder, UtteranceMVN
    from espnet_amd.espnet2.frontend import DefaultFrontend
    fe = DefaultFrontend(n_fft=64, hop_length=16, n_mels=20, fs=8000, frontend_conf=dict(CONF))
    enc = ConformerEncoder(20, output_size=32, attention_heads=2, linear_units=48, num_blocks=1, dropout_rate=0.0,
                           positional_dropout_rate=0.0, attention_dropout_rate=0.0, macaron_style=True, cnn_module_kernel=7)
    dec = TransformerDecoder(30, 32, attention_heads=2, linear_units=48, num_blocks=1, dropout_rate=0.0, positional_dropout_rate=0.0)
    model = ESPnetASRModel(vocab_size=30, frontend=fe, normalize=UtteranceMVN(), encoder=enc, decoder=dec,
                           ctc=CTC(30, 32, ctc_type="builtin"), ctc_weight=0.3)
    model = seeded_weights().fill_parameters(model, salt=32).to(DEV).eval()
    wav, lens = _wave()
    with torch.no_grad():
        out, olens = model.encode(wav.to(DEV), torch.as_tensor(lens))
        feats, flens = fe(wav.to(DEV), lens)
    assert out.shape[0] == 2 and out.shape[2] == 32 and torch.isfinite(out).all()
    assert int(max(olens)) == out.shape[1] and flens.tolist() == [51, 38]


def test_default_frontend_without_conf_is_unchanged():
    """no frontend_conf (or all switches off): the code path of before the beamformer existed - Stft.spectrum -> fused
    log-mel kernel, channel 0 of a multi-channel input - restated here line for line; the features are bit-identical"""
    from espnet_amd import ops
    from espnet_amd.espnet2.frontend import DefaultFrontend
    g = load_golden("frontend.npz")
    wav, wlens = torch.from_numpy(g["wav"]).to(DEV), torch.from_numpy(g["wlens"])
    for conf in (None, dict(use_beamformer=False)):
        fe = DefaultFrontend(frontend_conf=conf).to(DEV).eval()
        assert fe.frontend is None
        feats, flens = fe(wav, wlens)
        spec, rpu, T = fe.stft.spectrum(wav)
        lens = fe.stft.olens(torch.as_tensor(wlens).cpu())
        fl = ops.h2d_cached("frontend_lens", lens.numpy().astype(np.int32), wav.device)
        want = fe.logmel.from_spectrum(spec, rpu, T, wav.size(0), fl)
        assert torch.equal(feats, want) and flens.tolist() == lens.tolist()
        assert float((feats.cpu() - torch.from_numpy(g["default_feats"])).abs().max()) < 1e-3
        wav2 = torch.stack([wav, wav.flip(0)], dim=-1)
        assert torch.equal(fe(wav2, wlens)[0], feats)
