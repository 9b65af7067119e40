"""Jointly trained speech-enhancement front-end of the RNN E2E on the GPU: the kernels of csrc/feature_transform.hip
element-wise against the float64 restatement (tests/feature_transform_restatement.py), FeatureTransform and
E2E(use_frontend=True) against the reference's float64 run (tests/golden/frontend_e2e.npz).

Bounds.  The forward log-mel, the mean-only MVN in both directions and the convolution's input gradient are sums of
products: a-priori bounds (n + 8) 2^-24 sum |terms| per element, written at each test.  The log-mel backward (a quotient by
mel + 1e-20) and the MVN forward with norm_vars depend on the data: they are bounded by 4 times the error the restatement
itself makes in float32 on the CPU on the same inputs (4x: this project's margin for a differently ordered fp32
evaluation), in the measure max |a - ref| / max |ref|.  No bound is taken from the kernels.  The models use the RNN bars of
tests/test_gpu_rnn.py.  Observed on an MI355X: see the docstrings."""
import numpy as np
import pytest
import torch

import feature_transform_restatement as R
from conftest import load_golden, seeded_weights
from test_frontend_e2e import E2E_CASES, FT_TAGS, e2e_args, ft_inputs
from test_gpu_model import check_grads, load_sd

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
B = 2
TL = ((1, (1, 1)), (5, (5, 3)), (70, (70, 50)))
_CACHE = {}


@pytest.fixture(autouse=True)
def _fp32():
    import espnet_amd
    espnet_amd.set_precision("fp32")
    yield
    espnet_amd.set_precision("fp32")


@pytest.fixture(scope="module")
def golden():
    return load_golden("frontend_e2e.npz")


def nan_like(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def i32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32), device=DEV)


def ranges(nz):
    any_ = nz.any(1)
    return (np.where(any_, nz.argmax(1), 0).astype(np.int32), np.where(any_, nz.shape[1] - nz[:, ::-1].argmax(1), 0).astype(np.int32))


def mel_cases():
    """name -> melmat [F, M] float32: the real matrices of (n_fft 32, 8 filters) and (n_fft 512, 80 filters), and for every
    F in {1, 17, 65, 257} a synthetic banded non-negative matrix with an empty filter (1), a bin that no filter covers (F - 2)
    and a bin covered by three filters (0 for F = 1, else 5); 83 filters at F = 257 (more filters than lanes)"""
    if "mel" not in _CACHE:
        from espnet_amd.espnet2.frontend import mel_filterbank
        out = {"real17x8": np.ascontiguousarray(mel_filterbank(16000, 32, 8).T), "real257x80": np.ascontiguousarray(mel_filterbank(16000, 512, 80).T)}
        rng = np.random.RandomState(5)
        for F, M in ((1, 4), (17, 6), (65, 9), (257, 83)):
            w = np.zeros((F, M), np.float32)
            width = max(2, (2 * F) // M + 1)
            for m in range(M):
                s = (m * max(F - width, 0)) // max(M - 1, 1)
                w[s:s + width, m] = rng.uniform(0.1, 1.0, size=min(width, F - s))
            three = 0 if F == 1 else 5
            w[three, :] = 0
            w[three, [0, 2, 3]] = rng.uniform(0.1, 1.0, size=3)
            w[:, 1] = 0                                                        # an empty filter
            if F > 1:
                w[F - 2, :] = 0                                                # a bin that no filter covers
                assert int((w[three] > 0).sum()) == 3 and not (w[F - 2] > 0).any()
            assert not (w[:, 1] > 0).any() and int((w[three] > 0).sum()) == 3
            out["synth%dx%d" % (F, M)] = w
        _CACHE["mel"] = out
    return _CACHE["mel"]


def spectrum(F, T, lens, seed):
    """complex64 [B,T,F]: padded frames zero, bin F // 2 identically zero (F > 1), utterance 0's frame T // 2 all zero"""
    key = ("spec", F, T, lens)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        x = torch.complex(torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)) * torch.exp(2.0 * torch.randn(B, T, 1, generator=g))
        for b, n in enumerate(lens):
            x[b, n:] = 0
        if F > 1:
            x[..., F // 2] = 0
        if T > 1:
            x[0, T // 2] = 0
        _CACHE[key] = x.to(torch.complex64)
    return _CACHE[key]


def dev_ri(x):
    return R.ri(x).to(DEV)


# ---- kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["real17x8", "real257x80", "synth1x4", "synth17x6", "synth65x9", "synth257x83"])
def test_logmel_forward(name):
    """log(sum_f |x|^2 melmat + 1e-20) against float64.  The mel sum is a sum of non-negative products: relative error
    (n_terms + 8) 2^-24 with n_terms = 2 + hi - lo, which is an absolute error on the log; the log itself adds
    4 * 2^-24 |log|.  Padded frames are exactly 0, NaN pre-fill is overwritten, two launches give the same bits.
    MI355X: worst error / bound 0.56."""
    from espnet_amd import ops
    w = mel_cases()[name]
    F, M = w.shape
    lo, hi = ranges((w != 0).T)
    worst = 0.0
    for T, lens in TL:
        x = spectrum(F, T, lens, 100 + F)
        ref = R.logmel(x.to(torch.complex128), torch.from_numpy(w).double(), lens)
        bound = torch.from_numpy((2 + hi - lo + 8).astype(np.float64))[None, None, :] * U + 4 * U * ref.abs()
        args = (dev_ri(x), torch.from_numpy(w).to(DEV), i32(lo), i32(hi), i32(lens))
        out = ops.ft_logmel_fwd(*args, out=nan_like(B, T, M))
        again = ops.ft_logmel_fwd(*args, out=nan_like(B, T, M))
        torch.cuda.synchronize()
        assert torch.equal(out, again) and torch.isfinite(out).all()
        err = (out.cpu().double() - ref).abs()
        assert bool((err <= bound).all()), (name, T, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
        for b, n in enumerate(lens):
            assert torch.equal(out[b, n:], torch.zeros_like(out[b, n:]))
        if T > 1:                                                     # the all-zero valid frame sits at the floor log(1e-20)
            assert float((out[0, T // 2].cpu().double() - np.log(1e-20)).abs().max()) <= 12 * U * 47
    print("[feature transform] logmel forward %s: worst error / bound %.3f" % (name, worst))


@pytest.mark.parametrize("name", ["real17x8", "real257x80", "synth1x4", "synth17x6", "synth65x9", "synth257x83"])
def test_logmel_backward(name):
    """gradient with respect to the complex spectrum against float64 autograd of the restatement, within 4x the float32
    restatement's own error (max-abs over max-ref).  A bin without power gets exactly 0 (the all-zero frame's quotient is
    g / 1e-20), padded frames are exactly 0, nothing is NaN, two launches give the same bits.
    MI355X: worst error / (4 x float32 restatement error) 0.44."""
    from espnet_amd import ops
    w = mel_cases()[name]
    F, M = w.shape
    lo, hi = ranges((w != 0).T)
    mlo, mhi = ranges(w != 0)
    worst = 0.0
    for T, lens in TL:
        x = spectrum(F, T, lens, 100 + F)
        g = torch.randn(B, T, M, generator=torch.Generator().manual_seed(T))

        def grad(dtype):
            xi = x.to(torch.complex128 if dtype == torch.float64 else torch.complex64).clone().requires_grad_(True)
            (R.logmel(xi, torch.from_numpy(w).to(dtype), lens) * g.to(dtype)).sum().backward()
            return R.ri(xi.grad)
        ref, ref32 = grad(torch.float64), grad(torch.float32)
        args = (dev_ri(x), g.to(DEV), torch.from_numpy(w).to(DEV), i32(lo), i32(hi), i32(mlo), i32(mhi), i32(lens))
        out = ops.ft_logmel_bwd(*args, out=nan_like(B, T, F, 2))
        again = ops.ft_logmel_bwd(*args, out=nan_like(B, T, F, 2))
        torch.cuda.synchronize()
        assert torch.equal(out, again) and torch.isfinite(out).all()
        e, e32 = R.err_vs(out.cpu().double(), ref), R.err_vs(ref32.double(), ref)
        print("[feature transform] logmel backward %s T=%d: %.2e vs the fp32 restatement's %.2e" % (name, T, e, e32))
        assert e <= 4 * e32, (name, T, e, e32)
        worst = max(worst, e / (4 * e32) if e32 > 0 else float(e > 0))
        zero = (R.ri(x) == 0).all(-1)                                  # bins without power, padded frames among them
        assert torch.equal(out.cpu()[zero], torch.zeros_like(out.cpu()[zero]))
    print("[feature transform] logmel backward %s: worst error / (4 x fp32 restatement error) %.3f" % (name, worst))


MVN_T = (1, 3, 4, 5, 70)
MVN_M = (1, 8, 80, 83)


def mvn_data(T, M):
    g = torch.Generator().manual_seed(10 * T + M)
    x = 3.0 * torch.randn(B, T, M, generator=g) - 4.0
    lens = (T, max(1, T - 2))
    bias = -(3.0 * torch.randn(M, generator=g) - 4.0)
    scale = 1.0 / (0.5 + torch.rand(M, generator=g))
    return x, lens, bias, scale, torch.randn(B, T, M, generator=g)


@pytest.mark.parametrize("stats", [False, True])
def test_mvn_forward_and_backward_means_only(stats):
    """norm_vars = False, both values of norm_means (the mean-subtracted copy comes back either way), and global MVN alone.
    y[t] = z[t] - sum_t' z[t'] / len over ALL T frames with z = (x + bias) * scale: bound (T + 8) 2^-24 (|z[t]| +
    sum_t' |z[t']| / len) per element; the backward scale * (g[t] - sum_t' g[t'] / len) likewise.  Two launches give the
    same bits.  MI355X: worst error / bound 0.23 (forward), 0.16 (backward), measured with 4 sub-rows per
    column sum (16 now: shorter chains)."""
    from espnet_amd import ops
    worst = [0.0, 0.0]
    for T in MVN_T:
        for M in MVN_M:
            x, lens, bias, scale, gy = mvn_data(T, M)
            n = torch.tensor([float(v) for v in lens], dtype=torch.float64)[:, None, None]
            b64, s64 = (bias.double(), scale.double()) if stats else (torch.zeros(M, dtype=torch.float64), torch.ones(M, dtype=torch.float64))
            z = (x.double() + b64) * s64
            ref = z - z.sum(1, keepdim=True) / n
            bound = (T + 8) * U * (z.abs() + z.abs().sum(1, keepdim=True) / n)
            bs = (bias.to(DEV), scale.to(DEV)) if stats else (None, None)
            for nm in (True, False):
                out = ops.ft_mvn_fwd(x.to(DEV), i32(lens), *bs, True, nm, False, 1e-20, out=nan_like(B, T, M))
                again = ops.ft_mvn_fwd(x.to(DEV), i32(lens), *bs, True, nm, False, 1e-20, out=nan_like(B, T, M))
                torch.cuda.synchronize()
                assert torch.equal(out, again) and torch.isfinite(out).all()
                err = (out.cpu().double() - ref).abs()
                assert bool((err <= bound).all()), ("fwd", T, M, nm, float((err / bound).max()))
                worst[0] = max(worst[0], float((err / bound).max()))
            if stats:                                                  # GlobalMVN on its own: two roundings per element
                out = ops.ft_mvn_fwd(x.to(DEV), None, *bs, False, False, False, 0.0, out=nan_like(B, T, M))
                assert bool(((out.cpu().double() - z).abs() <= 4 * U * (z.abs() + (x.double() + b64).abs() * s64.abs())).all())
            gref = s64 * (gy.double() - gy.double().sum(1, keepdim=True) / n)
            gbound = (T + 8) * U * s64.abs() * (gy.double().abs() + gy.double().abs().sum(1, keepdim=True) / n)
            out = ops.ft_mvn_bwd(gy.to(DEV), i32(lens), bs[1], True, out=nan_like(B, T, M))
            again = ops.ft_mvn_bwd(gy.to(DEV), i32(lens), bs[1], True, out=nan_like(B, T, M))
            torch.cuda.synchronize()
            assert torch.equal(out, again) and torch.isfinite(out).all()
            err = (out.cpu().double() - gref).abs()
            assert bool((err <= gbound).all()), ("bwd", T, M, float((err / gbound).max()))
            worst[1] = max(worst[1], float((err / gbound).max()))
            if stats:
                out = ops.ft_mvn_bwd(gy.to(DEV), None, bs[1], False, out=nan_like(B, T, M))
                assert bool(((out.cpu().double() - s64 * gy.double()).abs() <= 2 * U * (s64 * gy.double()).abs()).all())
    print("[feature transform] mvn stats=%s: worst error / bound forward %.3f backward %.3f" % (stats, worst[0], worst[1]))


@pytest.mark.parametrize("stats", [False, True])
def test_mvn_forward_with_norm_vars(stats):
    """norm_vars = True with and without norm_means against the float64 restatement, within 4x the float32 restatement's own
    error (max-abs over max-ref).  MI355X: worst error / (4 x float32 restatement error) 0.39 (with 4 sub-rows per column sum)."""
    from espnet_amd import ops
    worst = 0.0
    for T in MVN_T:
        for M in MVN_M:
            x, lens, bias, scale, _ = mvn_data(T, M)
            bs = (bias.to(DEV), scale.to(DEV)) if stats else (None, None)
            for nm in (True, False):
                def restated(dtype):
                    h = x.to(dtype)
                    if stats:
                        h = R.global_mvn(h, bias.to(dtype), scale.to(dtype))
                    return R.utterance_mvn(h, lens, nm, True)
                ref, ref32 = restated(torch.float64), restated(torch.float32).double()
                out = ops.ft_mvn_fwd(x.to(DEV), i32(lens), *bs, True, nm, True, 1e-20, out=nan_like(B, T, M))
                again = ops.ft_mvn_fwd(x.to(DEV), i32(lens), *bs, True, nm, True, 1e-20, out=nan_like(B, T, M))
                torch.cuda.synchronize()
                assert torch.equal(out, again)
                assert torch.isfinite(out).all()        # one frame: x - mean = 0 and the variance clamps at eps
                fin = torch.isfinite(ref) & torch.isfinite(ref32)
                e, e32 = R.err_vs(out.cpu().double()[fin], ref[fin]), R.err_vs(ref32[fin], ref[fin])
                assert e <= 4 * e32, (T, M, nm, e, e32)
                worst = max(worst, e / (4 * e32) if e32 > 0 else float(e > 0))
    print("[feature transform] mvn norm_vars stats=%s: worst error / (4 x fp32 restatement error) %.3f" % (stats, worst))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv3x3_c1_input_gradient(dtype):
    """dx = sum_c sum_ij dy[t+1-i, f+1-j, c] w[c,i,j] against float64 on the values the kernel reads (bf16 dy: the rounded
    ones): 576 products per element, bound (576 + 8) 2^-24 sum |dy| |w|.  33 frames cross the 32-frame segment of a
    workgroup.  Two launches give the same bits.  MI355X: worst error / bound 0.0014."""
    from espnet_amd import ops
    C, worst = 64, 0.0
    for T, F in ((1, 1), (2, 3), (7, 9), (33, 83)):
        g = torch.Generator().manual_seed(T * 100 + F)
        dy = torch.randn(B, T, F, C, generator=g).to(dtype)
        dy[torch.rand(B, T, F, C, generator=g) < 0.4] = 0                          # ReLU-masked
        w = torch.randn(C, 1, 3, 3, generator=g) / 3.0
        ref = R.conv3x3_c1_input_grad(dy.double(), w.double())
        bound = (576 + 8) * U * R.conv3x3_c1_input_grad(dy.double().abs(), w.double().abs())
        out = ops.conv3x3_c1_bwd_x(dy.to(DEV), w.to(DEV), B, T, F, C, out=nan_like(B, T, F))
        again = ops.conv3x3_c1_bwd_x(dy.to(DEV), w.to(DEV), B, T, F, C, out=nan_like(B, T, F))
        torch.cuda.synchronize()
        assert torch.equal(out, again) and torch.isfinite(out).all()
        err = (out.cpu().double() - ref).abs()
        assert bool((err <= bound).all()), (T, F, float((err / bound.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / bound.clamp_min(1e-300))[bound > 0].max()))
    print("[feature transform] conv3x3_c1_bwd_x %s: worst error / bound %.4f" % (dtype, worst))


# ---- modules and model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", FT_TAGS)
def test_feature_transform_module_vs_reference(golden, tag, tmp_path):
    """FeatureTransform.eval() on the recorded inputs: outputs on all frames (padded ones included) and, without
    norm_vars, the gradient of sum(w * h) with respect to the complex input, within 4x the reference's own float32 error"""
    from espnet_amd.nets.frontends.feature_transform import FeatureTransform
    x, melmat, ilens, bias, _, nm, nv = ft_inputs(golden, tag, torch.float32)
    stats_file = None
    if bias is not None:
        stats_file = str(tmp_path / "stats.npy")
        np.save(stats_file, golden["ft/stats"])
    m = FeatureTransform(fs=16000, n_fft=32, n_mels=8, stats_file=stats_file, uttmvn_norm_means=nm, uttmvn_norm_vars=nv).eval()
    m.logmel.melmat.copy_(melmat)
    m.logmel.set_ranges()
    m = m.to(DEV)
    xi = R.ri(x).to(DEV).requires_grad_(not nv)
    h, hl = m(xi, ilens)
    want = torch.from_numpy(golden["ft/%s/out" % tag])
    e, e32 = R.err_vs(h.detach().cpu().double(), want), float(golden["ft/%s/err32/out" % tag])
    assert [int(v) for v in hl] == ilens and h.shape == want.shape and e <= 4 * e32, (tag, e, e32)
    if not nv:
        (h * torch.from_numpy(golden["ft/w"]).to(DEV)).sum().backward()
        wg = torch.from_numpy(golden["ft/%s/gx" % tag])
        eg, eg32 = R.err_vs(xi.grad.cpu().double(), wg), float(golden["ft/%s/err32/gx" % tag])
        assert eg <= 4 * eg32, (tag, eg, eg32)


def e2e_model(golden, case):
    from espnet_amd.nets.e2e_asr import E2E
    SW = seeded_weights()
    p = "e2e/%s/" % case
    m = E2E(17, int(golden["e2e/odim"]), e2e_args(golden, etype="vggblstmp" if case.startswith("vgg") else "blstmp"))
    sd = {k[len(p) + 3:]: torch.from_numpy(v) for k, v in golden.items() if k.startswith(p + "sd/")}
    own = m.state_dict()
    for k in golden[p + "seeded_keys"].tolist():                       # too large for the fixture: name-keyed values
        sd[k] = SW.seeded_value(k, own[k].shape, int(golden[p + "model_seed"])) * 3.0 ** 0.5
    m = load_sd(m, sd)
    m.feature_transform.logmel.set_ranges()
    return m


class _Params:
    """the parameters of `module` whose names pass `keep`, for check_grads"""

    def __init__(self, module, keep):
        self.items = [(k, p) for k, p in module.named_parameters() if keep(k)]

    def named_parameters(self):
        return self.items


@pytest.mark.parametrize("case", E2E_CASES)
def test_e2e_training_step_vs_reference(golden, case):
    """one training forward / backward with numpy seeded as recorded (the same frontend and channel draws): losses within
    1e-5 relative, accuracy within 1e-6, every parameter gradient - the frontend's included - within 5e-4 (check_grads; the
    tensors too large for the fixture against their recorded projections at the same 5e-4).  blstmp_pass: the frontend is
    not applied and receives no gradient."""
    SW = seeded_weights()
    p = "e2e/%s/" % case
    m = e2e_model(golden, case).train()
    xs, ilens, ys = torch.from_numpy(golden["e2e/xs"]).to(DEV), golden["e2e/ilens"].tolist(), torch.from_numpy(golden["e2e/ys"]).to(DEV)
    np.random.seed(int(golden[p + "seed"]))
    loss = m(xs, ilens, ys)
    for name, got in (("loss", loss), ("loss_ctc", m.loss_ctc), ("loss_att", m.loss_att)):
        want = float(golden[p + name])
        rel = abs(float(got) - want) / abs(want)
        print("[parity] frontend e2e %s %s hip %.6f ref %.6f rel %.2e" % (case, name, float(got), want, rel))
        assert rel < 1e-5
    assert abs(float(m.acc) - float(golden[p + "acc"])) < 1e-6
    loss.backward()
    fix = {k[len(p):]: v for k, v in golden.items() if k.startswith(p)}
    zero = set(golden[p + "zero_grads"].tolist())
    passthrough = int(golden[p + "draws"][0]) == 0
    grads = {k[5:]: torch.from_numpy(v) for k, v in fix.items() if k.startswith("grad/")}
    for k, prm in m.named_parameters():
        if k in zero:
            grads[k] = torch.zeros(prm.shape, dtype=torch.float64)
    if passthrough:
        for k, prm in m.frontend.named_parameters():
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, k
    full = _Params(m, lambda k: k in grads)
    probed = [(k, prm) for k, prm in m.named_parameters() if k not in grads and not (passthrough and k.startswith("frontend."))]
    assert len(full.items) + len(probed) + (len(list(m.frontend.parameters())) if passthrough else 0) == len(list(m.parameters()))
    check_grads(full, grads, tol=5e-4)
    assert sorted(k for k, _ in probed) == sorted(golden[p + "seeded_keys"].tolist())
    for k, prm in probed:
        kind, e = SW.grad_check(k, prm.grad, fix)
        print("[parity] frontend e2e %s grad %s (%s) rel err %.2e" % (case, k, kind, e))
        assert kind != "full" and e <= 5e-4, (k, e)


def test_vgg_training_step_needs_the_input_gradient_kernel(golden, monkeypatch):
    """with features that carry a gradient the VGG front-end's backward goes through eamd_conv3x3_c1_bwd_x (there is no
    other way to the beamformer); for plain features it is not called"""
    from espnet_amd import ops
    from espnet_amd import rnn_functional as R_
    m = e2e_model(golden, "vggblstmp_bf").train()
    calls = []

    def refuse(*a, **k):
        calls.append(1)
        raise RuntimeError("input-gradient kernel called")
    monkeypatch.setattr(ops, "conv3x3_c1_bwd_x", refuse)
    vgg = m.enc.enc[0]
    x = torch.randn(2, 8, 8, device=DEV)
    y, _, _ = vgg(x, [8, 8])
    y.sum().backward()
    assert not calls
    y, _, _ = vgg(x.clone().requires_grad_(True), [8, 8])
    with pytest.raises(RuntimeError, match="input-gradient kernel called"):
        y.sum().backward()
    assert calls and R_.VGG2LFn is not None


def test_e2e_eval_vs_reference(golden):
    """encode and enhance within 4x the reference's own float32 error; recognize (beam 2, ctc_weight 0.3, nbest 2): the same
    token ids, scores within 1e-4 max(1, |s|)"""
    import argparse
    m = e2e_model(golden, "blstmp_bf").train()          # enhance / recognize switch to eval themselves
    p = "e2e/eval/"
    x = R.cx(golden[p + "x"]).numpy()                    # complex64 [T, C, F]
    enhanced, mask, ilens = m.enhance([x])
    assert m.training and ilens.tolist() == [x.shape[0]]
    for name, got in (("enhanced", enhanced), ("mask", mask)):
        want = golden[p + name]
        e = R.err_vs(torch.from_numpy(got).double(), torch.from_numpy(want))
        assert got.shape == want.shape and e <= 4 * float(golden[p + "err32/" + name]), (name, e)
    hs = m.encode(x)
    assert not m.training
    e = R.err_vs(hs.cpu().double(), torch.from_numpy(golden[p + "encode"]))
    assert e <= 4 * float(golden[p + "err32/encode"]), e
    args = e2e_args(golden)
    ra = argparse.Namespace(beam_size=2, penalty=0.0, ctc_weight=0.3, maxlenratio=0.0, minlenratio=0.0, lm_weight=0.0, nbest=2)
    nb = m.recognize(x, ra, args.char_list, None)
    ids, scores = golden[p + "nbest_ids"], golden[p + "nbest_scores"]
    assert len(nb) == len(ids)
    for h, want_ids, s in zip(nb, ids, scores):
        assert [int(t) for t in h["yseq"]] == [int(t) for t in want_ids if t >= 0]
        assert abs(float(h["score"]) - float(s)) <= 1e-4 * max(1.0, abs(float(s))), (float(h["score"]), float(s))
    # the batched search takes the same route (a dict with real and imag is one of the accepted input forms)
    nbb = m.recognize_batch([dict(real=x.real.copy(), imag=x.imag.copy())], ra, args.char_list, None)
    assert len(nbb) == 1 and len(nbb[0]) >= 1 and all(np.isfinite(float(h["score"])) for h in nbb[0])
