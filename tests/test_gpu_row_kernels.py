"""Loss and row kernels against float64 on every dispatch path: eamd_lsm_loss (register forms <5> / <8> and the scalar
kernel), eamd_ctc_loss (label-prep chunks, float4 / scalar log-sum-exp loads, up to 1024-thread scans, the LDS limit of
the gradient), eamd_log_softmax_rows (register / re-reading), eamd_argmax_rows, eamd_layernorm_fwd / _bwd (vector and
generic forms, direct atomics / workspace, the 4096-block cap) with the deferred eamd_layernorm_bwd_reduce, and
eamd_reduce_sum.

Every comparison is element-wise: the largest error of a row relative to that row's scale (never a whole-tensor norm,
which hides one wrong row among hundreds).  Integer outputs match exactly; regions the kernel must define (ignored
rows, frames past hlens) are exactly 0; outputs are filled with NaN before the launch so an unwritten row fails.
Each bound is set from a run on an MI355X: at most 4x the observed error, noted beside it."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F


pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
INF = float("inf")


@pytest.fixture(scope="module")
def ops():
    from espnet_amd import ops as o
    o.set_precision("fp32")
    return o


@pytest.fixture(scope="module")
def lib():
    from espnet_amd import _lib
    return _lib


def row_err(got, ref, floor=0.0, scale=None):
    """max over rows of (max |got - ref| / the row's scale) over the last dim, in float64; the scale is max |ref| unless
    given per row (the magnitude of the operands where a row's result is a difference of much larger terms).
    Non-finite reference entries must be matched exactly; a non-finite value where the reference is finite counts as
    an infinite error."""
    g = got.detach().double().cpu().reshape(-1, got.shape[-1])
    r = ref.detach().double().cpu().reshape(-1, ref.shape[-1])
    fin = torch.isfinite(r)
    assert torch.equal(g[~fin], r[~fin]), "non-finite reference entries differ"
    d = (g - r).abs().where(fin, torch.zeros((), dtype=torch.float64))
    d = torch.where(torch.isnan(d), torch.full_like(d, INF), d)
    if scale is None:
        s = r.abs().where(fin, torch.zeros((), dtype=torch.float64)).amax(-1).clamp_min(floor)
    else:
        s = scale.detach().double().cpu().reshape(-1)
    dm = d.amax(-1)
    e = torch.where(dm == 0, torch.zeros_like(dm), dm / s)
    i = int(e.argmax())
    return float(e[i]), i


def check(name, got, ref, tol, floor=0.0, scale=None):
    e, i = row_err(got, ref, floor, scale)
    print(f"[rows] {name}: max row-relative err {e:.3e} (row {i}, tol {tol:g})")
    assert e <= tol, f"{name}: row {i} relative error {e:.3e} > {tol:g}"
    return e


def misaligned(t):
    """a copy of t whose storage starts one float past a 16-byte boundary (forces the scalar / generic kernels)"""
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------------------------------------
# label-smoothing loss
# ---------------------------------------------------------------------------------------------
LSM_LOSS_TOL = 6.5e-7  # loss row, relative to sum_v |td_v log td_v| + td_v (|x_v| + |lse|); observed 1.6e-7
LSM_GRAD_TOL = 1.4e-7  # gradient row, relative to inv_denom * max_v (softmax_v + td_v) * max(1, |lse|); observed 3.4e-8
LSM_MISALIGNED_TOL = 0.0  # scalar kernel (misaligned view) against the register kernel (aligned); observed: bit-identical


def lsm_call(lib, x, t, smoothing, inv_denom, ignore_id, want_grad=True):
    rows, V = x.shape
    loss = torch.full((rows,), NAN, device=DEV)
    correct = torch.full((rows,), NAN, device=DEV)
    grad = torch.full((rows, V), NAN, device=DEV) if want_grad else None
    p = lib.ptr
    lib.check(lib.lib().eamd_lsm_loss(p(x), p(t), p(loss), p(correct), p(grad), rows, V, ignore_id, C.c_float(smoothing),
                                      C.c_float(inv_denom), lib.stream_ptr()), "eamd_lsm_loss")
    return loss, correct, grad


def lsm_ref(x, t, smoothing, inv_denom, ignore_id):
    """transformer/label_smoothing_loss.py: KL(true_dist || softmax) per row (xlogy semantics), its gradient times
    inv_denom, and th_accuracy's per-row flag (torch.argmax on the same fp32 logits).  Row scales: the loss sums
    td_v * (x_v - lse), so fp32 carries it to ulp(|x_v| + |lse|); the gradient is softmax - td, two terms <= 1, the
    softmax exp(x_v - lse) with the relative error ulp(|lse|)."""
    xd = x.double().cpu()
    tc = t.cpu()
    V = xd.shape[1]
    keep = tc != ignore_id
    logp = torch.log_softmax(xd, -1)
    td = torch.full_like(xd, smoothing / (V - 1))
    td.scatter_(1, tc.clamp_min(0)[:, None], 1.0 - smoothing)
    terms = torch.xlogy(td, td) - td * logp
    loss = terms.sum(-1).where(keep, torch.zeros((), dtype=torch.float64))
    lse = torch.logsumexp(xd, -1, keepdim=True)
    scale = (torch.xlogy(td, td).abs() + td * (xd.abs() + lse.abs())).sum(-1)
    grad = ((logp.exp() - td) * inv_denom).where(keep[:, None], torch.zeros((), dtype=torch.float64))
    gscale = inv_denom * (logp.exp() + td).amax(-1) * lse[:, 0].abs().clamp_min(1.0)
    correct = ((x.cpu().argmax(-1) == tc) & keep).float()
    return loss, scale, grad, gscale, correct


def lsm_tie_pairs(V):
    """(i, j) index pairs given equal maximal logits: within one float4, across lanes of one wave, across waves, across
    the NV register chunks (i, i + 1024 k) and the row's ends"""
    cand = [(9, 10), (8, 11), (13, 162), (40, 801), (50, 50 + 1024), (50, 50 + 3 * 1024), (77, 77 + 7 * 1024),
            (0, V - 1), (V - 2, V - 1)]
    return sorted({(i, j) for i, j in cand if 0 <= i < j < V})


def lsm_case(V, seed):
    g = torch.Generator().manual_seed(seed)
    pairs = lsm_tie_pairs(V)
    rows = 6 + 2 * len(pairs)
    x = torch.randn(rows, V, generator=g)
    t = torch.randint(0, V, (rows,), generator=g)
    x[0] = 0.25                           # constant row: every index ties, argmax 0
    x[1] *= 50.0
    x[2] *= 50.0
    t[1] = int(x[1].argmax())
    t[3] = t[5] = -1                      # ignored
    for k, (i, j) in enumerate(pairs):
        for h in range(2):
            r = 6 + 2 * k + h
            x[r, i] = x[r, j] = float(x[r].max()) + 3.0
            t[r] = i if h == 0 else j     # target at the later index of a tie: not correct
    return x, t


@pytest.mark.parametrize("V", [2, 17, 4999, 5000, 5116, 5120, 5124, 8188, 8192, 8196, 12000])
def test_lsm_loss_vs_float64(ops, lib, V):
    x, t = lsm_case(V, 1000 + V)
    xd, td = x.to(DEV), t.to(DEV)
    for smoothing in (0.0, 0.1, 0.3):
        inv = 1.0 / 7
        loss, correct, grad = lsm_call(lib, xd, td, smoothing, inv, -1)
        rl, rs, rg, gs, rc = lsm_ref(x, t, smoothing, inv, -1)
        ign = t == -1
        assert torch.equal(correct.cpu(), rc), f"V={V} s={smoothing}: correct_rows {correct.cpu().tolist()} != {rc.tolist()}"
        assert (loss.cpu()[ign] == 0).all() and (grad.cpu()[ign] == 0).all()
        e = float(((loss.cpu().double() - rl).abs() / rs).max())
        print(f"[rows] lsm_loss V={V} s={smoothing}: max loss err / scale {e:.3e} (tol {LSM_LOSS_TOL:g})")
        assert e <= LSM_LOSS_TOL
        check(f"lsm_grad V={V} s={smoothing}", grad, rg, LSM_GRAD_TOL, scale=gs)
        if smoothing == 0.1:
            loss2, correct2, _ = lsm_call(lib, xd, td, smoothing, inv, -1, want_grad=False)
            assert torch.equal(loss2, loss) and torch.equal(correct2, correct)
    # every row ignored
    tall = torch.full_like(td, -1)
    loss, correct, grad = lsm_call(lib, xd, tall, 0.1, 1.0, -1)
    assert (loss == 0).all() and (correct == 0).all() and (grad == 0).all()


def test_lsm_loss_misaligned_scalar_kernel(ops, lib):
    """V = 5000 from a view one float off a 16-byte boundary runs the scalar kernel: same answer as the register kernel"""
    V = 5000
    x, t = lsm_case(V, 77)
    xa, td = x.to(DEV), t.to(DEV)
    xm = misaligned(xa)
    for smoothing in (0.0, 0.1):
        la, ca, ga = lsm_call(lib, xa, td, smoothing, 0.5, -1)
        lm, cm, gm = lsm_call(lib, xm, td, smoothing, 0.5, -1)
        rl, rs, rg, gs, rc = lsm_ref(x, t, smoothing, 0.5, -1)
        assert torch.equal(cm.cpu(), rc) and torch.equal(ca.cpu(), rc)
        e = float(((lm - la).abs().cpu().double() / rs).max())
        print(f"[rows] lsm_loss misaligned vs aligned s={smoothing}: {e:.3e} (tol {LSM_MISALIGNED_TOL:g})")
        assert e <= LSM_MISALIGNED_TOL
        check(f"lsm_grad misaligned vs aligned s={smoothing}", gm, ga, LSM_MISALIGNED_TOL, scale=gs)
        check(f"lsm_grad misaligned s={smoothing}", gm, rg, LSM_GRAD_TOL, scale=gs)


# ---------------------------------------------------------------------------------------------
# CTC loss
# ---------------------------------------------------------------------------------------------
# The lattice sums log-probabilities x_v - lse_t: fp32 carries each to ulp(|lse_t|), so an utterance's nll is scaled
# by sum_t |lse_t| (floor 1).  A gradient row is softmax minus occupancies, terms <= 1 that cancel on peaked rows,
# exponentials of log-space values of magnitude |lse_t| (softmax) and |nll| (alpha + beta): it is scaled by
# grad_scale * max_v (softmax_v + occupancy_v) * max(1, |lse_t|, |nll|).
CTC_NLL_TOL = 3.3e-7  # |nll - ref| / sum_t |lse_t|; observed 8.2e-8
CTC_GRAD_TOL = 1.4e-6  # gradient row (one frame of one utterance) relative to its scale; observed 3.5e-7
CTC_ROWSUM_TOL = 1.4e-6  # |sum_v grad[t, b, v]| relative to the row's scale; observed 3.5e-7


def ctc_call(lib, acts, ys, hl, grad_scale=1.0, want_grad=True, time_major=False, blank=0, ignore_id=-1):
    if time_major:
        T, B, V = acts.shape
        st, sb = B * V, V
    else:
        B, T, V = acts.shape
        st, sb = V, T * V
    L = lib.lib()
    Lmax = ys.shape[1]
    ws = torch.empty(int(L.eamd_ctc_workspace_bytes(B, T, Lmax)), device=DEV, dtype=torch.uint8)
    nll = torch.full((B,), NAN, device=DEV)
    grad = torch.full_like(acts, NAN) if want_grad else None
    p = lib.ptr
    lib.check(L.eamd_ctc_loss(p(acts), C.c_int64(st), C.c_int64(sb), p(ys), p(hl), p(nll), p(grad), C.c_int64(st),
                              C.c_int64(sb), p(ws), B, T, V, Lmax, blank, ignore_id, C.c_float(grad_scale),
                              lib.stream_ptr()), "eamd_ctc_loss")
    return nll, grad


def ctc_ref(oracle, x, ys, hl, grad_scale):
    """per-utterance nll (oracle.ctc_loss on each utterance alone, float64), grad_scale * d(sum nll)/dx, and the scales
    of both (see CTC_NLL_TOL)"""
    xd = x.double().requires_grad_(True)
    nll = [oracle.ctc_loss(xd[b:b + 1], hl[b:b + 1], ys[b:b + 1], use_builtin=True) for b in range(x.shape[0])]
    (grad_scale * sum(nll)).backward()
    lse = torch.logsumexp(x.double(), -1)
    valid = torch.arange(x.shape[1])[None, :] < hl[:, None].long()
    nscale = (lse.abs() * valid).sum(-1).clamp_min(1.0)
    p = torch.softmax(x.double(), -1)
    occ = (p - xd.grad / grad_scale) * valid[..., None]
    nll = torch.stack([n.detach() for n in nll])
    gscale = grad_scale * (p + occ).amax(-1) * torch.maximum(lse.abs(), nll.abs()[:, None]).clamp_min(1.0)
    return nll, xd.grad, nscale, gscale


def ctc_case(seed, T, V, hl, labels, boost, scale=1.0, ramp=0.0):
    """logits [B, T, V]: scale * randn (+ ramp * v, maxima rising along the row); with boost > 0 each utterance's labels
    and blank are raised by `boost` over the row maximum along an even alignment (a trained model's peaked posteriors:
    the log-space lattice then stays O(10) in magnitude, where fp32 carries it to ~1e-7).  labels: lists of ints, -1
    entries are holes left in ys_pad"""
    g = torch.Generator().manual_seed(seed)
    B = len(labels)
    x = scale * torch.randn(B, T, V, generator=g) + ramp * torch.arange(V, dtype=torch.float32)
    Lmax = max(1, max(len(y) for y in labels))
    ys = torch.full((B, Lmax), -1, dtype=torch.int64)
    for b, y in enumerate(labels):
        ys[b, :len(y)] = torch.tensor(y, dtype=torch.int64)
        if boost <= 0:
            continue
        lab = [v for v in y if v != -1]
        tb = hl[b]
        tok = [0] * tb
        for k, v in enumerate(lab):
            tok[int((k + 0.5) * tb / len(lab))] = v
        for f in range(tb):
            x[b, f, tok[f]] = float(x[b, f].max()) + boost
    return x, ys, torch.tensor(hl, dtype=torch.int32)


def rand_labels(g, n, V):
    return torch.randint(1, V, (n,), generator=g).tolist()


def ctc_compare(name, oracle, lib, x, ys, hl, grad_scale, time_major=False):
    rn, rg, ns, gs = ctc_ref(oracle, x, ys, hl, grad_scale)
    acts = (x.transpose(0, 1).contiguous() if time_major else x).to(DEV)
    nll, grad = ctc_call(lib, acts, ys.to(DEV), hl.to(DEV), grad_scale, time_major=time_major)
    grad = grad.cpu()
    if time_major:
        grad = grad.transpose(0, 1)
    e = float(((nll.cpu().double() - rn).abs() / ns).max())
    print(f"[rows] {name} nll: max err {e:.3e} (tol {CTC_NLL_TOL:g})  nll {[round(float(v), 3) for v in rn]}")
    assert e <= CTC_NLL_TOL
    for b in range(x.shape[0]):
        assert (grad[b, int(hl[b]):] == 0).all(), f"{name}: frames of utterance {b} past hlens not zeroed"
    check(f"{name} grad", grad, rg, CTC_GRAD_TOL, scale=gs)
    valid = torch.arange(x.shape[1])[None, :] < hl[:, None].long()
    e = float((grad.double().sum(-1).abs() / gs)[valid].max())
    print(f"[rows] {name} grad row sums: max |sum| / scale {e:.3e} (tol {CTC_ROWSUM_TOL:g})")
    assert e <= CTC_ROWSUM_TOL
    return nll, grad


@pytest.mark.parametrize("time_major", [False, True])
def test_ctc_config2_vs_float64(ops, lib, oracle, time_major):
    """B = 8, T' = 249, V = 5000, label lengths up to 100 (two 64-label chunks of the prep kernel), ragged hlens, a row
    with ignore_id holes; both layouts, the gradient returned in the input layout"""
    V = 5000
    g = torch.Generator().manual_seed(249)
    lens = [100, 90, 70, 65, 64, 63, 30, 1]
    labels = [rand_labels(g, n, V) for n in lens]
    labels[2][10:10] = [-1, -1]                   # holes in the middle of a row
    labels[3][64:64] = [-1]                       # a hole on the chunk boundary
    hl = [249, 230, 160, 140, 130, 128, 70, 5]
    x, ys, hlt = ctc_case(2490, 249, V, hl, labels, boost=8.0)
    ctc_compare(f"ctc_config2[time_major={time_major}]", oracle, lib, x, ys, hlt, 0.37, time_major=time_major)


def test_ctc_scalar_loads_and_large_logits(ops, lib, oracle):
    """V = 4999 (rows not float4-divisible: scalar log-sum-exp loads); logits x30 with maxima rising along the row (the
    running-max rescale of the one-pass log-sum-exp), on the float4 (V = 1000) and scalar (V = 999) loads"""
    g = torch.Generator().manual_seed(4999)
    labels = [rand_labels(g, n, 999) for n in (20, 11, 3, 24)]
    x, ys, hl = ctc_case(4999, 50, 4999, [50, 41, 9, 50], labels, boost=8.0)
    ctc_compare("ctc_V4999", oracle, lib, x, ys, hl, 0.5)
    for V in (1000, 999):
        x, ys, hl = ctc_case(V, 60, V, [60, 33, 48], labels[:3], boost=5.0, scale=30.0, ramp=0.2)
        ctc_compare(f"ctc_x30_ramp_V{V}", oracle, lib, x, ys, hl, 2.0)


def test_ctc_lds_limit(ops, lib, oracle):
    """V = 16384 is the widest vocabulary the gradient's LDS table holds; V = 16385 is refused with a gradient and runs
    without one"""
    from espnet_amd._lib import EamdError
    g = torch.Generator().manual_seed(16384)
    labels = [rand_labels(g, 7, 16384), rand_labels(g, 3, 16384)]
    x, ys, hl = ctc_case(16384, 24, 16384, [24, 17], labels, boost=8.0)
    ctc_compare("ctc_V16384", oracle, lib, x, ys, hl, 1.0)
    x, ys, hl = ctc_case(16385, 24, 16385, [24, 17], labels, boost=8.0)
    with pytest.raises(EamdError):
        ctc_call(lib, x.to(DEV), ys.to(DEV), hl.to(DEV), want_grad=True)
    nll, _ = ctc_call(lib, x.to(DEV), ys.to(DEV), hl.to(DEV), want_grad=False)
    rn, _, ns, _ = ctc_ref(oracle, x, ys, hl, 1.0)
    e = float(((nll.cpu().double() - rn).abs() / ns).max())
    print(f"[rows] ctc_V16385 nll (no gradient): {e:.3e} (tol {CTC_NLL_TOL:g})")
    assert e <= CTC_NLL_TOL


def test_ctc_longest_labels(ops, lib, oracle):
    """label length 511 (S = 1023 states: a 1024-thread scan) over 1100 frames; 512 is refused before any launch"""
    from espnet_amd._lib import EamdError
    V = 600
    g = torch.Generator().manual_seed(511)
    labels = [rand_labels(g, 511, V), rand_labels(g, 300, V)]
    x, ys, hl = ctc_case(511, 1100, V, [1100, 901], labels, boost=8.0)
    ctc_compare("ctc_L511", oracle, lib, x, ys, hl, 1.0)
    ys512 = torch.randint(1, V, (2, 512), generator=g)
    with pytest.raises(EamdError):
        ctc_call(lib, x.to(DEV), ys512.to(DEV), hl.to(DEV))


def test_ctc_prefetch_edges_and_feasibility(ops, lib, oracle):
    """hlens 1, 7, 8, 9, 17 around the 8-frame emission prefetch of the scan (diffuse logits); the shortest feasible
    input for repeated labels (L + repeats frames) and one frame less (+inf); hlens = 0"""
    g = torch.Generator().manual_seed(17)
    labels = [rand_labels(g, n, 64) for n in (1, 3, 4, 2, 8)]
    labels[4][2] = labels[4][3]                   # a repeat
    x, ys, hl = ctc_case(17, 17, 64, [1, 7, 8, 9, 17], labels, boost=0.0)
    ctc_compare("ctc_prefetch_edges", oracle, lib, x, ys, hl, 0.25)
    # [3, 3, 4, 4, 4, 5]: 6 labels + 3 repeats need 9 frames
    lab = [3, 3, 4, 4, 4, 5]
    x, ys, hl = ctc_case(9, 9, 8, [9, 8], [lab, lab], boost=0.0)
    nll, _ = ctc_call(lib, x.to(DEV), ys.to(DEV), hl.to(DEV), want_grad=False)
    rn = torch.stack([oracle.ctc_loss(x[b:b + 1].double(), hl[b:b + 1], ys[b:b + 1]) for b in range(2)])
    assert math.isfinite(float(nll[0])) and math.isinf(float(rn[1]))
    assert float(nll[1]) == INF
    assert abs(float(nll[0]) - float(rn[0])) <= CTC_NLL_TOL * float(torch.logsumexp(x[0].double(), -1).abs().sum())
    x, ys, hl = ctc_case(9, 9, 8, [9], [lab], boost=0.0)
    ctc_compare("ctc_minimal_T", oracle, lib, x, ys, hl, 1.0)
    # hlens = 0: an empty label costs 0, a non-empty one is infeasible; no frame has a gradient
    ys0 = torch.tensor([[-1, -1], [4, 5]])
    x = torch.randn(2, 6, 8, generator=g)
    nll, grad = ctc_call(lib, x.to(DEV), ys0.to(DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    assert nll.cpu().tolist() == [0.0, INF]
    assert (grad == 0).all()


# ---------------------------------------------------------------------------------------------
# log_softmax_rows / argmax_rows
# ---------------------------------------------------------------------------------------------
LOGSOFTMAX_TOL = 6.6e-7  # row relative to max(1, max |ref|); observed 1.7e-7
LOGSOFTMAX_LSE_TOL = 6.6e-7  # |logsumexp(row)| relative to max(1, |logsumexp(x)|); observed 1.6e-7


def row_set(V, rows, seed):
    """rows x V logits: random, then (when there are rows to spare) a constant row, a x100 row, a row with -inf
    entries (masked vocabulary) and rows with two equal maxima at index pairs around the strides of the kernels"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g)
    pairs = sorted({(i, j) for i, j in [(5, 69), (5, 261), (0, V - 1), (7, 7 + 1024), (300, 300 + 3 * 256),
                                        (11, 11 + 6144), (6143, 6144), (100, 100 + 4 * 6144)] if 0 <= i < j < V})
    special = [("const", None), ("x100", None), ("ninf", None)] + [("tie", p) for p in pairs]
    if rows < 3 or V < 2:
        return x
    for r, (kind, p) in enumerate(special[:rows]):
        if kind == "const":
            x[r] = -1.5
        elif kind == "x100":
            x[r] *= 100.0
        elif kind == "ninf":
            x[r, torch.randperm(V, generator=g)[: max(1, V // 3)]] = -INF
            x[r, V // 2] = 0.0        # keep one finite entry
        else:
            i, j = p
            x[r, i] = x[r, j] = float(x[r].max()) + 1.0
    return x


@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 5000, 6143, 6144, 6145, 12000, 50000])
def test_log_softmax_rows_vs_float64(ops, lib, V):
    for rows in (1, 10, 320):
        x = row_set(V, rows, V * 7 + rows)
        xd = x.to(DEV)
        y = torch.full_like(xd, NAN)
        lib.check(lib.lib().eamd_log_softmax_rows(lib.ptr(xd), lib.ptr(y), rows, V, lib.stream_ptr()),
                  "eamd_log_softmax_rows")
        ref = torch.log_softmax(x.double(), -1)
        check(f"log_softmax V={V} rows={rows}", y, ref, LOGSOFTMAX_TOL, floor=1.0)
        # y = x - lse(x) in fp32: lse(x) is rounded to ulp(|lse(x)|)
        lse = torch.logsumexp(y.cpu().double(), -1).abs() / torch.logsumexp(x.double(), -1).abs().clamp_min(1.0)
        lse = float(lse.max())
        print(f"[rows] log_softmax V={V} rows={rows}: max |logsumexp(row)| / scale {lse:.3e} (tol {LOGSOFTMAX_LSE_TOL:g})")
        assert lse <= LOGSOFTMAX_LSE_TOL
        assert torch.equal(ops.log_softmax_rows(xd), y)


@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 5000, 6143, 6144, 6145, 12000, 50000])
def test_argmax_rows_bit_exact(ops, lib, V):
    for rows in (1, 10, 320):
        x = row_set(V, rows, V * 11 + rows)
        if rows > 3:
            x[-1] = -INF          # all -inf: the kernel answers 0 (as torch.argmax does); pinned, not a contract of the reference
        xd = x.to(DEV)
        out = torch.full((rows,), -7, device=DEV, dtype=torch.int32)
        lib.check(lib.lib().eamd_argmax_rows(lib.ptr(xd), C.c_int64(V), lib.ptr(out), rows, V, lib.stream_ptr()),
                  "eamd_argmax_rows")
        want = x.argmax(-1)
        assert torch.equal(out.cpu().long(), want), f"V={V} rows={rows}: rows {(out.cpu().long() != want).nonzero().flatten().tolist()}"
        if rows > 3:
            assert int(out[-1]) == 0
        assert torch.equal(ops.argmax_rows(xd), out)


@pytest.mark.parametrize("V", [7, 300, 6145])
def test_selection_kernels_agree_on_the_first_maximum(ops, V):
    """argmax_rows, topk_rows(k = 1) and transducer_expand_rows (top-1 over tokens 1..V of a row with a column 0 in
    front) name the same element: the larger value and, of equal values, the lower index (csrc/select.h).  NaN-free rows
    only: argmax_rows skips a NaN, the top-k kernels rank it as -inf."""
    g = torch.Generator().manual_seed(V)

    def distinct():
        # distinct multiples of 1/8: x - lse (|.| < 1024, ulp <= 6.1e-5) keeps them distinct, so the subtraction of
        # transducer_expand_rows cannot turn two neighbours into a tie the other two kernels do not see
        return torch.randperm(V, generator=g).float() / 8

    x = torch.empty(6, V)
    x[0] = 0.75                                             # constant: index 0
    x[1] = -INF                                             # -inf only: index 0
    x[2] = distinct()                                       # a tie at the top, far apart: the lower index
    x[2, 1] = x[2, V - 2] = V
    x[3] = -1 - distinct()                                  # -0 in front of +0 at the top of a negative row
    x[3, 2], x[3, V - 1] = -0.0, 0.0
    x[4] = -1 - distinct()                                  # +0 in front of -0
    x[4, 2], x[4, V - 1] = 0.0, -0.0
    x[5] = distinct() - V / 16
    want = torch.tensor([0, 0, 1, 2, 2, int(x[5].argmax())])
    xd = x.to(DEV)
    am = ops.argmax_rows(xd).cpu().long()
    tk = ops.topk_rows(xd, 1)[1].cpu().reshape(-1)
    rows, _ = ops.transducer_expand_rows(torch.cat([torch.zeros(6, 1), x], 1).to(DEV), 1)
    ex = torch.tensor([r[1][0][1] - 1 for r in rows])
    assert torch.equal(am, want), f"argmax_rows {am.tolist()} != {want.tolist()}"
    assert torch.equal(tk, am), f"topk_rows {tk.tolist()} != argmax_rows {am.tolist()}"
    assert torch.equal(ex, am), f"transducer_expand_rows {ex.tolist()} != argmax_rows {am.tolist()}"


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------
# x_hat = (x - mean) rstd: the fp32 mean is rounded to ulp(|mean|), so x_hat carries an error kappa = 1 + |mean| rstd
# times its own ulp (kappa ~ 1000 for the rows of mean 1000 and unit variance; 1 for a constant row, whose mean is
# exact).  Scales: y and dx rows max |.| * kappa; dgamma max_v |dgamma0_v| + sum_r |dy_rv| (|x_hat_rv| + kappa_r - 1);
# dbeta max_v |dbeta0_v| + sum_r |dy_rv|.
LN_FWD_TOL = 8.6e-7  # y row relative to its scale; observed 2.2e-7
LN_STAT_TOL = 5.9e-7  # mean (relative to max(1, |mean|)) and rstd (relative); observed 1.5e-7
LN_DX_TOL = 9.1e-7  # dx row relative to its scale; observed 2.3e-7
LN_DGB_TOL = 4.9e-7  # dgamma / dbeta relative to their scale; observed 1.2e-7
LN_ROUND_TOL = 8.6e-7  # two orders of the same fp32 sums (misaligned vs aligned, deferred vs immediate reduction); observed 2.2e-7


def ln_inputs(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g)
    if rows >= 3:
        x[0] = 0.75                              # constant row: variance 0, rstd = 1 / sqrt(eps)
        x[1] += 1000.0                           # mean 1000, unit variance
        x[2] = 1000.0 + torch.randn(D, generator=g)
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g)
    dres = torch.randn(rows, D, generator=g)
    dg0 = torch.randn(D, generator=g)
    db0 = torch.randn(D, generator=g)
    return x, gamma, beta, dy, dres, dg0, db0


def ln_ref(x, gamma, beta, dy, eps):
    """float64 F.layer_norm with autograd -> y, mean, rstd, dx, dgamma, dbeta, and the scales (see LN_FWD_TOL):
    kappa per row, the dgamma and dbeta scales for zero initial values"""
    xd = x.double().requires_grad_(True)
    gd = gamma.double().requires_grad_(True)
    bd = beta.double().requires_grad_(True)
    y = F.layer_norm(xd, (x.shape[1],), gd, bd, eps)
    y.backward(dy.double())
    xx = x.double()
    mean = xx.mean(-1)
    var = xx.var(-1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    kappa = torch.where(var == 0, torch.ones_like(var), 1.0 + mean.abs() * rstd)
    xh = (xx - mean[:, None]) * rstd[:, None]
    ady = dy.double().abs()
    sg = (ady * (xh.abs() + kappa[:, None] - 1.0)).sum(0)
    sb = ady.sum(0)
    return y.detach(), mean, rstd, xd.grad, gd.grad, bd.grad, kappa, sg, sb


def ln_fwd_call(lib, x, gamma, beta, eps):
    rows, D = x.shape
    y = torch.full((rows, D), NAN, device=DEV)
    mean = torch.full((rows,), NAN, device=DEV)
    rstd = torch.full((rows,), NAN, device=DEV)
    p = lib.ptr
    lib.check(lib.lib().eamd_layernorm_fwd(p(x), p(gamma), p(beta), p(y), None, p(mean), p(rstd), rows, D, C.c_float(eps),
                                           lib.stream_ptr()), "eamd_layernorm_fwd")
    return y, mean, rstd


def ln_bwd_call(lib, dy, x, gamma, mean, rstd, dres, dg, db, deferred=False):
    """-> dx (NaN-filled before the launch), workspace; deferred: dgamma = dbeta = NULL, the partials stay in the workspace"""
    rows, D = x.shape
    L = lib.lib()
    ws = torch.full((int(L.eamd_layernorm_bwd_workspace(rows, D)),), NAN, device=DEV)
    dx = torch.full((rows, D), NAN, device=DEV)
    p = lib.ptr
    lib.check(L.eamd_layernorm_bwd(p(dy), p(x), p(gamma), p(mean), p(rstd), p(dres), p(dx), None if deferred else p(dg),
                                   None if deferred else p(db), p(ws), rows, D, lib.stream_ptr()), "eamd_layernorm_bwd")
    return dx, ws


def ln_check_all(name, lib, x, gamma, beta, dy, dres, dg0, db0, eps, xdev=None):
    yr, mr, rr, dxr, dgr, dbr, kappa, sg, sb = ln_ref(x, gamma, beta, dy, eps)
    dxr = dxr + (0 if dres is None else dres.double())
    sc = dict(y=yr.abs().amax(-1) * kappa, dx=dxr.abs().amax(-1) * kappa,
              dgamma=(dg0.double().abs() + sg).amax()[None], dbeta=(db0.double().abs() + sb).amax()[None])
    xg = x.to(DEV) if xdev is None else xdev
    gg, bg = gamma.to(DEV), beta.to(DEV)
    y, mean, rstd = ln_fwd_call(lib, xg, gg, bg, eps)
    check(f"{name} y", y, yr, LN_FWD_TOL, scale=sc["y"])
    check(f"{name} mean", mean[:, None], mr[:, None], LN_STAT_TOL, floor=1.0)
    check(f"{name} rstd", rstd[:, None], rr[:, None], LN_STAT_TOL)
    dg, db = dg0.to(DEV), db0.to(DEV)
    dx, _ = ln_bwd_call(lib, dy.to(DEV), xg, gg, mean, rstd, None if dres is None else dres.to(DEV), dg, db)
    check(f"{name} dx", dx, dxr, LN_DX_TOL, scale=sc["dx"])
    check(f"{name} dgamma", dg[None], (dg0.double() + dgr)[None], LN_DGB_TOL, scale=sc["dgamma"])
    check(f"{name} dbeta", db[None], (db0.double() + dbr)[None], LN_DGB_TOL, scale=sc["dbeta"])
    return (y, dx, dg, db), sc


LN_ROWS = [1, 9, 17, 23, 496, 497, 512]


@pytest.mark.parametrize("D", [64, 144, 256, 320, 512, 768, 1024])
def test_layernorm_vs_float64(ops, lib, D):
    """vector (D = 256 / 512) and generic forms; rows 17 / 23: odd pair tails in the 8-wave blocks; 496 / 497: the
    32-block switch from direct atomics to workspace + reduce; 7968 (config 2) and 65537 (the 4096-block cap: 17 rows per
    block); dgamma / dbeta start non-zero (the += contract on both paths); the residual gradient on and off"""
    big = {144: [7968], 256: [7968, 65537], 512: [7968], 64: [65537], 1024: [7968]}.get(D, [])
    for k, rows in enumerate(LN_ROWS + big):
        for eps in ((1e-12, 1e-5) if rows <= 512 else (1e-12,)):
            x, gamma, beta, dy, dres, dg0, db0 = ln_inputs(rows, D, D * 1000 + rows)
            ln_check_all(f"ln D={D} rows={rows} eps={eps:g}", lib, x, gamma, beta, dy, dres if k % 2 == 0 else None,
                         dg0, db0, eps)


@pytest.mark.parametrize("D", [256, 512])
def test_layernorm_misaligned_generic(ops, lib, D):
    """a view one float off a 16-byte boundary runs the generic forward and backward: same results as the vector forms
    to fp32 rounding, and float64 to the bound"""
    for rows in (17, 497):
        x, gamma, beta, dy, dres, dg0, db0 = ln_inputs(rows, D, 31 * D + rows)
        outa, sc = ln_check_all(f"ln aligned D={D} rows={rows}", lib, x, gamma, beta, dy, dres, dg0, db0, 1e-5)
        outm, _ = ln_check_all(f"ln misaligned D={D} rows={rows}", lib, x, gamma, beta, dy, dres, dg0, db0, 1e-5,
                               xdev=misaligned(x.to(DEV)))
        for name, a, m in zip(("y", "dx", "dgamma", "dbeta"), outa, outm):
            a, m = (a[None], m[None]) if a.dim() == 1 else (a, m)
            check(f"ln misaligned vs aligned D={D} rows={rows} {name}", m, a, LN_ROUND_TOL, scale=sc[name])


def test_layernorm_bf16_out_wide_and_refused(ops, lib):
    """bf16 output within one bf16 ulp of the fp32 output; D = 2048 forward (generic); D = 1025 backward is refused"""
    from espnet_amd._lib import EamdError
    for D, rows in ((64, 23), (256, 497), (320, 17), (512, 9)):
        x, gamma, beta, *_ = ln_inputs(rows, D, 5 * D + rows)
        xg, gg, bg = x.to(DEV), gamma.to(DEV), beta.to(DEV)
        y32, m32, r32 = ops.layernorm_fwd(xg, gg, bg, 1e-12)
        y16, m16, r16 = ops.layernorm_fwd(xg, gg, bg, 1e-12, out_dtype=torch.bfloat16)
        assert torch.equal(m16, m32) and torch.equal(r16, r32)
        _, e = torch.frexp(y32)
        ulp = torch.ldexp(torch.ones_like(y32), e - 8)              # |y| in [2^(e-1), 2^e): a bf16 ulp is 2^(e-8)
        d = (y16.float() - y32).abs()
        print(f"[rows] ln bf16 D={D}: max |y16 - y32| / ulp {float((d / ulp).max()):.3f}")
        assert (d <= ulp).all()
    x, gamma, beta, *_ = ln_inputs(40, 2048, 2048)
    yr, mr, rr, _, _, _, kappa, _, _ = ln_ref(x, gamma, beta, torch.zeros(40, 2048), 1e-12)
    y, mean, rstd = ln_fwd_call(lib, x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-12)
    check("ln D=2048 y", y, yr, LN_FWD_TOL, scale=yr.abs().amax(-1) * kappa)
    x, gamma, beta, dy, *_ = ln_inputs(5, 1025, 1025)
    xg = x.to(DEV)
    y, mean, rstd = ops.layernorm_fwd(xg, gamma.to(DEV), beta.to(DEV), 1e-12)
    with pytest.raises(EamdError):
        ops.layernorm_bwd(dy.to(DEV), xg, gamma.to(DEV), mean, rstd, None, torch.zeros(1025, device=DEV),
                          torch.zeros(1025, device=DEV))


@pytest.mark.parametrize("njobs", [1, 3, 130])
def test_layernorm_deferred_reduce(ops, lib, njobs):
    """partials left in workspaces (dgamma = dbeta = NULL), then ONE eamd_layernorm_bwd_reduce over njobs jobs (130: D in
    {144, 256, 512} and 1 .. 57 blocks, across the 64-job table boundary twice): every job equals its own immediate
    reduction to fp32 rounding and float64 to the bound"""
    Ds = (144, 256, 512)
    rowss = (1, 17, 100, 497, 900)
    jobs, keep = [], []
    for j in range(njobs):
        D, rows = Ds[j % 3], rowss[(j // 3 + j) % 5]
        x, gamma, beta, dy, dres, dg0, db0 = ln_inputs(rows, D, 7000 + j)
        xg, gg, bg, dyg = x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)
        y, mean, rstd = ln_fwd_call(lib, xg, gg, bg, 1e-12)
        dgi, dbi = dg0.to(DEV), db0.to(DEV)
        dxi, _ = ln_bwd_call(lib, dyg, xg, gg, mean, rstd, None, dgi, dbi)
        dgd, dbd = dg0.to(DEV), db0.to(DEV)
        dxd, ws = ln_bwd_call(lib, dyg, xg, gg, mean, rstd, None, None, None, deferred=True)   # dgd / dbd untouched
        assert torch.equal(dxd, dxi)
        _, _, _, _, dgr, dbr, _, sg, sb = ln_ref(x, gamma, beta, dy, 1e-12)
        jobs.append((ws, dgd, dbd, ws.numel() // (2 * D), D))
        keep.append((dgi, dbi, dg0.double() + dgr, db0.double() + dbr, (dg0.double().abs() + sg).amax()[None],
                     (db0.double().abs() + sb).amax()[None]))
    tab = (ops._LnReduceJob * njobs)()
    for i, (ws, dg, db, nblk, D) in enumerate(jobs):
        tab[i].ws, tab[i].dgamma, tab[i].dbeta, tab[i].nblk, tab[i].D = ws.data_ptr(), dg.data_ptr(), db.data_ptr(), nblk, D
    lib.check(lib.lib().eamd_layernorm_bwd_reduce(tab, njobs, lib.stream_ptr()), "eamd_layernorm_bwd_reduce")
    torch.cuda.synchronize()
    print(f"[rows] ln deferred reduce: {njobs} jobs, blocks per job {sorted({j[3] for j in jobs})}")
    e_round = e_ref = 0.0
    for j, ((ws, dg, db, nblk, D), (dgi, dbi, dgr, dbr, sg, sb)) in enumerate(zip(jobs, keep)):
        for name, got, imm, ref, sc in (("dgamma", dg, dgi, dgr, sg), ("dbeta", db, dbi, dbr, sb)):
            er, _ = row_err(got[None], imm[None], scale=sc)
            ef, _ = row_err(got[None], ref[None], scale=sc)
            assert er <= LN_ROUND_TOL, f"job {j} (D={D}, {nblk} blocks) {name}: deferred vs immediate {er:.3e}"
            assert ef <= LN_DGB_TOL, f"job {j} (D={D}, {nblk} blocks) {name}: vs float64 {ef:.3e}"
            e_round, e_ref = max(e_round, er), max(e_ref, ef)
    print(f"[rows] ln deferred reduce: vs immediate {e_round:.3e} (tol {LN_ROUND_TOL:g}), vs float64 {e_ref:.3e} "
          f"(tol {LN_DGB_TOL:g})")


# ---------------------------------------------------------------------------------------------
# reduce_sum
# ---------------------------------------------------------------------------------------------
REDUCE_SUM_TOL = 1.8e-7  # |sum - ref| relative to scale * sum |x|; observed 4.6e-8


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 10 ** 7])
def test_reduce_sum_vs_float64(ops, lib, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) + 0.25
    xd = x.to(DEV)
    scale = -0.37
    outs = []
    for _ in range(2):
        out = torch.full((), NAN, device=DEV)
        lib.check(lib.lib().eamd_reduce_sum(lib.ptr(xd), C.c_int64(n), lib.ptr(out), C.c_float(scale), lib.stream_ptr()),
                  "eamd_reduce_sum")
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "two runs on the same input differ"
    assert torch.equal(ops.reduce_sum(xd, scale), outs[0])
    ref = scale * x.double().sum()
    e = abs(float(outs[0]) - float(ref)) / max(abs(scale) * float(x.double().abs().sum()), 1e-30)
    if n == 0:      # caught: eamd_reduce_sum refused the NULL data pointer of an empty tensor (EamdError)
        assert float(outs[0]) == 0.0
    print(f"[rows] reduce_sum n={n}: err / (|scale| sum|x|) {e:.3e} (tol {REDUCE_SUM_TOL:g})")
    assert e <= REDUCE_SUM_TOL
