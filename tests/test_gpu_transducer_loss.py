"""The transducer (RNN-T) loss and joint kernels against float64 on every dispatch path: eamd_rnnt_loss / eamd_rnnt_grad
(log-sum-exp gather: wave form, V > 6144 and misaligned block form; alpha / beta diagonals longer than the 256 threads of
a workgroup, up to the 64 KiB LDS limit; scalar and float4 gradient loops), the streamed lattice-row entry points
(eamd_rnnt_node_stats / _node_stats_part / _row_coef / _alpha_beta / _node_grad), GEMM epilogues 7 (row statistics) and
8 (softmax-gradient rows) in the fp32 and bf16 operand kernels, eamd_joint_fwd / eamd_joint_bwd (one-slice and sliced
atomic forms) and JointRNNTLossFn end to end.

Every comparison is element-wise, per lattice node, per utterance or per output row (row_err / check of
test_gpu_row_kernels), never a whole-tensor norm.  Integer outputs match exactly; what the kernels must define outside an
utterance's lattice is exactly 0 or exactly -inf; outputs are NaN-filled before the launch.  Each bound is at most 4x the
error seen on an MI355X, noted beside it.

The float64 reference (lattice_ref) runs alpha / beta along anti-diagonals; test_lattice_ref_vs_oracle checks it against
oracle.rnnt_loss (itself checked by brute force in test_oracle_golden.py) and its autograd without a GPU."""
import ctypes as C
import math

import pytest
import torch

from test_gpu_row_kernels import check, misaligned

gpu = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
INF = float("inf")
EPS = 2.0 ** -24          # fp32 unit roundoff
EUNSUPPORTED = -2


# ---------------------------------------------------------------------------------------------
# float64 lattice reference
# ---------------------------------------------------------------------------------------------
def lattice_ref(z, labels, tlens, ulens, blank, sc=1.0):
    """float64 transducer loss of raw logits z [B,T,U,V] (labels [B,U-1], padded with anything in [0, V)):
    per node lse, lpb = log p(blank), lpl = log p(next label) (-inf in the last column U-1), alpha / beta (-inf outside
    each utterance's Tb x Ub lattice), loss[b] (+inf for invalid lengths), the occupancy gamma = exp(alpha + beta - logZ),
    the blank / label transition posteriors gb / gl, tot = log gamma - lse, the gradient
    sc * (gamma * softmax - [v = blank] gb - [v = label] gl) and the per-node magnitude
    S = |alpha| + |beta| + |logZ| + |lse| + max|z| that bounds fp32's error in the exponent, with walk = sqrt(Tb + Ub - 1):
    alpha and beta gather their rounding errors along a path of Tb + Ub - 1 steps, and they add up like a random walk."""
    zd = z.detach().double().cpu()
    B, T, U, V = zd.shape
    ninf = torch.tensor(-INF, dtype=torch.float64)
    lse = torch.logsumexp(zd, -1)
    lp = zd - lse[..., None]
    lab = labels.detach().long().cpu().reshape(B, max(U - 1, 0))
    lpb = lp[..., blank].clone()
    lpl = torch.full((B, T, U), -INF, dtype=torch.float64)
    labu = torch.full((B, T, U), blank, dtype=torch.long)          # next label of node (t, u); blank where there is none
    if U > 1:
        labu[:, :, :U - 1] = lab[:, None, :]
        lpl[:, :, :U - 1] = lp[:, :, :U - 1].gather(3, labu[:, :, :U - 1, None]).squeeze(3)
    alpha = torch.full((B, T, U), -INF, dtype=torch.float64)
    beta = torch.full((B, T, U), -INF, dtype=torch.float64)
    gam = torch.zeros(B, T, U, dtype=torch.float64)
    gb = torch.zeros(B, T, U, dtype=torch.float64)
    gl = torch.zeros(B, T, U, dtype=torch.float64)
    loss = torch.full((B,), INF, dtype=torch.float64)
    logz = torch.full((B,), -INF, dtype=torch.float64)
    walk = torch.ones(B, T, U, dtype=torch.float64)
    for b in range(B):
        Tb, Ub = int(tlens[b]), int(ulens[b]) + 1
        if not (0 < Tb <= T and 0 < Ub <= U):
            continue
        walk[b] = math.sqrt(Tb + Ub - 1)
        pb, pl = lpb[b, :Tb, :Ub], lpl[b, :Tb, :Ub]
        a = torch.full((Tb, Ub), -INF, dtype=torch.float64)
        be = torch.full((Tb, Ub), -INF, dtype=torch.float64)
        a[0, 0] = 0.0
        for dg in range(1, Tb + Ub - 1):
            u = torch.arange(max(0, dg - Tb + 1), min(dg, Ub - 1) + 1)
            t = dg - u
            tm, um = (t - 1).clamp_min(0), (u - 1).clamp_min(0)
            a[t, u] = torch.logaddexp(torch.where(t > 0, a[tm, u] + pb[tm, u], ninf),
                                      torch.where(u > 0, a[t, um] + pl[t, um], ninf))
        be[Tb - 1, Ub - 1] = pb[Tb - 1, Ub - 1]
        for dg in range(Tb + Ub - 3, -1, -1):
            u = torch.arange(max(0, dg - Tb + 1), min(dg, Ub - 1) + 1)
            t = dg - u
            tp, up = (t + 1).clamp_max(Tb - 1), (u + 1).clamp_max(Ub - 1)
            be[t, u] = torch.logaddexp(torch.where(t < Tb - 1, be[tp, u] + pb[t, u], ninf),
                                       torch.where(u < Ub - 1, be[t, up] + pl[t, u], ninf))
        lz = be[0, 0]
        logz[b], loss[b] = lz, -lz
        alpha[b, :Tb, :Ub], beta[b, :Tb, :Ub] = a, be
        gam[b, :Tb, :Ub] = (a + be - lz).exp()
        gb[b, :Tb - 1, :Ub] = (a[:-1] + pb[:-1] + be[1:] - lz).exp()
        gb[b, Tb - 1, Ub - 1] = (a[-1, -1] + pb[-1, -1] - lz).exp()
        gl[b, :Tb, :Ub - 1] = (a[:, :-1] + pl[:, :-1] + be[:, 1:] - lz).exp()
    grad = gam[..., None] * lp.exp()
    grad[..., blank] -= gb
    grad.scatter_add_(3, labu[..., None], -gl[..., None])
    grad *= sc
    inside = torch.isfinite(alpha) & torch.isfinite(beta)
    fin = lambda x: x.abs().where(inside, torch.zeros((), dtype=torch.float64))       # noqa: E731
    S = fin(alpha) + fin(beta) + fin(logz[:, None, None].expand(B, T, U)) + lse.abs() + zd.abs().amax(-1)
    tot = (alpha + beta - logz[:, None, None] - lse).where(inside, ninf)
    return dict(lse=lse, lpb=lpb, lpl=lpl, alpha=alpha, beta=beta, loss=loss, logz=logz, gamma=gam, gb=gb, gl=gl,
                grad=grad, S=S, walk=walk, tot=tot, labu=labu, inside=inside,
                zmax=zd.abs().amax(-1))


def test_lattice_ref_vs_oracle(oracle):
    """the float64 reference against oracle.rnnt_loss and its autograd on ragged batches (U = 1, T = 1 included)"""
    g = torch.Generator().manual_seed(11)
    for B, T, U, V, tl, ul, blank in ((3, 6, 4, 7, [6, 4, 1], [3, 1, 2], 0), (2, 1, 5, 5, [1, 1], [4, 0], 4),
                                      (2, 5, 1, 3, [5, 2], [0, 0], 0), (3, 9, 7, 6, [9, 9, 3], [6, 4, 0], 2)):
        z = torch.randn(B, T, U, V, generator=g, dtype=torch.float64) * 2.0
        lab = torch.randint(0, V, (B, max(U - 1, 1)), generator=g)[:, :U - 1]
        lab[lab == blank] = (blank + 1) % V
        ref = lattice_ref(z, lab, tl, ul, blank, sc=1.0)
        zr = z.clone().requires_grad_(True)
        want = oracle.rnnt_loss(zr, lab, tl, ul, blank=blank, reduction="none")
        want.sum().backward()
        assert torch.allclose(ref["loss"], want.detach(), rtol=1e-12, atol=0), (ref["loss"], want)
        d = (ref["grad"] - zr.grad).abs().max().item()
        assert d < 1e-12, d
        for b in range(B):                        # the occupancy of one anti-diagonal sums to 1
            occ = ref["gamma"][b]
            for dg in range(tl[b] + ul[b]):
                s = sum(float(occ[t, dg - t]) for t in range(tl[b]) if 0 <= dg - t <= ul[b])
                assert abs(s - 1.0) < 1e-12, (b, dg, s)


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    from espnet_amd import ops as o
    o.set_precision("fp32")
    yield o
    o.set_precision("fp32")


@pytest.fixture(scope="module")
def lib():
    from espnet_amd import _lib
    return _lib


def ptr(t):
    from espnet_amd import _lib
    return _lib.ptr(t)


def stream():
    from espnet_amd import _lib
    return _lib.stream_ptr()


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def labels_dev(lab, U):
    """labels [B, U-1] int32 on the device; one dummy element when U = 1 (the ABI wants a pointer)"""
    lab = lab.to(torch.int32)
    return (lab if U > 1 else torch.zeros(1, dtype=torch.int32)).contiguous().to(DEV)


def rnnt_loss_call(lib, z, lab, tl, ul, blank, grad=True, gscale=None, scale=1.0):
    """eamd_rnnt_loss with NaN-filled workspace / loss / gradient -> (rc, loss, ws [5, B,T,U], grad or None)"""
    B, T, U, V = z.shape
    ws = torch.full((5 * B * T * U,), NAN, device=DEV)
    loss = torch.full((B,), NAN, device=DEV)
    if grad is True:
        grad = torch.full_like(z, NAN)
    elif grad is False:
        grad = None
    rc = lib.lib().eamd_rnnt_loss(ptr(z), ptr(lab), ptr(tl), ptr(ul), ptr(ws), ptr(loss), ptr(grad), B, T, U, V, blank,
                                  ptr(gscale), C.c_float(scale), stream())
    torch.cuda.synchronize()
    return rc, loss, ws.view(5, B, T, U), grad


def rnnt_grad_call(lib, z, lab, tl, ul, blank, ws, gscale=None, scale=1.0, grad=None):
    B, T, U, V = z.shape
    grad = torch.full_like(z, NAN) if grad is None else grad
    lib.check(lib.lib().eamd_rnnt_grad(ptr(z), ptr(lab), ptr(tl), ptr(ul), ptr(ws), ptr(grad), B, T, U, V, blank,
                                       ptr(gscale), C.c_float(scale), stream()), "eamd_rnnt_grad")
    return grad


def f64(x):
    return x.detach().double().cpu()


# Bounds.  Node statistics: |err| / (|lse| + max|z|) per node.  alpha / beta: |err| / (max|alpha or beta| + (Tb + Ub) *
# max(|lse| + max|z|)) per utterance.  Gradient rows and (gb, gl): |err| / (gamma |sc| S walk) with S and walk of
# lattice_ref, i.e. (constant) x 2^-24 x (|alpha| + |beta| + |logZ| + |lse| + max|z|) x sqrt(Tb + Ub - 1).
STATS_TOL = 8e-7          # lse / lpb / lpl; observed 2.1e-7 (U255 lpl)
AB_TOL = 9e-7             # alpha / beta per utterance; observed 2.4e-7 (U8192 beta)
LOSS_TOL = 3e-7           # loss[b] relative to (Tb + Ub) * max(|lse| + max|z|) + |loss|; observed 7.8e-8 (U8192)
GRAD_K = 1.9              # gradient rows in units of 2^-24 * gamma * |sc| * S * walk; observed 0.50 (peaked)
GAMMA_FLOOR = 1e-30       # gamma below this is compared in absolute terms


def check_stats(name, stats, ref, tol=STATS_TOL, extra=0.0):
    """lse, lpb, lpl per node against the float64 reference (lpl = -inf exactly in the last column), relative to
    |lse| + max|z| (+ extra: the size of the GEMM terms where the logits are recomputed)"""
    s = (ref["lse"].abs() + ref["zmax"]).reshape(-1) + extra
    e = 0.0
    for nm, got, want in zip(("lse", "lpb", "lpl"), stats, (ref["lse"], ref["lpb"], ref["lpl"])):
        e = max(e, check(f"{name} {nm}", got.reshape(-1, 1), want.reshape(-1, 1), tol, scale=s))
    return e


def check_alpha_beta(name, alpha, beta, ref, tl, ul, tol=AB_TOL):
    """alpha / beta of each utterance relative to its largest |alpha| (|beta|) plus (Tb + Ub) steps of max(|lse| + max|z|);
    exactly -inf outside the lattice.  Returns the step term per utterance."""
    B = alpha.shape[0]
    step = (ref["lse"].abs() + ref["zmax"]).reshape(B, -1).amax(-1)
    nstep = torch.tensor([max(1, int(t) + int(u) + 1) for t, u in zip(tl, ul)], dtype=torch.float64) * step
    for nm, got, want in (("alpha", alpha, ref["alpha"]), ("beta", beta, ref["beta"])):
        mag = torch.where(torch.isfinite(want), want.abs(), torch.zeros((), dtype=torch.float64)).reshape(B, -1).amax(-1)
        check(f"{name} {nm}", got.reshape(B, -1), want.reshape(B, -1), tol, scale=mag + nstep)
    return nstep


def check_loss(name, loss, ref, nstep, tol=LOSS_TOL):
    want = ref["loss"]
    fin = torch.isfinite(want)
    assert torch.equal(f64(loss)[~fin], want[~fin]), f"{name}: invalid utterances must give +inf"
    return check(f"{name} loss", loss.reshape(-1, 1), want.reshape(-1, 1), tol,
                 scale=nstep + want.abs().where(fin, torch.zeros(()).double()))


def check_grad(name, grad, ref, sc, k=GRAD_K):
    """gradient rows relative to gamma |sc| S walk; nodes with gamma = 0 must be exactly 0"""
    V = grad.shape[-1]
    gam = ref["gamma"].reshape(-1)
    zero = gam == 0
    g = f64(grad).reshape(-1, V)
    assert torch.equal(g[zero], torch.zeros_like(g[zero])), f"{name}: rows with zero occupancy must be exactly 0"
    s = gam.clamp_min(GAMMA_FLOOR) * abs(sc) * (ref["S"] * ref["walk"]).reshape(-1) * EPS
    return check(f"{name} grad", g, ref["grad"].reshape(-1, V), k, scale=s)


def make_case(seed, B, T, U, V, tl, ul, blank=0, zscale=2.0, pad="blank"):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, T, U, V, generator=g) * zscale
    lab = torch.randint(0, V, (B, max(U - 1, 1)), generator=g)[:, :U - 1]
    lab[lab == blank] = (blank + 1) % V
    for b in range(B):
        u = max(0, min(int(ul[b]), U - 1))
        if pad == "blank":
            lab[b, u:] = blank
    return z, lab


def run_loss_case(lib, name, z, lab, tl, ul, blank, gscale=None, scale=1.0, zdev=None, k=GRAD_K):
    B, T, U, V = z.shape
    zd = z.to(DEV) if zdev is None else zdev
    labd = labels_dev(lab, U)
    gs = None if gscale is None else torch.tensor([gscale], device=DEV)
    rc, loss, ws, grad = rnnt_loss_call(lib, zd, labd, i32(tl), i32(ul), blank, gscale=gs, scale=scale)
    lib.check(rc, "eamd_rnnt_loss")
    sc = scale * (1.0 if gscale is None else gscale)
    ref = lattice_ref(z, lab, tl, ul, blank, sc=sc)
    check_stats(name, (ws[0], ws[1], ws[2]), ref)
    nstep = check_alpha_beta(name, ws[3], ws[4], ref, tl, ul)
    check_loss(name, loss, ref, nstep)
    check_grad(name, grad, ref, sc, k)
    return loss, ws, grad, ref


# ---------------------------------------------------------------------------------------------
# 2. materialised loss: eamd_rnnt_loss, eamd_rnnt_grad
# ---------------------------------------------------------------------------------------------
# (B, T, U, V, tlens, ulens, blank, logit scale)
V_CASES = {
    "V2": (2, 5, 4, 2, [5, 3], [3, 2], 0, 2.0),
    "V4": (2, 5, 4, 4, [5, 4], [3, 1], 0, 2.0),
    "V5-blankV-1": (2, 6, 3, 5, [6, 2], [2, 2], 4, 2.0),
    "V33": (3, 7, 5, 33, [7, 5, 1], [4, 0, 3], 0, 2.0),
    "V4999": (2, 4, 3, 4999, [4, 3], [2, 1], 0, 2.0),
    "V5000": (2, 4, 3, 5000, [4, 3], [2, 1], 0, 2.0),
    "V5000-blankV-1": (2, 4, 3, 5000, [4, 2], [2, 2], 4999, 2.0),
    "V6144": (2, 4, 3, 6144, [4, 3], [2, 1], 0, 2.0),
    "V6148": (2, 4, 3, 6148, [4, 3], [2, 1], 0, 2.0),
    "V10000": (2, 4, 3, 10000, [4, 2], [2, 1], 0, 2.0),
}


@gpu
@pytest.mark.parametrize("case", list(V_CASES))
def test_rnnt_loss_vocab(lib, case):
    B, T, U, V, tl, ul, blank, zs = V_CASES[case]
    z, lab = make_case(len(case) * 7 + V, B, T, U, V, tl, ul, blank, zs)
    run_loss_case(lib, case, z, lab, tl, ul, blank)


@gpu
def test_rnnt_loss_misaligned_logits(lib):
    """logits one float past a 16-byte boundary at V = 5000: block gather and scalar gradient loop; on the same workspace
    the aligned float4 loop gives the same gradient bit for bit (same arithmetic per element)"""
    B, T, U, V, tl, ul = 2, 4, 3, 5000, [4, 3], [2, 1]
    z, lab = make_case(5, B, T, U, V, tl, ul)
    zm = misaligned(z.to(DEV))
    _, ws_m, g_m, _ = run_loss_case(lib, "misaligned", z, lab, tl, ul, 0, zdev=zm)
    g_a = rnnt_grad_call(lib, z.to(DEV), labels_dev(lab, U), i32(tl), i32(ul), 0, ws_m)     # same workspace, float4 loop
    assert torch.equal(g_m, g_a), "scalar and float4 gradient loops differ"


# (B, T, U, V, tlens, ulens, blank, logit scale): diagonals longer than one pass of 256 threads need Tb, Ub > 256
U_CASES = {
    "U1": (2, 7, 1, 6, [7, 3], [0, 0], 0, 2.0),
    "U255": (1, 258, 255, 3, [258], [254], 0, 1.0),
    "U256": (1, 258, 256, 3, [258], [255], 0, 1.0),
    "U257": (2, 260, 257, 3, [260, 259], [256, 200], 0, 1.0),
    "U1000": (1, 300, 1000, 4, [300], [999], 0, 1.0),
    "U8192": (1, 3, 8192, 3, [3], [8191], 0, 1.0),
    "T1500": (1, 1500, 30, 8, [1500], [29], 0, 8.0),
    "peaked": (2, 40, 12, 33, [40, 31], [11, 7], 0, 30.0),
    "flat": (2, 40, 12, 33, [40, 31], [11, 7], 0, 0.01),
    "lengths": (5, 9, 6, 7, [9, 6, 1, 9, 2], [5, 2, 0, 0, 5], 0, 2.0),
}


@gpu
@pytest.mark.parametrize("case", list(U_CASES))
def test_rnnt_loss_lattice_shapes(lib, case):
    B, T, U, V, tl, ul, blank, zs = U_CASES[case]
    z, lab = make_case(len(case) * 13 + U, B, T, U, V, tl, ul, blank, zs)
    run_loss_case(lib, case, z, lab, tl, ul, blank)


@gpu
def test_rnnt_lds_limit_rejected(lib):
    """U = 8193 needs more than 64 KiB of LDS for two diagonals: refused before any launch, outputs untouched"""
    B, T, U, V = 1, 1, 8193, 2
    z = torch.zeros(B, T, U, V, device=DEV)
    lab = torch.ones(B, U - 1, dtype=torch.int32, device=DEV)
    tl, ul = i32([1]), i32([U - 1])
    rc, loss, ws, grad = rnnt_loss_call(lib, z, lab, tl, ul, 0)
    assert rc == EUNSUPPORTED
    assert torch.isnan(loss).all() and torch.isnan(ws).all() and torch.isnan(grad).all()
    ws = torch.full((5 * B * T * U,), NAN, device=DEV)
    loss = torch.full((B,), NAN, device=DEV)
    rc = lib.lib().eamd_rnnt_alpha_beta(ptr(ws), ptr(tl), ptr(ul), ptr(loss), B, T, U, stream())
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED
    assert torch.isnan(loss).all() and torch.isnan(ws).all()


@gpu
def test_rnnt_invalid_lengths(lib):
    """tlens = 0, tlens = T + 1, ulens = U, ulens = -1: loss = +inf exactly, alpha / beta all -inf, zero gradient rows;
    the other utterances bit-identical to a run where every length is valid"""
    B, T, U, V = 6, 7, 5, 9
    tl_bad, ul_bad = [7, 0, 8, 5, 6, 3], [4, 2, 2, 5, -1, 1]
    tl_ok, ul_ok = [7, 4, 7, 5, 6, 3], [4, 2, 2, 4, 1, 1]
    z, lab = make_case(17, B, T, U, V, tl_ok, ul_ok)
    zd, labd = z.to(DEV), labels_dev(lab, U)
    rc, loss, ws, grad = rnnt_loss_call(lib, zd, labd, i32(tl_bad), i32(ul_bad), 0)
    lib.check(rc, "eamd_rnnt_loss")
    rc, loss0, ws0, grad0 = rnnt_loss_call(lib, zd, labd, i32(tl_ok), i32(ul_ok), 0)
    lib.check(rc, "eamd_rnnt_loss")
    bad = [1, 2, 3, 4]
    for b in range(B):
        if b in bad:
            assert float(loss[b]) == INF, (b, float(loss[b]))
            assert bool((ws[3:, b] == -INF).all()), b
            assert bool((grad[b] == 0).all()), b
        else:
            assert torch.equal(loss[b], loss0[b]) and torch.equal(ws[:, b], ws0[:, b]) and torch.equal(grad[b], grad0[b]), b
    # the valid utterances also against float64
    ref = lattice_ref(z, lab, tl_bad, ul_bad, 0)
    nstep = check_alpha_beta("invalid lengths", ws[3], ws[4], ref, [max(0, t) for t in tl_bad], [max(0, u) for u in ul_bad])
    check_loss("invalid lengths", loss, ref, nstep)
    check_grad("invalid lengths", grad, ref, 1.0)


@gpu
def test_rnnt_label_padding_is_ignored(lib):
    """labels past ulens[b] set to random valid ids give results bit-identical to blank padding"""
    B, T, U, V, tl, ul = 3, 8, 7, 13, [8, 6, 3], [6, 3, 0]
    z, lab = make_case(23, B, T, U, V, tl, ul)
    g = torch.Generator().manual_seed(24)
    lab_r = lab.clone()
    for b in range(B):
        lab_r[b, ul[b]:] = torch.randint(1, V, (U - 1 - ul[b],), generator=g)
    assert not torch.equal(lab_r, lab)
    zd = z.to(DEV)
    res = []
    for lb in (lab, lab_r):
        rc, loss, ws, grad = rnnt_loss_call(lib, zd, labels_dev(lb, U), i32(tl), i32(ul), 0)
        lib.check(rc, "eamd_rnnt_loss")
        res.append((loss, ws, grad))
    (l0, w0, g0), (l1, w1, g1) = res
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert torch.equal(w0[[0, 1, 3, 4]], w1[[0, 1, 3, 4]])                 # lse, lpb, alpha, beta
    for b in range(B):                                                    # lpl inside the lattice
        assert torch.equal(w0[2, b, :, :ul[b]], w1[2, b, :, :ul[b]])


@gpu
@pytest.mark.parametrize("gscale", [0.37, -2.0])
def test_rnnt_upstream_scale(lib, gscale):
    """gscale_dev (the upstream gradient, read on the device) and scale = 1/B are both folded into the gradient, by
    eamd_rnnt_loss(grad=...) and by eamd_rnnt_grad"""
    B, T, U, V, tl, ul = 3, 9, 6, 40, [9, 7, 4], [5, 5, 2]
    z, lab = make_case(31, B, T, U, V, tl, ul)
    _, ws, grad, _ = run_loss_case(lib, "gscale %g" % gscale, z, lab, tl, ul, 0, gscale=gscale, scale=1.0 / B)
    g2 = rnnt_grad_call(lib, z.to(DEV), labels_dev(lab, U), i32(tl), i32(ul), 0, ws, torch.tensor([gscale], device=DEV), 1.0 / B)
    assert torch.equal(grad, g2)
    sc = gscale / B
    check_grad("gscale %g via eamd_rnnt_grad" % gscale, g2, lattice_ref(z, lab, tl, ul, 0, sc=sc), sc)


@gpu
@pytest.mark.parametrize("V", [5000, 777])
def test_rnnt_gradient_aliasing(lib, V):
    """the gradient written over the logits equals the gradient in a separate buffer; eamd_rnnt_loss(grad=...) equals a
    later eamd_rnnt_grad (bit for bit; float4 loop at V = 5000, scalar loop at V = 777)"""
    B, T, U, tl, ul = 2, 5, 4, [5, 3], [3, 2]
    z, lab = make_case(37 + V, B, T, U, V, tl, ul)
    zd, labd, tld, uld = z.to(DEV), labels_dev(lab, U), i32(tl), i32(ul)
    gs = torch.tensor([0.37], device=DEV)
    rc, loss, ws, g_sep = rnnt_loss_call(lib, zd, labd, tld, uld, 0, gscale=gs, scale=0.5)
    lib.check(rc, "eamd_rnnt_loss")
    rc, loss2, ws2, _ = rnnt_loss_call(lib, zd, labd, tld, uld, 0, grad=False)
    lib.check(rc, "eamd_rnnt_loss")
    assert torch.equal(loss, loss2) and torch.equal(ws, ws2)
    g_later = rnnt_grad_call(lib, zd, labd, tld, uld, 0, ws2, gs, 0.5)
    assert torch.equal(g_sep, g_later)
    zin = zd.clone()
    rc, loss3, _, g_in = rnnt_loss_call(lib, zin, labd, tld, uld, 0, grad=zin, gscale=gs, scale=0.5)
    lib.check(rc, "eamd_rnnt_loss")
    assert g_in.data_ptr() == zin.data_ptr() and torch.equal(g_in, g_sep) and torch.equal(loss3, loss)
    zin = zd.clone()
    rnnt_grad_call(lib, zin, labd, tld, uld, 0, ws2, gs, 0.5, grad=zin)
    assert torch.equal(zin, g_sep)


# ---------------------------------------------------------------------------------------------
# 3. streamed lattice rows
# ---------------------------------------------------------------------------------------------
def chunkings(n, U):
    return {"1": [1] * n, "7": [7] * (n // 7) + ([n % 7] if n % 7 else []),
            "13": [13] * (n // 13) + ([n % 13] if n % 13 else []), "whole": [n]}


@gpu
@pytest.mark.parametrize("V", [5000, 12])
def test_rnnt_node_entry_points_match_materialised(lib, V):
    """eamd_rnnt_node_stats over chunks of 1, 7, 13 rows and the whole lattice fills the first 3n workspace floats of
    one eamd_rnnt_loss call bit for bit (V % 4 == 0 keeps every chunk 16-byte aligned: the wave form at V = 5000);
    eamd_rnnt_alpha_beta on it then matches too; eamd_rnnt_node_grad over the same chunks equals eamd_rnnt_grad; its bf16
    output is RNE of its fp32 output, through the float4 path (aligned) and the scalar path (misaligned rows)"""
    B, T, U, tl, ul = 2, 6, 5, [6, 4], [4, 2]
    n = B * T * U
    z, lab = make_case(41 + V, B, T, U, V, tl, ul)
    zd, labd, tld, uld = z.to(DEV), labels_dev(lab, U), i32(tl), i32(ul)
    gs = torch.tensor([-0.37], device=DEV)
    rc, loss_m, ws_m, g_m = rnnt_loss_call(lib, zd, labd, tld, uld, 0, gscale=gs, scale=0.5)
    lib.check(rc, "eamd_rnnt_loss")
    zr = zd.view(n, V)
    L = lib.lib()
    for cname, sizes in chunkings(n, U).items():
        ws = torch.full((5 * n,), NAN, device=DEV)
        node0 = 0
        for s in sizes:
            lib.check(L.eamd_rnnt_node_stats(ptr(zr[node0:node0 + s]), ptr(labd), ptr(ws), C.c_int64(node0), C.c_int64(s),
                                             B, T, U, V, 0, stream()), "eamd_rnnt_node_stats")
            node0 += s
        assert torch.equal(ws[:3 * n], ws_m.reshape(-1)[:3 * n]), cname
        loss = torch.full((B,), NAN, device=DEV)
        lib.check(L.eamd_rnnt_alpha_beta(ptr(ws), ptr(tld), ptr(uld), ptr(loss), B, T, U, stream()), "eamd_rnnt_alpha_beta")
        assert torch.equal(ws, ws_m.reshape(-1)) and torch.equal(loss, loss_m), cname
        for mis in (False, True):
            g32 = torch.full((n, V), NAN, device=DEV)
            g16 = torch.full((n, V), NAN, device=DEV).to(torch.bfloat16)
            src = misaligned(zr) if mis else zr
            node0 = 0
            for s in sizes:
                lib.check(L.eamd_rnnt_node_grad(ptr(src[node0:node0 + s]), ptr(g32[node0:node0 + s]), None, ptr(labd),
                                                ptr(tld), ptr(uld), ptr(ws), C.c_int64(node0), C.c_int64(s), B, T, U, V, 0,
                                                ptr(gs), C.c_float(0.5), stream()), "eamd_rnnt_node_grad")
                lib.check(L.eamd_rnnt_node_grad(ptr(src[node0:node0 + s]), None, ptr(g16[node0:node0 + s]), ptr(labd),
                                                ptr(tld), ptr(uld), ptr(ws), C.c_int64(node0), C.c_int64(s), B, T, U, V, 0,
                                                ptr(gs), C.c_float(0.5), stream()), "eamd_rnnt_node_grad bf16")
                node0 += s
            assert torch.equal(g32, g_m.view(n, V)), (cname, mis)
            assert torch.equal(g16.view(torch.int16), g32.to(torch.bfloat16).view(torch.int16)), (cname, mis)
            if cname != "whole":
                break          # the misaligned form once, on the whole lattice


def joint_operands(seed, B, T, U, J, V, bf16, wscale=0.2):
    """joint activations H [B*T*U, J], W [V, J], b [V] (bf16 operands rounded on the host, so float64 sees them too)"""
    g = torch.Generator().manual_seed(seed)
    H = torch.tanh(torch.randn(B * T * U, J, generator=g))
    W = torch.randn(V, J, generator=g) * wscale
    bias = torch.randn(V, generator=g)
    if bf16:
        H, W = H.to(torch.bfloat16), W.to(torch.bfloat16)
    z = (H.double() @ W.double().t() + bias.double()).view(B, T, U, V)
    zmag = H.double().abs() @ W.double().abs().t() + bias.double().abs()       # size of the terms of each logit
    return H, W, bias, z, zmag


STATS_GEMM_TOL = 4.4e-7   # lse / lpb / lpl from epilogue 7 + eamd_rnnt_node_stats_part, scale + max_v sum |h w| + |b|; observed 1.1e-7 (fp32 t64 V2 lpb)
ZCOL_TOL = 6.2e-7         # the gathered logits zcol / zfix relative to sum_j |h_j w_vj| + |b_v|; observed 1.6e-7 (fp32 t128 V63 zfix)


@gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("V", [2, 63, 777, 4999, 5000])
def test_rnnt_stats_epilogue(lib, ops, prec, tile, V):
    """EPI_ROW_STATS (fp32 operands on the pipelined fp32 kernel, bf16 operands on the bf16 kernel) then
    eamd_rnnt_node_stats_part: nrows not a multiple of the tile, blank in the last (partial) column tile, rows with
    col = -1; lse, lpb, lpl per node against float64 of the same operands; zcol of col = -1 rows is not written"""
    bf16 = prec == "bf16"
    B, T, U, J = 2, 13, 9, 64
    n = B * T * U
    blank = V - 1
    tl, ul = [13, 9], [8, 5]
    H, W, bias, z, zmag = joint_operands(V * 10 + tile, B, T, U, J, V, bf16)
    g = torch.Generator().manual_seed(V)
    lab = torch.randint(0, V - 1, (B, U - 1), generator=g)
    ref = lattice_ref(z, lab, tl, ul, blank)
    labu = torch.cat([lab, torch.full((B, 1), -1)], 1)[:, None, :].expand(B, T, U).reshape(-1).to(torch.int32)
    Hd, Wd, bd = H.to(DEV), W.to(DEV), bias.to(DEV)
    ops.set_precision("fp32")
    ws = torch.full((5 * n,), NAN, device=DEV)
    tn = (V + tile - 1) // tile
    node0 = 0
    for s in (n - 150, 150):            # 150 rows: 2 full tiles + 22 at tile 64, 1 + 22 at tile 128
        part = torch.full((s * tn * 2,), NAN, device=DEV)
        zcol = torch.full((s,), NAN, device=DEV)
        zfix = torch.full((s,), NAN, device=DEV)
        col = labu[node0:node0 + s].to(DEV)
        ops.gemm(Hd[node0:node0 + s], Wd, None, s, V, J, J, J, V, bias=bd, epilogue=ops.EPI_ROW_STATS, tile=tile,
                 stats=(part, col, zcol, zfix, blank), precision=0)
        none = (col < 0).cpu()
        assert bool(torch.isnan(zcol.cpu()[none]).all()), "zcol written for a row with col = -1"
        zrow, mrow = z.reshape(n, V)[node0:node0 + s], zmag[node0:node0 + s]
        check(f"stats epi {prec} t{tile} V{V} zfix", zfix.reshape(-1, 1), zrow[:, blank:blank + 1], ZCOL_TOL,
              scale=mrow[:, blank])
        have = ~none
        check(f"stats epi {prec} t{tile} V{V} zcol", zcol.cpu()[have].reshape(-1, 1),
              zrow.gather(1, labu[node0:node0 + s].long().clamp_min(0)[:, None])[have], ZCOL_TOL,
              scale=mrow.gather(1, labu[node0:node0 + s].long().clamp_min(0)[:, None])[have][:, 0])
        lib.check(lib.lib().eamd_rnnt_node_stats_part(ptr(part), ptr(zcol), ptr(zfix), ptr(ws), C.c_int64(node0), C.c_int64(s),
                                                      tn, B, T, U, stream()), "eamd_rnnt_node_stats_part")
        node0 += s
    ws = ws.view(5, B, T, U)
    check_stats(f"stats epi {prec} t{tile} V{V}", (ws[0], ws[1], ws[2]), ref, STATS_GEMM_TOL, extra=zmag.amax(-1))
    assert bool((ws[2, :, :, U - 1] == -INF).all())
    assert torch.isnan(ws[3:]).all()     # node_stats_part writes the first three blocks only


ROWCOEF_TOT_K = 7.0       # row_coef tot in units of 2^-24 S; observed 1.75
ROWCOEF_K = 1.9           # row_coef gb / gl in units of 2^-24 gamma S walk; observed 0.48 (gb)
ROWGRAD_K = 0.95          # epilogue 8 rows, units of 2^-24 * |sc| * max_v (exp(z + tot) + gb + gl) * (|tot| + max|z| + 1); observed 0.25 (fp32 V64)
ROWGRAD_BF16_K = 16000.0  # the same for the bf16 output alone (its own rounding: up to 2^-9 of an element); observed 4149 (V64)
LATTICE_BF16_K = 560.0    # bf16 output alone against the lattice gradient, units of check_grad; observed 145 (V64)


@gpu
@pytest.mark.parametrize("out", ["fp32", "bf16-C", "bf16-Cb", "bf16-both"])
@pytest.mark.parametrize("V", [777, 64])
def test_rnnt_row_coef_and_grad_epilogue(lib, ops, out, V):
    """eamd_rnnt_row_coef (tot, gb, gl) against float64, tot = -inf exactly outside the lattice, col exact; then
    EPI_ROW_GRAD from those coefficients (fp32 with C; bf16 operands with C only, Cb only, both: Cb = RNE(C)); odd V
    (ldc % 4 != 0: the scalar tail) and gscale != 1; rows with tot = -inf exactly 0; the rows against float64"""
    bf16 = out != "fp32"
    B, T, U, J = 2, 11, 8, 64
    n = B * T * U
    tl, ul = [11, 6], [7, 3]
    blank = 0
    H, W, bias, z, _ = joint_operands(V + len(out), B, T, U, J, V, bf16)
    g = torch.Generator().manual_seed(3 * V)
    lab = torch.randint(1, V, (B, U - 1), generator=g)
    for b in range(B):
        lab[b, ul[b]:] = blank
    gscale, scale = -0.37, 0.5
    sc = gscale * scale
    ref = lattice_ref(z, lab, tl, ul, blank, sc=sc)
    tld, uld, labd = i32(tl), i32(ul), labels_dev(lab, U)
    # the lattice workspace from the materialised logits (fp32)
    rc, _, ws, _ = rnnt_loss_call(lib, z.float().to(DEV), labd, tld, uld, blank, grad=False)
    lib.check(rc, "eamd_rnnt_loss")
    rowc = torch.full((n * 3,), NAN, device=DEV)
    col = torch.full((n,), 12345, dtype=torch.int32, device=DEV)
    node0, s = 5, n - 9
    lib.check(lib.lib().eamd_rnnt_row_coef(ptr(labd), ptr(tld), ptr(uld), ptr(ws), ptr(rowc[3 * node0:]), ptr(col[node0:]),
                                           C.c_int64(node0), C.c_int64(s), B, T, U, stream()), "eamd_rnnt_row_coef")
    rows = slice(node0, node0 + s)
    rc3 = f64(rowc).view(n, 3)
    assert torch.isnan(rc3[:node0]).all() and torch.isnan(rc3[node0 + s:]).all()
    inside = ref["inside"].reshape(-1)
    want_col = torch.where(inside & (torch.arange(U).repeat(B * T) < torch.tensor(ul).repeat_interleave(T * U)),
                           ref["labu"].reshape(-1), torch.full((n,), -1, dtype=torch.long))
    assert torch.equal(col.cpu()[rows].long(), want_col[rows])
    tot = rc3[rows, 0]
    out_ = ~inside[rows]
    assert bool((tot[out_] == -INF).all()) and bool((rc3[rows, 1:][out_] == 0).all())
    S = ref["S"].reshape(-1)[rows]
    check("row_coef tot", tot[~out_].reshape(-1, 1), ref["tot"].reshape(-1)[rows][~out_].reshape(-1, 1), ROWCOEF_TOT_K * EPS,
          scale=S[~out_])
    gsc = ref["gamma"].reshape(-1)[rows].clamp_min(GAMMA_FLOOR) * S * ref["walk"].reshape(-1)[rows] * EPS
    check("row_coef gb", rc3[rows, 1:2], ref["gb"].reshape(-1)[rows][:, None], ROWCOEF_K, scale=gsc)
    check("row_coef gl", rc3[rows, 2:3], ref["gl"].reshape(-1)[rows][:, None], ROWCOEF_K, scale=gsc)
    # epilogue 8 on the rows node0 .. node0 + s - 1
    ops.set_precision("fp32")
    Hd, Wd, bd = H.to(DEV), W.to(DEV), bias.to(DEV)
    gs = torch.tensor([gscale], device=DEV)
    C32 = torch.full((s, V), NAN, device=DEV) if out in ("fp32", "bf16-C", "bf16-both") else None
    Cb = torch.full((s, V), NAN, device=DEV).to(torch.bfloat16) if out in ("bf16-Cb", "bf16-both") else None
    Cm = C32 if C32 is not None else Cb
    ops.gemm(Hd[rows], Wd, Cm, s, V, J, J, J, V, bias=bd, epilogue=ops.EPI_ROW_GRAD, tile=64,
             stats=(rowc[3 * node0:], col[node0:], blank, gs, scale), Cb=Cb if C32 is not None else None, precision=0)
    if C32 is not None and Cb is not None:
        assert torch.equal(Cb.view(torch.int16), C32.to(torch.bfloat16).view(torch.int16))
    got = C32 if C32 is not None else Cb
    zrow = z.reshape(n, V)[rows]
    totc, gbc, glc = rc3[rows, 0:1], rc3[rows, 1:2], rc3[rows, 2:3]
    want = torch.exp(zrow + totc)
    want[:, blank] -= gbc[:, 0]
    cr = col.cpu()[rows].long()
    has = cr >= 0
    want[has, cr[has]] -= glc[has, 0]
    want = (want * sc).where(totc > -INF, torch.zeros(()).double())
    dead = (totc[:, 0] == -INF)
    assert bool((f64(got)[dead] == 0).all()), "rows with tot = -inf must be exactly 0"
    mag = abs(sc) * (torch.exp(zrow + totc).amax(-1) + gbc[:, 0] + glc[:, 0]) * (totc[:, 0].abs() + zrow.abs().amax(-1) + 1)
    mag = mag.where(~dead, torch.ones(()).double())
    k = ROWGRAD_K if C32 is not None else ROWGRAD_BF16_K
    check(f"rowgrad epi {out} V{V}", got, want, k * EPS, scale=mag)
    # and against the float64 gradient of the lattice itself
    check_grad(f"rowgrad epi {out} V{V} vs lattice", got.float().view(1, 1, s, V),
               {"gamma": ref["gamma"].reshape(-1)[rows], "S": S, "walk": ref["walk"].reshape(-1)[rows],
                "grad": ref["grad"].reshape(n, V)[rows]}, sc,
               GRAD_K if C32 is not None else LATTICE_BF16_K)


# ---------------------------------------------------------------------------------------------
# 4. joint kernels
# ---------------------------------------------------------------------------------------------
ACTS = {0: "none", 1: "relu", 2: "swish", 3: "tanh", 4: "hardtanh", 5: "selu"}
SELU_A, SELU_S = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946


def act64(x, a):
    if a == 1:
        return x.clamp_min(0)
    if a == 2:
        return x * torch.sigmoid(x)
    if a == 3:
        return torch.tanh(x)
    if a == 4:
        return x.clamp(-1, 1)
    if a == 5:
        return SELU_S * torch.where(x > 0, x, SELU_A * torch.expm1(x))
    return x


def dact64(x, a):
    if a == 1:
        return (x > 0).double()
    if a == 2:
        s = torch.sigmoid(x)
        return s * (1 + x * (1 - s))
    if a == 3:
        return 1 - torch.tanh(x) ** 2
    if a == 4:
        return ((x > -1) & (x < 1)).double()
    if a == 5:
        return SELU_S * torch.where(x > 0, torch.ones_like(x), SELU_A * torch.exp(x))
    return torch.ones_like(x)


JOINT_FWD_TOL = 3.3e-7    # |err| / max_j (|act(x)| + |act'(x)| |x|) per (b,t,u) row; observed 8.5e-8 (grid cap, tanh)
JOINT_BWD_TOL = 7.2e-7    # |err| / max_j sum |dh act'| per d_enc (b,t) / d_dec (b,u) row; observed 1.8e-7 (swish sliced d_enc)


@gpu
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("J", [1, 64, 320, 520])
def test_joint_fwd(lib, act, J):
    """eamd_joint_fwd, every activation, fp32 and bf16 output (bf16 = RNE of fp32, bit for bit)"""
    B, T, U = 2, 9, 5
    g = torch.Generator().manual_seed(J * 10 + act)
    e, d = torch.randn(B, T, J, generator=g) * 1.5, torch.randn(B, U, J, generator=g) * 1.5
    _joint_fwd_check(lib, e, d, act, f"joint fwd {ACTS[act]} J{J}")


def _joint_fwd_check(lib, e, d, act, name):
    B, T, J = e.shape
    U = d.shape[1]
    ed, dd = e.to(DEV), d.to(DEV)
    o32 = torch.full((B, T, U, J), NAN, device=DEV)
    o16 = torch.full((B, T, U, J), NAN, device=DEV).to(torch.bfloat16)
    lib.check(lib.lib().eamd_joint_fwd(ptr(ed), ptr(dd), ptr(o32), None, B, T, U, J, act, stream()), "eamd_joint_fwd")
    lib.check(lib.lib().eamd_joint_fwd(ptr(ed), ptr(dd), None, ptr(o16), B, T, U, J, act, stream()), "eamd_joint_fwd bf16")
    assert torch.equal(o16.view(torch.int16), o32.to(torch.bfloat16).view(torch.int16)), name
    x = e.double()[:, :, None, :] + d.double()[:, None, :, :]
    want = act64(x, act)
    s = (want.abs() + dact64(x, act).abs() * x.abs()).reshape(-1, J).amax(-1)
    check(name, o32, want, JOINT_FWD_TOL, scale=s)


@gpu
def test_joint_fwd_past_grid_cap(lib):
    """B*T*U*J > 65535 * 256: the grid-stride loop past the 65535-block cap"""
    B, T, U, J = 2, 170, 101, 520
    assert B * T * U * J > 65535 * 256
    g = torch.Generator().manual_seed(99)
    e, d = torch.randn(B, T, J, generator=g), torch.randn(B, U, J, generator=g)
    _joint_fwd_check(lib, e, d, 3, "joint fwd grid cap")


@gpu
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("form", ["one-slice", "sliced"])
def test_joint_bwd(lib, act, form):
    """eamd_joint_bwd: d_enc rows (b,t) and d_dec rows (b,u) against float64; 'sliced': B*U = 7 splits the frames into 8
    slices (T = 203, not a multiple of 8) added with atomics; 'one-slice': B*U = 39, T = 21; J = 300 > 256 threads"""
    B, T, U, J = (1, 203, 7, 300) if form == "sliced" else (3, 21, 13, 300)
    g = torch.Generator().manual_seed(act + (100 if form == "sliced" else 0))
    e, d = torch.randn(B, T, J, generator=g) * 1.5, torch.randn(B, U, J, generator=g) * 1.5
    dh = torch.randn(B, T, U, J, generator=g)
    ed, dd, dhd = e.to(DEV), d.to(DEV), dh.to(DEV)
    de = torch.full((B, T, J), NAN, device=DEV)
    ddec = torch.full((B, U, J), NAN, device=DEV)
    lib.check(lib.lib().eamd_joint_bwd(ptr(dhd), ptr(ed), ptr(dd), ptr(de), ptr(ddec), B, T, U, J, act, stream()),
              "eamd_joint_bwd")
    x = e.double()[:, :, None, :] + d.double()[:, None, :, :]
    p = dh.double() * dact64(x, act)
    name = f"joint bwd {ACTS[act]} {form}"
    check(name + " d_enc", de, p.sum(2), JOINT_BWD_TOL, scale=p.abs().sum(2).amax(-1).reshape(-1))
    check(name + " d_dec", ddec, p.sum(1), JOINT_BWD_TOL, scale=p.abs().sum(1).amax(-1).reshape(-1))


# ---------------------------------------------------------------------------------------------
# 5. end to end: JointRNNTLossFn
# ---------------------------------------------------------------------------------------------
# per row, relative to the row's sum of |terms| (the loss: relative to |loss|).  Observed, fp32: loss 1.4e-7, d e 2.0e-5,
# d d 2.8e-5, d W_out 3.8e-5, d b_out 3.7e-5 (config5-width); bf16: loss 2.1e-5, d e 2.8e-3 (declined-J),
# d d 3.1e-3, d W_out 3.5e-3, d b_out 2.3e-3 (config5-width)
E2E_TOL = {"fp32": {"loss": 5.5e-7, "d e": 7.8e-5, "d d": 1.1e-4, "d W_out": 1.5e-4, "d b_out": 1.45e-4},
           "bf16": {"loss": 8.4e-5, "d e": 1.1e-2, "d d": 1.2e-2, "d W_out": 1.38e-2, "d b_out": 9e-3}}

# (B, T, U, J, V, tlens, ulens, chunk_rows, act)
E2E_CASES = {
    "ragged": (3, 23, 9, 64, 777, [23, 17, 5], [8, 5, 0], 40, 3),
    "config5-width": (2, 14, 30, 320, 5000, [14, 9], [29, 17], 200, 3),
    "declined-J": (2, 12, 6, None, 130, [12, 7], [5, 3], 25, 2),
}


@gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(E2E_CASES))
def test_joint_rnnt_loss_fn(ops, prec, case):
    """JointRNNTLossFn on a ragged batch, several chunks per utterance, (0.37 loss).backward(), against the float64 chain
    act(e + d) W^T + b -> lattice_ref: the loss, rows (b,t) of d e (exactly 0 past tlens), rows (b,u) of d d, rows of
    d W_out and d b_out.  'declined-J': J = 33 (fp32) / 36 (bf16) operands the row-epilogue GEMM declines, so the
    function stores the logits instead"""
    import espnet_amd
    from espnet_amd import rnn_functional as R
    B, T, U, J, V, tl, ul, chunk, act = E2E_CASES[case]
    if J is None:
        J = 33 if prec == "fp32" else 36
    espnet_amd.set_precision(prec)
    try:
        g = torch.Generator().manual_seed(B * T + J)
        e0, d0 = torch.randn(B, T, J, generator=g) * 0.5, torch.randn(B, U, J, generator=g) * 0.5
        w0, b0 = torch.randn(V, J, generator=g) * (1.0 / math.sqrt(J)), torch.randn(V, generator=g) * 0.5
        lab = torch.randint(1, V, (B, U - 1), generator=g)
        for b in range(B):
            lab[b, ul[b]:] = 0
        e, d, w, bo = (t.to(DEV).requires_grad_(True) for t in (e0, d0, w0, b0))
        tld, uld, labd = i32(tl), i32(ul), labels_dev(lab, U)
        if case == "declined-J":
            H = ops.joint_fwd(e.detach()[:1, :2].contiguous(), d.detach()[:1], act, out_dtype=ops.act_dtype()).view(-1, J)
            ws = ops.rnnt_workspace(B, T, U, DEV)
            col = torch.zeros(H.shape[0], dtype=torch.int32, device=DEV)
            assert ops.rnnt_node_stats_fused(H, ops.wshadow(w.detach()), bo.detach(), col, ws, 0, B, T, U, 0) is False
            assert ops.rnnt_node_grad_fused(H, ops.wshadow(w.detach()), bo.detach(), labd, tld, uld, ws, 0, B, T, U, 0,
                                            torch.ones(1, device=DEV), 1.0, ops.act_dtype()) is None
        loss = R.JointRNNTLossFn.apply(e, d, w, bo, labd, tld, uld, 0, act, tl, chunk)
        (0.37 * loss).backward()
        # float64 chain on the same operands
        e64, d64, w64, b64 = (t.double().requires_grad_(True) for t in (e0, d0, w0, b0))
        Hd = act64(e64[:, :, None, :] + d64[:, None, :, :], act)
        Z = Hd @ w64.t() + b64
        sc = 0.37 / B
        ref = lattice_ref(Z.detach(), lab, tl, ul, 0, sc=sc)
        Z.backward(ref["grad"])
        tol = E2E_TOL[prec]
        name = f"e2e {prec} {case}"
        check(name + " loss", loss.detach().reshape(1, 1), ref["loss"].mean().reshape(1, 1), tol["loss"])
        # row scales: sums of |terms|
        dZ = ref["grad"]
        x = (e64.detach()[:, :, None, :] + d64.detach()[:, None, :, :])
        pa = (dZ.abs() @ w64.detach().abs()) * dact64(x, act).abs()
        check(name + " d e", e.grad, e64.grad, tol["d e"], scale=pa.sum(2).amax(-1).reshape(-1).clamp_min(1e-30))
        for b in range(B):
            assert bool((e.grad[b, tl[b]:] == 0).all()), f"{name}: d e past tlens[{b}] must be exactly 0"
        check(name + " d d", d.grad, d64.grad, tol["d d"], scale=pa.sum(1).amax(-1).reshape(-1).clamp_min(1e-30))
        Hf = Hd.detach().reshape(-1, J)
        dZf = dZ.reshape(-1, V)
        check(name + " d W_out", w.grad, w64.grad, tol["d W_out"], scale=(dZf.abs().t() @ Hf.abs()).amax(-1).clamp_min(1e-30))
        check(name + " d b_out", bo.grad.reshape(-1, 1), b64.grad.reshape(-1, 1), tol["d b_out"],
              scale=dZf.abs().sum(0).clamp_min(1e-30))
    finally:
        espnet_amd.set_precision("fp32")
