"""Conformer conv-module and front-end convolution kernels (csrc/convmod.hip, eamd_mask_time) against float64 on every
dispatch path: BatchNorm statistics (every bn_geom slab shape, both trips of the finalize loop, groups that see no
slab, the statistics left by eamd_dwconv_glu_fwd's epilogue), BatchNorm apply / backward (six activations, training and
eval, the grid-stride second trip), the time-bounded forms, the depthwise convolution (several tiles per block in the
weight gradient, T below one tile and below the halo, refused kernel sizes) and the first 3x3 convolution of both
front-ends (stride 2 / pad 0 and stride 1 / pad 1: pair and non-pair bf16 forms, both NPOS trips, several rows per
block, the LDS row limit).

The reference is plain torch in float64 on the CPU from the same fp32 inputs.  Every comparison is element-wise: a sum
of products is judged against the float64 sum of the absolute values of its terms (cancellation does not inflate the
bound), BatchNorm outputs against the row's / channel's scale.  Output buffers are filled with NaN before the launch;
accumulated buffers start from non-zero values and are called twice.  Each test recomputes the launch geometry from the
host code's formulas and asserts that the intended branch is reached.

Each bound is a named constant at the top of its section.  For the kernels that only add and multiply the error must
also sit under the a-priori bound (n_terms + 8) * 2^-24 (one rounding per term of the longest sum plus a few for the
operands), asserted with every such check.  Each constant is at most 4x the largest error observed under its name
on an MI355X, noted beside it; every check prints its observed error, and the share of the scale that a kink allowance
takes, in a "[convmod] <constant> <case>" line."""
import ctypes as ct
import math

import pytest
import torch
import torch.nn.functional as F


pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
INF = float("inf")
U24 = 2.0 ** -24
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ops():
    from espnet_amd import ops as o
    o.set_precision("fp32")
    return o


@pytest.fixture(scope="module")
def lib():
    from espnet_amd import _lib
    return _lib


def apriori(n_terms):
    return (n_terms + 8) * U24


def nan_(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def cdiv(a, b):
    return -(-a // b)


def check(tolname, name, got, ref, scale, n_terms=None, keep=None, slack=None):
    """max over elements of |got - ref| / scale (scale broadcast against ref), in float64, with the worst element's
    index.  keep: elements left out of the comparison where False; slack: an absolute allowance taken off the error
    first.  A NaN (an unwritten element) is an infinite error.  n_terms: also assert the a-priori bound."""
    tol = globals()[tolname]
    g = got.detach().double().cpu().reshape(ref.shape)
    r = ref.detach().double()
    d = (g - r).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, INF), d)
    note = ""
    if slack is not None:
        sl = slack.detach().double().expand_as(d)
        d = (d - sl).clamp_min(0.0)
        note = f", largest allowance / scale {float((sl / scale.detach().double().expand_as(d)).max()):.1e}"
    if keep is not None:
        d = torch.where(keep, d, torch.zeros_like(d))
    s = scale.detach().double().expand_as(d)
    e = torch.where(d == 0, torch.zeros_like(d), d / s).reshape(-1)
    i = int(e.argmax()) if e.numel() else 0
    worst = float(e[i]) if e.numel() else 0.0
    idx, j = [], i
    for n in reversed(ref.shape):
        idx.insert(0, j % n)
        j //= n
    idx = tuple(idx)
    extra = "" if n_terms is None else f", a-priori {apriori(n_terms):.3g}"
    print(f"[convmod] {tolname} {name}: max err/scale {worst:.3e} at {idx} (tol {tol:g}{extra}{note})")
    assert worst <= tol, f"{name}: element {idx} error/scale {worst:.3e} > {tolname} = {tol:g}"
    if n_terms is not None:
        assert worst <= apriori(n_terms), f"{name}: {worst:.3e} above the a-priori bound of {n_terms} terms"
    return worst


def row_scale(ref, floor):
    return ref.abs().amax(-1, keepdim=True).clamp_min(floor)


# =============================================================================================
# 1. BatchNorm statistics
# =============================================================================================
BN_EPS = 1e-5
BN_MEAN_TOL = 4.8e-7   # mean / running_mean, relative to the channel's max |x| (+ the running start); observed 1.23e-7
BN_RSTD_TOL = 8.4e-7   # rstd, relative (division and rsqrtf inside: the 4x rule alone); observed 2.11e-7
BN_RVAR_TOL = 8.4e-7   # running_var, relative (the 4x rule alone); observed 2.12e-7
# x = 1000 + randn: the partial means are fp32 numbers near 1000 (ulp 6e-5 against a spread of 1), and each Chan merge
# carries that rounding into the cross term d * d * n * f: 2 d (6e-5) per merge, incoherently over the merges.  That is
# what the observed 1.2e-5 is; the slab sums themselves are exact two-pass.
BN_OFFSET_VAR_TOL = 4.9e-5   # unbiased variance / rstd of x = 1000 + randn, relative; observed 1.23e-5 (rstd 6.1e-6)
# a one-pass E[x^2] - mean^2 in fp32 would miss this by about 2^-24 * mean^2 / var = 6e-2
BN_OFFSET_VAR_CEILING = 1e-3


def bn_geom(Cc):
    """bn_geom of convmod.hip: float4 channel groups, row-subgroups of a 256-thread block, rows per slab (BN_R = 4)"""
    cq = Cc // 4
    rs = 256 // cq
    return cq, rs, 4 * rs


def bn_stats_call(lib, x, rm, rv, nbt, momentum, bound=None):
    """eamd_bn_stats / eamd_bn_stats_bounded on x [M, C] (bound = (T, int32 device scalar)) -> mean, rstd"""
    M, Cc = x.shape
    L = lib.lib()
    nslab = L.eamd_bn_nslab(ct.c_int64(M), Cc)
    assert nslab == cdiv(M, bn_geom(Cc)[2])
    ws, mean, rstd = nan_(3 * Cc * nslab), nan_(Cc), nan_(Cc)
    p = lib.ptr
    if bound is None:
        lib.check(L.eamd_bn_stats(p(x), p(ws), p(mean), p(rstd), p(rm), p(rv), p(nbt), ct.c_int64(M), Cc, ct.c_float(BN_EPS),
                                  ct.c_float(momentum), lib.stream_ptr()), "eamd_bn_stats")
    else:
        lib.check(L.eamd_bn_stats_bounded(p(x), p(ws), p(mean), p(rstd), p(rm), p(rv), p(nbt), ct.c_int64(M), Cc,
                                          ct.c_float(BN_EPS), ct.c_float(momentum), bound[0], p(bound[1]), lib.stream_ptr()),
                  "eamd_bn_stats_bounded")
    return mean, rstd


def bn_stats_ref(x64, rm, rv, momentum):
    rmd, rvd = rm.double().clone(), rv.double().clone()
    F.batch_norm(x64, rmd, rvd, None, None, True, momentum, BN_EPS)        # running update: unbiased variance
    var = x64.var(0, unbiased=False)
    return x64.mean(0), (var + BN_EPS).rsqrt(), rmd, rvd


def bn_stats_check(name, x64, got, rm0, rv0, momentum):
    """got = (mean, rstd, running_mean, running_var) of the kernel; x64 the rows that take part"""
    mean, rstd, rm, rv = got
    rmean, rrstd, rrm, rrv = bn_stats_ref(x64, rm0, rv0, momentum)
    n = x64.shape[0]
    xmax = x64.abs().amax(0)
    check("BN_MEAN_TOL", f"{name} mean", mean, rmean, xmax, n_terms=n)
    # rstd and the running statistics pass through a division, rsqrtf and the momentum blend: the 4x rule alone
    check("BN_RSTD_TOL", f"{name} rstd", rstd, rrstd, rrstd)
    check("BN_MEAN_TOL", f"{name} running_mean", rm, rrm, (1 - momentum) * rm0.double().abs() + momentum * xmax)
    check("BN_RVAR_TOL", f"{name} running_var", rv, rrv, rrv)


# (M, C, slab_rows, nslab, idle threads of the statistics block)
BN_SHAPES = [(50, 4, 1024, 1, 0), (2500, 4, 1024, 3, 0), (87, 100, 40, 3, 6), (1000, 144, 28, 36, 4),
             (7968 // 8, 256, 16, 63, 0), (1030, 768, 4, 258, 64), (1100, 1024, 4, 275, 0), (9, 1024, 4, 3, 0)]


@pytest.mark.parametrize("M,Cc,slab_rows,nslab,idle", BN_SHAPES)
def test_bn_stats_vs_float64(lib, M, Cc, slab_rows, nslab, idle):
    """every bn_geom slab shape; nslab > 256 = second trip of bn_finalize's 8-slab loop (clamped loads on the ragged
    last group), nslab < 32 = finalize groups with no slab, C % 32 != 0 = a last finalize block with dead channels, M not
    a multiple of slab_rows = a partly empty slab.  Launched with two momenta from non-trivial running statistics: mean
    and rstd of the two launches are bit-identical (fixed merge order), num_batches_tracked goes up by one each."""
    cq, rs, sr = bn_geom(Cc)
    assert (sr, cdiv(M, sr), 256 - cq * rs) == (slab_rows, nslab, idle)
    g = torch.Generator().manual_seed(100 + M + Cc)
    x = torch.randn(M, Cc, generator=g) * 2 + 1
    rm0, rv0 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    xd, x64 = x.to(DEV), x.double()
    nbt = torch.full((), 7, dtype=torch.int64, device=DEV)
    first = None
    for k, momentum in enumerate((0.1, 0.25)):
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        mean, rstd = bn_stats_call(lib, xd, rm, rv, nbt, momentum)
        assert int(nbt) == 8 + k
        bn_stats_check(f"bn_stats M={M} C={Cc} mom={momentum}", x64, (mean, rstd, rm, rv), rm0, rv0, momentum)
        if first is None:
            first = (mean, rstd)
        else:
            assert torch.equal(first[0], mean) and torch.equal(first[1], rstd), "statistics are not reproducible"


def test_bn_stats_large_offset(lib):
    """x = 1000 + randn: the slab statistics are an exact two-pass and slabs merge by Chan's update, so the variance
    keeps its digits where a one-pass sum of squares loses them all (momentum 1: running_var is the unbiased variance)"""
    M, Cc = 996, 256
    g = torch.Generator().manual_seed(5)
    x = 1000 + torch.randn(M, Cc, generator=g)
    rm, rv = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
    mean, rstd = bn_stats_call(lib, x.to(DEV), rm, rv, None, 1.0)
    x64 = x.double()
    check("BN_MEAN_TOL", "bn_stats offset mean", mean, x64.mean(0), x64.abs().amax(0), n_terms=M)
    var = x64.var(0, unbiased=True)
    e = check("BN_OFFSET_VAR_TOL", "bn_stats offset running_var", rv, var, var)
    assert e < BN_OFFSET_VAR_CEILING
    check("BN_OFFSET_VAR_TOL", "bn_stats offset rstd", rstd, (x64.var(0, unbiased=False) + BN_EPS).rsqrt(),
          (x64.var(0, unbiased=False) + BN_EPS).rsqrt())


# ---- depthwise convolution references (also used by section 4) ---------------------------------
def conv_dw(u, w, b, K):
    return F.conv1d(u.transpose(1, 2), w.unsqueeze(1), b, padding=(K - 1) // 2, groups=w.shape[0]).transpose(1, 2)


def dw_ref(x, w, b, dy, K, glu=False):
    """float64 depthwise convolution of x [B, T, C] (or of GLU(x), x [B, T, 2C]) with its gradients, and for each result
    the sum of the absolute values of its terms (the same graph on absolute values).  The GLU input gradient is the
    depthwise one times the local factors sigmoid(g) / v sigmoid(g) (1 - sigmoid(g)): its scale carries their modulus."""
    xd, wd, bd = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    u = F.glu(xd, -1) if glu else xd
    y = conv_dw(u, wd, bd, K)
    dyd = None if dy is None else dy.double()
    r = dict(y=y.detach())
    ua, wa, ba = (t.detach().abs().requires_grad_(True) for t in (u, wd, bd))
    ya = conv_dw(ua, wa, ba, K)
    r["ys"] = ya.detach()
    if dy is not None:
        y.backward(dyd)
        ya.backward(dyd.abs())
        r.update(dx=xd.grad, dw=wd.grad, db=bd.grad, dws=wa.grad, dbs=ba.grad)
        if glu:
            v, gt = xd.detach().chunk(2, -1)
            s = torch.sigmoid(gt)
            r["dxs"] = torch.cat([ua.grad * s, ua.grad * v.abs() * s * (1 - s)], -1)
        else:
            r["dxs"] = ua.grad
    return r


def dw_glu_fwd_call(lib, a, w, b, B, T, Cc, K, part=None):
    y = nan_(B * T, Cc)
    p = lib.ptr
    rc = lib.lib().eamd_dwconv_glu_fwd(p(a), p(w), p(b), p(y), p(part), B, T, Cc, K, lib.stream_ptr())
    return rc, y


# __expf / rcpf inside: no derivable ceiling, the 4x rule alone
DW_GLU_FWD_TOL = 8.9e-7   # dwconv(GLU(a)) relative to sum_k |w| |GLU(a)| + |bias|; observed 2.24e-7


@pytest.mark.parametrize("B,T,Cc,K", [(3, 5500, 64, 31), (2, 65, 100, 7)])
def test_dwconv_glu_fwd_epilogue_stats(lib, B, T, Cc, K):
    """the BatchNorm partials left by eamd_dwconv_glu_fwd's epilogue (one slab per 64-frame tile) merged by
    eamd_bn_finalize: more than 256 slabs (second finalize trip), and T = 65 (a tile of one frame); the statistics are
    those of the fp32 y the launch wrote, and y is bit-identical to the launch without bn_part"""
    nslab = B * cdiv(T, 64)
    assert nslab > 256 or T % 64 == 1
    g = torch.Generator().manual_seed(7 + T)
    a = torch.randn(B, T, 2 * Cc, generator=g)
    w, b = torch.randn(Cc, K, generator=g) / math.sqrt(K), torch.randn(Cc, generator=g)
    ad, wd, bd = a.to(DEV), w.to(DEV), b.to(DEV)
    rc, y0 = dw_glu_fwd_call(lib, ad, wd, bd, B, T, Cc, K)
    assert rc == 0
    part = nan_(3 * Cc * nslab)
    rc, y = dw_glu_fwd_call(lib, ad, wd, bd, B, T, Cc, K, part)
    assert rc == 0
    assert torch.equal(y, y0)
    r = dw_ref(a, w, b, None, K, glu=True)
    check("DW_GLU_FWD_TOL", f"dwconv_glu_fwd {B}x{T}x{Cc} K={K}", y, r["y"].reshape(B * T, Cc), r["ys"].reshape(B * T, Cc))
    rm0, rv0 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    p = lib.ptr
    nbt = torch.full((), 3, dtype=torch.int64, device=DEV)
    outs = []
    for k in range(2):
        rm, rv, mean, rstd = rm0.to(DEV), rv0.to(DEV), nan_(Cc), nan_(Cc)
        lib.check(lib.lib().eamd_bn_finalize(p(part), nslab, p(mean), p(rstd), p(rm), p(rv), p(nbt), Cc, ct.c_float(BN_EPS),
                                             ct.c_float(0.1), lib.stream_ptr()), "eamd_bn_finalize")
        assert int(nbt) == 4 + k
        outs.append((mean, rstd))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    bn_stats_check(f"glu epilogue stats {B}x{T}x{Cc}", y.double().cpu(), (mean, rstd, rm, rv), rm0, rv0, 0.1)


# =============================================================================================
# 2. BatchNorm apply and backward
# =============================================================================================
ACTS = {"none": 0, "relu": 1, "swish": 2, "tanh": 3, "hardtanh": 4, "selu": 5}
SELU_ALPHA, SELU_SCALE = 1.6732632423543772, 1.0507009873554805
# kinks of the derivative and the size of its jump there
KINKS = {"relu": ((0.0,), 1.0), "hardtanh": ((-1.0, 1.0), 1.0), "selu": ((0.0,), SELU_SCALE * (SELU_ALPHA - 1.0))}
ALGEBRAIC = ("none", "relu", "hardtanh")      # add, multiply, compare; the others call __expf / rcpf / tanhf / expm1f
BN_ROW_FLOOR = 1.0   # y / dx rows are scaled by max |ref|, at least 1: pre-activations and dy are N(0, 1)-scale, a row
#                      whose reference is smaller (ReLU with every unit dead, C = 4) is judged in absolute terms
# mean / rstd are the fp32 results of eamd_bn_stats in training mode, so their error is part of what is observed; the
# (n + 8) 2^-24 bound is asserted on dgamma / dbeta where act = none (observed at most 0.35 of it)
BN_Y_ALG_TOL = 1.6e-6      # y, act none / relu / hardtanh; observed 4.06e-7
BN_Y_TRANS_TOL = 1.3e-6    # y, swish / tanh / selu (no derivable ceiling: the 4x rule alone); observed 3.28e-7
BN_DX_ALG_TOL = 1.0e-6     # dx; observed 2.58e-7
BN_DX_TRANS_TOL = 2.1e-6   # dx (the 4x rule alone); observed 5.39e-7
BN_DGB_ALG_TOL = 8.2e-7    # dgamma / dbeta relative to sum |dz xhat| / sum |dz| + |start|; observed 2.05e-7
BN_DGB_TRANS_TOL = 2.5e-6  # (the 4x rule alone); observed 6.34e-7
KINK_SHARE = 1e-3


def act_ref(z, act):
    return {"none": lambda t: t, "relu": torch.relu, "swish": lambda t: t * torch.sigmoid(t), "tanh": torch.tanh,
            "hardtanh": F.hardtanh, "selu": F.selu}[act](z)


def bn_ref(x, gamma, beta, dy, act, training, rm=None, rv=None):
    """float64 BatchNorm1d + activation over x [M, C] and its gradients; training: batch statistics, else (rm, rv).
    near: elements whose pre-activation lies within 1e-5 * max(1, |z|) of a kink of the derivative.  sb / sg: what those
    elements could move dbeta / dgamma by if fp32 puts them on the other side (|dy| jump, times |xhat|)."""
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    if training:
        z = F.batch_norm(xd, None, None, gd, bd, True, 0.0, BN_EPS)
        mean, rstd = xd.detach().mean(0), (xd.detach().var(0, unbiased=False) + BN_EPS).rsqrt()
    else:
        z = F.batch_norm(xd, rm.double(), rv.double(), gd, bd, False, 0.0, BN_EPS)
        mean, rstd = rm.double(), (rv.double() + BN_EPS).rsqrt()
    z.retain_grad()
    y = act_ref(z, act)
    y.backward(dy.double())
    zz, dz = z.detach(), z.grad
    xh = (xd.detach() - mean) * rstd
    near = torch.zeros_like(zz, dtype=torch.bool)
    jump = 0.0
    if act in KINKS:
        pts, jump = KINKS[act]
        for k in pts:
            near |= (zz - k).abs() <= 1e-5 * zz.abs().clamp_min(1.0)
    flip = torch.where(near, dy.double().abs() * jump, torch.zeros_like(zz))
    return dict(y=y.detach(), dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad, near=near, share=float(near.double().mean()),
                dbs=dz.abs().sum(0), dgs=(dz * xh).abs().sum(0), sb=flip.sum(0), sg=(flip * xh.abs()).sum(0),
                xh=xh, grs=(gd.detach() * rstd).abs(), mean=mean, rstd=rstd)


def bn_bwd_call(lib, dy, x, mean, rstd, gamma, beta, dgamma, dbeta, act, training, bound=None):
    M, Cc = x.shape
    L = lib.lib()
    nslab = L.eamd_bn_nslab(ct.c_int64(M), Cc)
    ws, dx = nan_((2 * nslab + 2) * Cc), nan_(M, Cc)
    p = lib.ptr
    if bound is None:
        lib.check(L.eamd_bn_bwd(p(dy), p(x), p(mean), p(rstd), p(gamma), p(beta), p(ws), p(dx), p(dgamma), p(dbeta),
                                ct.c_int64(M), Cc, act, training, lib.stream_ptr()), "eamd_bn_bwd")
    else:
        lib.check(L.eamd_bn_bwd_bounded(p(dy), p(x), p(mean), p(rstd), p(gamma), p(beta), p(ws), p(dx), p(dgamma), p(dbeta),
                                        ct.c_int64(M), Cc, act, training, bound[0], p(bound[1]), lib.stream_ptr()),
                  "eamd_bn_bwd_bounded")
    return dx


def bn_bwd_check(name, act, training, r, dx, dg, db, dg0, db0, ncall, n_rows, keep_rows=None):
    """dx / dgamma / dbeta of the kernel against bn_ref's r (over the n_rows rows that take part).  dgamma / dbeta sum
    every element, the near-kink ones included, so their error may carry those elements' flips (r['sb'], r['sg']); in
    training mode dx holds the same sums over M, and carries that term too.  Elements near a kink are left out of dx."""
    alg = act in ALGEBRAIC
    assert r["share"] <= KINK_SHARE, f"{name}: {r['share']:.2e} of the elements lie at a kink: pick another seed"
    slack = None
    if act in KINKS and training:
        slack = r["grs"] * (r["sb"] + r["xh"].abs() * r["sg"]) / n_rows
    if dx is not None:
        check("BN_DX_ALG_TOL" if alg else "BN_DX_TRANS_TOL", f"{name} dx", dx, r["dx"], row_scale(r["dx"], BN_ROW_FLOOR),
              keep=~r["near"], slack=slack)
    nt = n_rows if act == "none" else None
    tn = "BN_DGB_ALG_TOL" if alg else "BN_DGB_TRANS_TOL"
    check(tn, f"{name} dgamma x{ncall}", dg, dg0.double() + ncall * r["dgamma"], dg0.double().abs() + ncall * r["dgs"],
          n_terms=nt, slack=ncall * r["sg"])
    check(tn, f"{name} dbeta x{ncall}", db, db0.double() + ncall * r["dbeta"], db0.double().abs() + ncall * r["dbs"],
          n_terms=nt, slack=ncall * r["sb"])


# the bn_geom shapes of section 1 with distinct geometry, and M * C > 4096 * 256 (grid-stride second trip of
# bn_apply_kernel / bn_bwd_apply_kernel: grid_for caps the grid at 4096 blocks of 256 threads)
BN_APPLY_SHAPES = [(50, 4), (87, 100), (1000, 144), (996, 256), (1030, 768), (1100, 1024), (4104, 256)]


def bn_inputs(M, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, Cc, generator=g) * 2 + 1
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)      # both sides of every kink
    dy = torch.randn(M, Cc, generator=g)
    rm, rv = 1 + 0.5 * torch.randn(Cc, generator=g), 4 * (torch.rand(Cc, generator=g) + 0.5)   # not the batch's
    dg0, db0 = torch.randn(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) - 0.5
    return x, gamma, beta, dy, rm, rv, dg0, db0


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("M,Cc", BN_APPLY_SHAPES)
def test_bn_apply_bwd_vs_float64(lib, M, Cc, act):
    """eamd_bn_apply (fp32 and bf16) and eamd_bn_bwd for each activation, in training mode (mean / rstd from
    eamd_bn_stats on the device) and with training = 0 (mean / rstd from running statistics that differ from the
    batch's); dgamma / dbeta start non-zero and the backward is called twice"""
    if (M, Cc) == (4104, 256):
        assert M * Cc > 4096 * 256
    x, gamma, beta, dy, rm, rv, dg0, db0 = bn_inputs(M, Cc, 31 * M + Cc)
    xd, gd, bd, dyd = x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)
    p = lib.ptr
    alg = act in ALGEBRAIC
    for training in (1, 0):
        name = f"bn {act} M={M} C={Cc} train={training}"
        r = bn_ref(x, gamma, beta, dy, act, bool(training), rm, rv)
        if training:
            mean, rstd = bn_stats_call(lib, xd, None, None, None, 0.1)
        else:
            mean, rstd = r["mean"].float().to(DEV), r["rstd"].float().to(DEV)
        y32, y16 = nan_(M, Cc), nan_(M, Cc, dtype=torch.bfloat16)
        for y, bf in ((y32, 0), (y16, 1)):
            lib.check(lib.lib().eamd_bn_apply(p(xd), p(mean), p(rstd), p(gd), p(bd), p(y), ct.c_int64(M), Cc, ACTS[act], bf,
                                              lib.stream_ptr()), "eamd_bn_apply")
        check("BN_Y_ALG_TOL" if alg else "BN_Y_TRANS_TOL", f"{name} y", y32, r["y"], row_scale(r["y"], BN_ROW_FLOOR))
        assert torch.equal(y16, y32.to(torch.bfloat16)), f"{name}: bf16 y is not the fp32 y rounded once"
        dg, db = dg0.to(DEV), db0.to(DEV)
        for ncall in (1, 2):
            dx = bn_bwd_call(lib, dyd, xd, mean, rstd, gd, bd, dg, db, ACTS[act], training)
            bn_bwd_check(name, act, training, r, dx if ncall == 1 else None, dg, db, dg0, db0, ncall, M)
            if ncall == 2:
                assert torch.equal(dx, dx1), f"{name}: dx differs between two launches"
            dx1 = dx


# =============================================================================================
# 3. time-bounded forms
# =============================================================================================
# (B, T, tb, C); the last is the grid-stride case (M = 4104)
BOUNDED_SHAPES = [(3, 70, 37, 256), (4, 64, 64, 100), (2, 129, 1, 144), (8, 513, 300, 256)]


def bounded_inputs(B, T, tb, Cc):
    x, gamma, beta, dy, rm, rv, dg0, db0 = bn_inputs(B * T, Cc, 17 * T + tb)
    x, dy = x.view(B, T, Cc).clone(), dy.view(B, T, Cc).clone()
    if tb == 1:
        # two rows take part: keep them at least 1 apart in every channel, so rstd stays O(1) and the test measures the
        # kernel rather than the conditioning of a two-sample variance
        x[1, 0] = x[0, 0] + torch.sign(x[1, 0] - x[0, 0]) * (1 + (x[1, 0] - x[0, 0]).abs())
    x[:, tb:] = NAN          # rows from the bound on are not read
    dy[:, tb:] = NAN
    return x, gamma, beta, dy, rm, rv, dg0, db0


@pytest.mark.parametrize("B,T,tb,Cc", BOUNDED_SHAPES)
def test_bn_stats_bounded_vs_cropped(lib, B, T, tb, Cc):
    """eamd_bn_stats_bounded with NaN in every row t >= tb (tb read from a device scalar) = the float64 statistics of the
    batch cropped to t < tb, B * tb rows counted"""
    x, _, _, _, rm0, rv0, _, _ = bounded_inputs(B, T, tb, Cc)
    tbd = torch.tensor([tb], dtype=torch.int32, device=DEV)
    xd = x.view(B * T, Cc).to(DEV)
    x64 = x[:, :tb].reshape(B * tb, Cc).double()
    nbt = torch.full((), 0, dtype=torch.int64, device=DEV)
    outs = []
    for k in range(2):
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        mean, rstd = bn_stats_call(lib, xd, rm, rv, nbt, 0.1, bound=(T, tbd))
        assert int(nbt) == k + 1
        outs.append((mean, rstd))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    bn_stats_check(f"bn_stats_bounded {B}x{T} tb={tb} C={Cc}", x64, (mean, rstd, rm, rv), rm0, rv0, 0.1)


@pytest.mark.parametrize("act", ["none", "swish"])
@pytest.mark.parametrize("B,T,tb,Cc", BOUNDED_SHAPES)
def test_bn_bwd_bounded_vs_cropped(lib, B, T, tb, Cc, act):
    """eamd_bn_bwd_bounded with NaN in x and dy on every row t >= tb: dgamma / dbeta / dx equal the cropped batch's
    (1 / M counting B * tb rows), dx is exactly 0 from the bound on"""
    x, gamma, beta, dy, _, _, dg0, db0 = bounded_inputs(B, T, tb, Cc)
    if (B, T) == (8, 513):
        assert B * T * Cc > 4096 * 256
    tbd = torch.tensor([tb], dtype=torch.int32, device=DEV)
    xd, dyd, gd, bd = x.view(B * T, Cc).to(DEV), dy.view(B * T, Cc).to(DEV), gamma.to(DEV), beta.to(DEV)
    n = B * tb
    r = bn_ref(x[:, :tb].reshape(n, Cc), gamma, beta, dy[:, :tb].reshape(n, Cc), act, True)
    mean, rstd = bn_stats_call(lib, xd, None, None, None, 0.1, bound=(T, tbd))
    dg, db = dg0.to(DEV), db0.to(DEV)
    name = f"bn_bwd_bounded {act} {B}x{T} tb={tb} C={Cc}"
    for ncall in (1, 2):
        dx = bn_bwd_call(lib, dyd, xd, mean, rstd, gd, bd, dg, db, ACTS[act], 1, bound=(T, tbd)).view(B, T, Cc)
        assert bool((dx[:, tb:] == 0).all()), f"{name}: dx is not 0 from the bound on"
        live = dx[:, :tb].reshape(n, Cc)
        bn_bwd_check(name, act, 1, r, live if ncall == 1 else None, dg, db, dg0, db0, ncall, n)
        if ncall == 2:
            assert torch.equal(live, live1)
        live1 = live.clone()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,tb,Cc", BOUNDED_SHAPES + [(3, 70, 70, 256)])
def test_mask_time_bit_exact(ops, B, T, tb, Cc, dtype):
    """eamd_mask_time: rows t >= tb become +0 whatever they held (NaN, inf, -0), every other element keeps its bits"""
    if (B, T) == (8, 513):
        assert B * T * Cc > 4096 * 256
    g = torch.Generator().manual_seed(T + tb)
    x = torch.randn(B, T, Cc, generator=g)
    pick = torch.rand(B, T, Cc, generator=g)
    x[pick < 0.02] = NAN
    x[(pick >= 0.02) & (pick < 0.04)] = -0.0
    x[(pick >= 0.04) & (pick < 0.05)] = INF
    x = x.to(dtype)
    ibits = torch.int32 if dtype == torch.float32 else torch.int16
    bits = x.view(ibits)
    want = torch.where((torch.arange(T) >= tb)[None, :, None], torch.zeros((), dtype=ibits), bits)
    xd = x.view(B * T, Cc).to(DEV)
    ops.mask_time(xd, T, torch.tensor([tb], dtype=torch.int32, device=DEV))
    assert torch.equal(xd.view(ibits).cpu().view(B, T, Cc), want)


# =============================================================================================
# 4. depthwise convolution
# =============================================================================================
# plain forms: add and multiply only, the a-priori bound ((31 + 8) 2^-24 = 2.3e-6 for the 31 taps) is asserted as well;
# the weight gradients are added with float atomics across blocks, so their last bits vary from run to run
DW_FWD_TOL = 8.2e-7        # y relative to sum_k |w| |x| + |bias|; observed 2.06e-7
DW_BWD_X_TOL = 1.0e-6      # dx relative to sum_k |w| |dy|; observed 2.65e-7
DW_BWD_W_TOL = 4.8e-7      # dw / db relative to sum_{b,t} |dy| |x| (/ sum |dy|) + |start|; observed 1.21e-7
DW_GLU_BWD_X_TOL = 2.5e-6  # da relative to sum_k |w| |dy| times the GLU factor (the 4x rule alone); observed 6.26e-7
DW_GLU_BWD_W_TOL = 6.3e-7  # dw relative to sum |dy| |GLU(a)| + |start| (the 4x rule alone); observed 1.59e-7


def dw_bwd_w_geom(B, T, Cc):
    """eamd_dwconv_bwd_w's launch: tiles of 64 frames, about 512 blocks -> (tiles, grid y, tiles per block)"""
    total = B * cdiv(T, 64)
    gx = cdiv(Cc, 64)
    gy = max(1, min(cdiv(512, gx), total))
    tpb = cdiv(total, gy)
    return total, cdiv(total, tpb), tpb


def dw_inputs(B, T, Cc, K, glu, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 2 * Cc if glu else Cc, generator=g)
    w, b = torch.randn(Cc, K, generator=g), torch.randn(Cc, generator=g)
    dy = torch.randn(B, T, Cc, generator=g)
    dw0, db0 = torch.randn(Cc, K, generator=g) + 0.5, torch.randn(Cc, generator=g) - 0.5
    return x, w, b, dy, dw0, db0


def dw_bwd_w_check(lib, name, x, dy, r, dw0, db0, B, T, Cc, K, glu):
    fn = lib.lib().eamd_dwconv_glu_bwd_w if glu else lib.lib().eamd_dwconv_bwd_w
    tn = "DW_GLU_BWD_W_TOL" if glu else "DW_BWD_W_TOL"
    nt = None if glu else B * T
    dw, db = dw0.to(DEV), db0.to(DEV)
    xd, dyd = x.to(DEV), dy.to(DEV)
    p = lib.ptr
    for ncall in (1, 2):
        lib.check(fn(p(dyd), p(xd), p(dw), p(db), B, T, Cc, K, lib.stream_ptr()), "dwconv_bwd_w")
        check(tn, f"{name} dw x{ncall}", dw, dw0.double() + ncall * r["dw"], dw0.double().abs() + ncall * r["dws"], n_terms=nt)
        check(tn, f"{name} db x{ncall}", db, db0.double() + ncall * r["db"], db0.double().abs() + ncall * r["dbs"],
              n_terms=None if glu else B * T)


@pytest.mark.parametrize("glu", [False, True])
@pytest.mark.parametrize("B,T,Cc,K,last_short", [(6, 400, 1024, 7, False), (1, 2561, 1024, 3, True)])
def test_dwconv_bwd_w_tiles_per_block(lib, B, T, Cc, K, last_short, glu):
    """dwconv_bwd_w_kernel walking two tiles per block: the LDS tile re-used after the barrier, a block whose two tiles
    lie in two utterances (7 tiles per utterance, 2 per block), and a last block that breaks after one tile"""
    total, gy, tpb = dw_bwd_w_geom(B, T, Cc)
    assert tpb >= 2, "the launch no longer walks several tiles per block at this shape: enlarge it"
    if last_short:
        assert total < gy * tpb
    else:
        assert cdiv(T, 64) % tpb != 0 and B > 1
    x, w, b, dy, dw0, db0 = dw_inputs(B, T, Cc, K, glu, 900 + T)
    r = dw_ref(x, w, b, dy, K, glu)
    dw_bwd_w_check(lib, f"dwconv{'_glu' if glu else ''}_bwd_w {B}x{T}x{Cc} K={K} tpb={tpb}", x, dy, r, dw0, db0, B, T, Cc, K, glu)


@pytest.mark.parametrize("T", [1, 5, 64, 65])
def test_dwconv_short_sequences(lib, T):
    """K = 31 with T below the halo (1, 5), exactly one tile (64) and one frame past it (65); C = 65: the second channel
    block has one live lane.  Forward, input gradient and weight gradient, plain and GLU-fused (da in fp32 and bf16)."""
    B, Cc, K = 2, 65, 31
    p = lib.ptr
    L = lib.lib()
    for glu in (False, True):
        x, w, b, dy, dw0, db0 = dw_inputs(B, T, Cc, K, glu, 40 + T)
        r = dw_ref(x, w, b, dy, K, glu)
        xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
        tag = f"dwconv{'_glu' if glu else ''} T={T}"
        if glu:
            rc, y = dw_glu_fwd_call(lib, xd, wd, bd, B, T, Cc, K)
            assert rc == 0
            check("DW_GLU_FWD_TOL", f"{tag} fwd", y, r["y"].reshape(B * T, Cc), r["ys"].reshape(B * T, Cc))
            da32, da16 = nan_(B, T, 2 * Cc), nan_(B, T, 2 * Cc, dtype=torch.bfloat16)
            for da, bf in ((da32, 0), (da16, 1)):
                lib.check(L.eamd_dwconv_glu_bwd_x(p(dyd), p(wd), p(xd), p(da), bf, B, T, Cc, K, lib.stream_ptr()),
                          "eamd_dwconv_glu_bwd_x")
            check("DW_GLU_BWD_X_TOL", f"{tag} bwd_x", da32, r["dx"], r["dxs"])
            assert torch.equal(da16, da32.to(torch.bfloat16)), f"{tag}: bf16 da is not the fp32 da rounded once"
        else:
            y, dx = nan_(B, T, Cc), nan_(B, T, Cc)
            lib.check(L.eamd_dwconv_fwd(p(xd), p(wd), p(bd), p(y), B, T, Cc, K, lib.stream_ptr()), "eamd_dwconv_fwd")
            check("DW_FWD_TOL", f"{tag} fwd", y, r["y"], r["ys"], n_terms=K + 1)
            lib.check(L.eamd_dwconv_bwd_x(p(dyd), p(wd), p(dx), B, T, Cc, K, lib.stream_ptr()), "eamd_dwconv_bwd_x")
            check("DW_BWD_X_TOL", f"{tag} bwd_x", dx, r["dx"], r["dxs"], n_terms=K)
        dw_bwd_w_check(lib, f"{tag} bwd_w", x, dy, r, dw0, db0, B, T, Cc, K, glu)


@pytest.mark.parametrize("K,rc_want", [(33, EUNSUPPORTED), (32, EINVAL), (4, EINVAL)])
def test_dwconv_refused_kernel_sizes(ops, lib, K, rc_want):
    """K above the LDS-tiled kernel's 32 taps is EAMD_EUNSUPPORTED, an even K is EAMD_EINVAL, and nothing is written"""
    B, T, Cc = 2, 20, 64
    g = torch.Generator().manual_seed(K)
    x, a = torch.randn(B, T, Cc, generator=g).to(DEV), torch.randn(B, T, 2 * Cc, generator=g).to(DEV)
    w, b = torch.randn(Cc, K, generator=g).to(DEV), torch.randn(Cc, generator=g).to(DEV)
    p, L, s = lib.ptr, lib.lib(), lib.stream_ptr()
    y, da, dw, db = nan_(B, T, Cc), nan_(B, T, 2 * Cc), nan_(Cc, K), nan_(Cc)
    assert L.eamd_dwconv_fwd(p(x), p(w), p(b), p(y), B, T, Cc, K, s) == rc_want
    assert L.eamd_dwconv_bwd_x(p(x), p(w), p(y), B, T, Cc, K, s) == rc_want
    assert L.eamd_dwconv_bwd_w(p(x), p(x), p(dw), p(db), B, T, Cc, K, s) == rc_want
    assert L.eamd_dwconv_glu_fwd(p(a), p(w), p(b), p(y), None, B, T, Cc, K, s) == rc_want
    assert L.eamd_dwconv_glu_bwd_x(p(x), p(w), p(a), p(da), 0, B, T, Cc, K, s) == rc_want
    assert L.eamd_dwconv_glu_bwd_w(p(x), p(a), p(dw), p(db), B, T, Cc, K, s) == rc_want
    torch.cuda.synchronize()
    for t in (y, da, dw, db):
        assert bool(torch.isnan(t).all())
    if K == 33:
        assert ops.dwconv_glu_fwd(a.view(B * T, 2 * Cc), w, b, B, T, Cc, K) is None
    else:
        with pytest.raises(lib.EamdError):
            ops.dwconv_glu_fwd(a.view(B * T, 2 * Cc), w, b, B, T, Cc, K)
    with pytest.raises(lib.EamdError):
        ops.dwconv_fwd(x, w, b, B, T, Cc, K)
    with pytest.raises(lib.EamdError):
        ops.dwconv_bwd_x(x, w, B, T, Cc, K)
    with pytest.raises(lib.EamdError):
        ops.dwconv_bwd_w(x, x, torch.zeros(Cc, K, device=DEV), torch.zeros(Cc, device=DEV), B, T, Cc, K)
    with pytest.raises(lib.EamdError):
        ops.dwconv_glu_bwd_x(x, w, a, B, T, Cc, K)
    with pytest.raises(lib.EamdError):
        ops.dwconv_glu_bwd_w(x, a, torch.zeros(Cc, K, device=DEV), torch.zeros(Cc, device=DEV), B, T, Cc, K)


# =============================================================================================
# 5. first front-end convolution: stride 2 / pad 0 (eamd_conv1_*) and stride 1 / pad 1 (eamd_conv3x3_c1_*)
# =============================================================================================
C1_FWD_TOL = 7.5e-7   # relu(conv) relative to sum |w| |x| + |bias|; observed 1.90e-7 (a-priori, 10 terms: 1.07e-6)
C1_BWD_W_TOL = 5.5e-7  # dw / db relative to sum_pos |dy| |x| (/ sum |dy|) + |start|; observed 1.40e-7
C1_MAXF = 512         # input row + 2 * pad must fit the LDS row


def c1_fns(lib, st):
    L = lib.lib()
    if st == 2:
        return L.eamd_conv1_fwd, L.eamd_conv1_bwd_w, L.eamd_conv1_bwd_w_workspace, 0
    return L.eamd_conv3x3_c1_fwd, L.eamd_conv3x3_c1_bwd_w, L.eamd_conv3x3_c1_bwd_w_workspace, 1


def c1_hw(T, Fd, st, pad):
    return (T + 2 * pad - 3) // st + 1, (Fd + 2 * pad - 3) // st + 1


def c1_bwd_grid(B, H, Cc):
    """conv_c1_bwd_w_grid: about 2048 blocks -> (grid y, output rows per block)"""
    nrow = B * H
    want = max(1, 2048 // cdiv(Cc, 256))
    rpb = max(1, cdiv(nrow, want))
    return cdiv(nrow, rpb), rpb


def is_pair(t, Cc):
    """the two-channels-per-thread bf16 form: even C and a 4-byte aligned pointer"""
    return t.dtype == torch.bfloat16 and Cc % 2 == 0 and t.data_ptr() % 4 == 0


def bf16_misaligned(shape):
    """a NaN-filled bf16 view that starts one element past a 4-byte boundary"""
    n = math.prod(shape)
    buf = nan_(n + 1, dtype=torch.bfloat16)
    v = buf[1:].view(shape)
    assert v.data_ptr() % 4 == 2
    return v


def c1_fwd_call(lib, st, x, w, b, y, B, T, Fd, Cc):
    fwd = c1_fns(lib, st)[0]
    p = lib.ptr
    return fwd(p(x), p(w), p(b), p(y), B, T, Fd, Cc, int(y.dtype == torch.bfloat16), lib.stream_ptr())


# (stride, B, T, F, C, expected W)
C1_FWD_CASES = [
    (1, 2, 3, 3, 1, 3), (1, 1, 1, 1, 3, 1),                       # smallest legal shapes; H = 1
    (1, 2, 9, 17, 64, 17), (1, 2, 9, 16, 64, 16),                 # W % 8 != 0 and == 0
    (1, 2, 9, 5, 7, 5),                                           # W < 8, odd C: bf16 takes the non-pair form
    (1, 1, 5, 20, 300, 20), (1, 1, 5, 20, 600, 20),               # thread loop's second trip: fp32 C > 256, pairs C/2 > 256
    (1, 1, 3, 510, 4, 510),                                       # F + 2 pad = 512: the LDS row limit
    (2, 2, 3, 3, 1, 1), (2, 2, 9, 17, 64, 8), (2, 2, 9, 16, 64, 7), (2, 2, 9, 5, 7, 2),
    (2, 1, 5, 20, 300, 9), (2, 1, 5, 20, 600, 9), (2, 1, 3, 512, 4, 255),
]


@pytest.mark.parametrize("st,B,T,Fd,Cc,W_want", C1_FWD_CASES)
def test_conv_c1_fwd_vs_float64(lib, st, B, T, Fd, Cc, W_want):
    """relu(conv2d(1 -> C, 3x3)) in NHWC at both strides: fp32 against float64, bf16 = the fp32 result rounded once (pair
    form for even C, non-pair for odd C), and bf16 into a view one element off a 4-byte boundary (non-pair form) equal
    to the aligned result bit for bit"""
    pad = c1_fns(lib, st)[3]
    H, W = c1_hw(T, Fd, st, pad)
    assert W == W_want and Fd + 2 * pad <= C1_MAXF
    g = torch.Generator().manual_seed(1000 * st + Fd + Cc)
    x = torch.randn(B, T, Fd, generator=g)
    w, b = torch.randn(Cc, 1, 3, 3, generator=g), torch.randn(Cc, generator=g)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    ref = torch.relu(F.conv2d(x.double().unsqueeze(1), w.double(), b.double(), stride=st, padding=pad)).permute(0, 2, 3, 1)
    scale = F.conv2d(x.double().abs().unsqueeze(1), w.double().abs(), b.double().abs(), stride=st, padding=pad).permute(0, 2, 3, 1)
    assert ref.shape == (B, H, W, Cc)
    name = f"conv_c1_fwd st={st} {B}x{T}x{Fd}x{Cc}"
    y32 = nan_(B, H, W, Cc)
    assert c1_fwd_call(lib, st, xd, wd, bd, y32, B, T, Fd, Cc) == 0
    check("C1_FWD_TOL", name, y32, ref, scale, n_terms=10)
    y16 = nan_(B, H, W, Cc, dtype=torch.bfloat16)
    assert is_pair(y16, Cc) == (Cc % 2 == 0)
    assert c1_fwd_call(lib, st, xd, wd, bd, y16, B, T, Fd, Cc) == 0
    assert torch.equal(y16, y32.to(torch.bfloat16)), f"{name}: bf16 y is not the fp32 y rounded once"
    if Cc % 2 == 0:
        ym = bf16_misaligned((B, H, W, Cc))
        assert not is_pair(ym, Cc)
        assert c1_fwd_call(lib, st, xd, wd, bd, ym, B, T, Fd, Cc) == 0
        assert torch.equal(ym, y16), f"{name}: the non-pair bf16 form differs from the pair form"


@pytest.mark.parametrize("st", [1, 2])
def test_conv_c1_row_limit_refused(lib, st):
    """an input row one wider than the LDS row is EAMD_EUNSUPPORTED in the forward and the weight gradient; nothing is
    written"""
    fwd, bwd, wsf, pad = c1_fns(lib, st)
    B, T, Cc = 1, 3, 4
    Fd = C1_MAXF - 2 * pad + 1
    H, W = c1_hw(T, Fd, st, pad)
    x, w, b = torch.zeros(B, T, Fd, device=DEV), torch.zeros(Cc, 9, device=DEV), torch.zeros(Cc, device=DEV)
    y, dw, db = nan_(B, H, W, Cc), nan_(Cc, 9), nan_(Cc)
    dy = torch.zeros(B, H, W, Cc, device=DEV)
    ws = nan_(int(wsf(B, T, Cc)))
    p = lib.ptr
    assert fwd(p(x), p(w), p(b), p(y), B, T, Fd, Cc, 0, lib.stream_ptr()) == EUNSUPPORTED
    assert bwd(p(dy), p(x), p(dw), p(db), p(ws), B, T, Fd, Cc, 0, lib.stream_ptr()) == EUNSUPPORTED
    # the two-stage reduction needs its workspace: NULL is refused, at a legal width too
    xs, dys = torch.zeros(B, T, 20, device=DEV), torch.zeros(B, *c1_hw(T, 20, st, pad), Cc, device=DEV)
    assert bwd(p(dys), p(xs), p(dw), p(db), None, B, T, 20, Cc, 0, lib.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    for t in (y, dw, db, ws):
        assert bool(torch.isnan(t).all())


def c1_bwd_w_case(lib, st, B, T, Fd, Cc, modes, seed, want=None):
    """weight / bias gradient of the first convolution for dy in each of `modes` (fp32, bf16, bf16 one element off a
    4-byte boundary): dw / db start non-zero and are called twice; the workspace is NaN-filled with 64 guard floats
    behind it.  With at most two reduction slices the result of a launch into zeroed buffers is reproducible."""
    fwd, bwd, wsf, pad = c1_fns(lib, st)
    H, W = c1_hw(T, Fd, st, pad)
    gy, rpb = c1_bwd_grid(B, H, Cc)
    slices = min(16, cdiv(gy, 32))
    if want:
        got = dict(W=W, gy=gy, rpb=rpb, slices=slices)
        assert {k: got[k] for k in want} == want, f"geometry {got} is not the intended {want}"
    nws = int(wsf(B, T, Cc))
    assert nws == gy * 10 * Cc
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, Fd, generator=g)
    dyf = torch.randn(B, H, W, Cc, generator=g) * (torch.rand(B, H, W, Cc, generator=g) > 0.5)     # ReLU-masked
    dw0, db0 = torch.randn(Cc, 9, generator=g) + 0.5, torch.randn(Cc, generator=g) - 0.5
    cols = F.unfold(x.double().unsqueeze(1), 3, stride=st, padding=pad).transpose(1, 2).reshape(B, H, W, 9)
    xd = x.to(DEV)
    p = lib.ptr
    for mode in modes:
        if mode == "fp32":
            dy = dyf.to(DEV)
        elif mode == "bf16":
            dy = dyf.to(torch.bfloat16).to(DEV)
            assert is_pair(dy, Cc) == (Cc % 2 == 0)
        else:
            dy = bf16_misaligned((B, H, W, Cc))
            dy.copy_(dyf.to(torch.bfloat16))
            assert not is_pair(dy, Cc)
        d64 = dy.double().cpu()
        dwr, dws = torch.einsum("bhwc,bhwk->ck", d64, cols), torch.einsum("bhwc,bhwk->ck", d64.abs(), cols.abs())
        dbr, dbs = d64.sum((0, 1, 2)), d64.abs().sum((0, 1, 2))
        name = f"conv_c1_bwd_w st={st} {B}x{T}x{Fd}x{Cc} {mode} W={W} gy={gy} rpb={rpb}"

        def launch(dw, db):
            ws = nan_(nws + 64)
            assert bwd(p(dy), p(xd), p(dw), p(db), p(ws), B, T, Fd, Cc, int(dy.dtype == torch.bfloat16), lib.stream_ptr()) == 0
            assert bool(torch.isnan(ws[nws:]).all()), f"{name}: wrote past the workspace"
            assert not bool(torch.isnan(ws[:nws]).any()), f"{name}: a partial sum was never written"

        dw, db = dw0.to(DEV), db0.to(DEV)
        for ncall in (1, 2):
            launch(dw, db)
            check("C1_BWD_W_TOL", f"{name} dw x{ncall}", dw, dw0.double() + ncall * dwr, dw0.double().abs() + ncall * dws,
                  n_terms=B * H * W)
            check("C1_BWD_W_TOL", f"{name} db x{ncall}", db, db0.double() + ncall * dbr, db0.double().abs() + ncall * dbs,
                  n_terms=B * H * W)
        if slices <= 2:
            outs = []
            for _ in range(2):
                dwz, dbz = torch.zeros(Cc, 9, device=DEV), torch.zeros(Cc, device=DEV)
                launch(dwz, dbz)
                outs.append((dwz, dbz))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), f"{name}: not reproducible"


# (W, C): W = 5 below one trip of eight; 24 / 25 around the pair form's 24 positions per request, 40 / 41 around the
# non-pair form's 40, 49 a third trip of the pair form; C = 7 odd, 300 > 256 (two channel blocks in fp32), 600: 300
# pairs > 256 (two channel blocks of pairs)
C1_BWD_WC = [(5, 7), (24, 64), (25, 64), (40, 300), (41, 64), (49, 600)]


@pytest.mark.parametrize("W,Cc", C1_BWD_WC)
@pytest.mark.parametrize("st", [1, 2])
def test_conv_c1_bwd_w_vs_float64(lib, st, W, Cc):
    Fd = W if st == 1 else 2 * W + 1
    c1_bwd_w_case(lib, st, 2, 9, Fd, Cc, ("fp32", "bf16", "bf16_misaligned"), 2000 * st + W, want=dict(W=W, rpb=1, slices=1))


def test_conv_c1_bwd_w_rows_per_block(lib):
    """stride 1 with 2100 output rows: two rows per block (the staged input rows are replaced between them)"""
    c1_bwd_w_case(lib, 1, 3, 700, 12, 8, ("fp32", "bf16"), 77, want=dict(rpb=2, gy=1050, slices=16))


@pytest.mark.parametrize("st,B,T,gy", [(1, 1, 1, 1), (1, 1, 3, 3), (2, 1, 3, 1), (2, 3, 4, 3), (1, 4, 9, 36), (2, 9, 9, 36)])
def test_conv_c1_bwd_w_few_row_blocks(lib, st, B, T, gy):
    """1 and 3 row blocks: reduce subgroups that have no partial row; 36 row blocks: two reduction slices, whose two
    atomic adds into a zeroed buffer commute"""
    c1_bwd_w_case(lib, st, B, T, 19, 64, ("fp32", "bf16"), 300 + 10 * st + gy, want=dict(gy=gy, rpb=1, slices=2 if gy > 32 else 1))
