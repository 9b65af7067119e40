"""Element-wise, dropout and optimizer kernels (csrc/elementwise.hip, csrc/optim.hip) on every dispatch path: the x2 dword
forms against the scalar forms, float4 bodies with scalar tails, the 2048-block grid cap with its grid-stride second
trip, strided column blocks, offset (misaligned) views, accumulating outputs.

The reference is plain torch / numpy in float64 on the CPU from the same fp32 or bf16 input values; the dropout mask and the
gradient noise are judged against tests/dropout_restatement.py (whose statistics tests/test_dropout_restatement.py checks
on the CPU), bit for bit.  Every comparison is element-wise and prints the worst element's index.  Output buffers are
filled with NaN (0x7FC0 for bf16) before the launch; every output that is a strided column block or shorter than its
allocation has guard elements that must come back bit-identical; accumulating outputs start from non-zero values and
are called twice.  Each case recomputes the host dispatcher's predicate from the actual data_ptr(), n, ld and parity and
asserts the intended branch; misalignment comes from offset views of live allocations only.

Each bound is a named constant.  The kernels that only add and multiply must also sit under the a-priori bound
(n_terms + 8) * 2^-24 of the sum of the absolute values of the terms; a bf16 output must be the round-to-nearest-even of
some fp32 value within the bound.  Each constant is at most 4x the largest error observed under its name on an MI355X,
noted beside it; every check prints its observed error in an "[elementwise] <constant> <case>" line."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_restatement as dr


pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
INF = float("inf")
U24 = 2.0 ** -24
EINVAL, EUNSUPPORTED = -1, -2
GRID_CAP = 2048 * 256          # threads of grid_for's 2048 blocks of 256
BF16, F32 = torch.bfloat16, torch.float32


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


def cdiv(a, b):
    return -(-a // b)


def grid_for(n_threads_needed):
    """grid_for of elementwise.hip"""
    return min(max(cdiv(n_threads_needed, 256), 1), 2048)


def past_cap(n_threads_needed):
    return n_threads_needed > GRID_CAP


def aligned(nbytes, *ts):
    """every tensor's (view's) address is a multiple of nbytes; None counts as NULL"""
    return all(t is None or t.data_ptr() % nbytes == 0 for t in ts)


def nan_buf(n, dtype=F32):
    """NaN-filled flat device buffer (bf16: the 0x7FC0 pattern)"""
    if dtype == BF16:
        return torch.full((n,), 0x7FC0, dtype=torch.int16, device=DEV).view(BF16)
    return torch.full((n,), NAN, device=DEV, dtype=dtype)


def ibits(t):
    """the bit patterns of an fp32 / bf16 tensor, on the CPU"""
    t = t.detach().contiguous().cpu()
    return t.view({F32: torch.int32, BF16: torch.int16}[t.dtype])


def assert_guards(name, buf, written):
    """the elements of the NaN-filled buffer outside `written` (bool, buf's shape, CPU) still hold the fill pattern"""
    b = ibits(buf).reshape(-1)
    pat = 0x7FC0 if buf.dtype == BF16 else 0x7FC00000
    bad = (~written.reshape(-1)) & (b != pat)
    assert not bool(bad.any()), f"{name}: guard element {int(bad.nonzero()[0])} was overwritten"


def block_mask(total, off, rows, cols, ld):
    """bool[total]: the elements off + r * ld + c, r < rows, c < cols"""
    m = torch.zeros(total, dtype=torch.bool)
    idx = off + (torch.arange(rows).unsqueeze(1) * ld + torch.arange(cols).unsqueeze(0)).reshape(-1)
    m[idx] = True
    return m


def block_of(buf, off, rows, cols, ld):
    """the [rows, cols] block at off with row stride ld of a flat buffer (CPU copy)"""
    return torch.as_strided(buf.detach().cpu(), (rows, cols), (ld, 1), off).clone()


def unravel(i, shape):
    idx = []
    for n in reversed(shape):
        idx.insert(0, i % n)
        i //= n
    return tuple(idx)


def assert_bits(name, got, ref):
    """bit equality of two fp32 / bf16 tensors, with the first differing element's index"""
    g, r = ibits(got).reshape(-1), ibits(ref).reshape(-1)
    assert g.shape == r.shape, f"{name}: {g.shape} vs {r.shape}"
    bad = g != r
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {g.numel()} elements differ, first at {unravel(i, tuple(ref.shape))}: "
                             f"got 0x{int(g[i]) & 0xffffffff:x}, expected 0x{int(r[i]) & 0xffffffff:x}")


def check(tolname, name, got, ref, scale, n_terms=None, keep=None, either=None):
    """max over elements of |got - ref| / scale (scale broadcast against ref), in float64, with the worst element's
    index.  keep: elements left out of the comparison where False; either: a second reference, an element passes with the
    smaller of its two errors (a derivative at a kink).  Where the reference is NaN or infinite the result must be NaN /
    the same infinity; any other NaN (an unwritten element) is an infinite error.  n_terms: also assert the a-priori bound."""
    tol = globals()[tolname]
    g = got.detach().double().cpu().reshape(ref.shape)
    r = ref.detach().double()
    special = torch.isnan(r) | torch.isinf(r)
    if bool(special.any()):
        same = torch.where(torch.isnan(r), torch.isnan(g), g == r)
        bad = special & ~same
        assert not bool(bad.any()), f"{name}: element {unravel(int(bad.reshape(-1).nonzero()[0]), tuple(ref.shape))} is not the reference's NaN / infinity"
        g, r = torch.where(special, torch.zeros_like(g), g), torch.where(special, torch.zeros_like(r), r)
    d = (g - r).abs()
    if either is not None:
        d = torch.minimum(d, (g - torch.where(special, torch.zeros_like(r), either.detach().double())).abs())
    d = torch.where(torch.isnan(d), torch.full_like(d, INF), d)
    if keep is not None:
        d = torch.where(keep, d, torch.zeros_like(d))
    s = scale.detach().double().expand_as(d)
    e = torch.where(d == 0, torch.zeros_like(d), d / s).reshape(-1)
    i = int(e.argmax()) if e.numel() else 0
    worst = float(e[i]) if e.numel() else 0.0
    idx = unravel(i, tuple(ref.shape))
    extra = "" if n_terms is None else f", a-priori {apriori(n_terms):.3g}"
    print(f"[elementwise] {tolname} {name}: max err/scale {worst:.3e} at {idx} (tol {tol:g}{extra})")
    assert worst <= tol, f"{name}: element {idx} error/scale {worst:.3e} > {tolname} = {tol:g}"
    if n_terms is not None:
        assert worst <= apriori(n_terms), f"{name}: {worst:.3e} above the a-priori bound of {n_terms} terms"
    return worst


def rne_bf16(x64):
    """float64 -> bf16 by round-to-nearest-even (through fp32: both roundings are monotonic)"""
    return x64.float().to(BF16)


def check_bf16(tolname, name, got, ref, scale, n_terms=None):
    """a bf16 output is the RNE rounding of an fp32 value within the bound of the float64 reference: by monotonicity it lies
    between RNE(ref - bound * scale) and RNE(ref + bound * scale), which is exact wherever the reference is not within the
    bound of a tie and one bf16 ulp otherwise.  bound = the named constant, and the a-priori bound where n_terms is given."""
    tol = globals()[tolname]
    bound = tol if n_terms is None else min(tol, apriori(n_terms))
    assert got.dtype == BF16
    g = got.detach().double().cpu().reshape(ref.shape)
    r = ref.detach().double()
    s = scale.detach().double().expand_as(r)
    lo, hi = rne_bf16(r - bound * s).double(), rne_bf16(r + bound * s).double()
    bad = ~((g >= lo) & (g <= hi))
    e = torch.where(bad, (g - r).abs() / s, torch.zeros_like(r)).reshape(-1)
    inexact = int((lo != hi).sum())
    seen = torch.where(torch.isnan(g), torch.full_like(r, INF), (g - r).abs() / s)
    print(f"[elementwise] {tolname} {name}: bf16 RNE interval at bound {bound:.3g}: {int(bad.sum())} of {r.numel()} outside, "
          f"{inexact} near a tie (either neighbour); with the bf16 rounding |got - ref| / scale <= {float(seen.max()):.3e}")
    if bool(bad.any()):
        i = int(e.argmax())
        idx = unravel(i, tuple(ref.shape))
        raise AssertionError(f"{name}: element {idx} = {float(g.reshape(-1)[i])!r} is not the bf16 rounding of an fp32 value "
                             f"within {bound:.3g} * scale of {float(r.reshape(-1)[i])!r}")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def stream(lib):
    return lib.stream_ptr()


# =============================================================================================
# 1. fp32 -> bf16 cast: bit equality
# =============================================================================================
CAST_SIZES = [1, 7, 8, 9, 4103, 8 * 2048 * 256 + 8 * 256 + 5]


def cast_specials():
    """every exact tie 0x????8000 of a block of mantissas (even and odd bf16 neighbours) at several exponents and both
    signs, +-0, +-inf, the largest finite fp32 (rounds to inf), just below / above a tie, NaN"""
    bits = []
    for sign in (0, 1):
        for e in (1, 100, 127, 128, 254):
            for m in range(128):
                bits.append((sign << 31) | (e << 23) | (m << 16) | 0x8000)
        for e in (100, 127):
            for m in (0, 1, 126, 127):
                bits += [(sign << 31) | (e << 23) | (m << 16) | 0x7fff, (sign << 31) | (e << 23) | (m << 16) | 0x8001]
        bits += [sign << 31, (sign << 31) | 0x7f800000, (sign << 31) | 0x7f7fffff, (sign << 31) | 0x7f7f8000,
                 (sign << 31) | 0x7f7f7fff]
    bits += [0x7fc00000, 0xffc00001, 0x7f800001]
    a = np.array(bits, dtype=np.uint32).view(np.int32)
    return torch.from_numpy(a.copy()).view(F32)


def cast_input(n, seed):
    g = gen(seed)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 31, (n,), generator=g).float())
    sp = cast_specials()
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n >= 2 * sp.numel():                     # the scalar tail of the 8-wide body sees them too
        x[n - sp.numel():] = sp
    return x


@pytest.mark.parametrize("path", ["vec", "scalar"])
@pytest.mark.parametrize("n", CAST_SIZES)
def test_cast_bf16_bits(lib, n, path):
    """eamd_cast_bf16 == x.to(bfloat16) on the CPU, bit for bit (a NaN stays a NaN); vec: the 8-wide uint4 body, its
    grid-stride second trip and the scalar tail; scalar: the same through an input view offset by one element"""
    x = cast_input(n, 40 + n % 97)
    off = 0 if path == "vec" else 1
    xb = torch.zeros(n + 1, device=DEV)
    xd = xb[off:off + n]
    xd.copy_(x)
    yb = nan_buf(n + 8, BF16)
    vec = aligned(16, xd, yb)
    assert vec == (path == "vec")
    n8 = n // 8 if vec else 0
    if n == CAST_SIZES[-1]:
        assert past_cap(n // 8 + 1 if vec else n) and (not vec or (n8 > GRID_CAP and n - 8 * n8 == 5))
    rc = lib.lib().eamd_cast_bf16(lib.ptr(xd), lib.ptr(yb), n, stream(lib))
    assert rc == 0
    ref = x.to(BF16)
    nanx = torch.isnan(x)
    got = yb[:n].cpu()
    assert bool(torch.isnan(got.float())[nanx].all()), "a NaN did not stay a NaN"
    assert_bits(f"cast_bf16 {path} n={n}", torch.where(nanx, ref, got), ref)
    assert_guards("cast_bf16", yb, torch.arange(n + 8) < n)


def test_cast_bf16_denormals(lib):
    """fp32 denormals: the result must be the RNE value or a zero of the same sign; the count of each is printed.  On the MI355X
    every one of the 4104 comes back as the RNE value (bf16 denormals included): the conversion does not flush."""
    m = torch.cat([torch.arange(1, 1 << 23, 4099, dtype=torch.int32), torch.tensor([1, 0x8000, 0x18000, 0x7fffff, 0x7f8000],
                                                                               dtype=torch.int32)])
    xi = torch.cat([m, m | torch.tensor(-0x80000000, dtype=torch.int32)])
    x = xi.view(F32)
    n = x.numel()
    yb = nan_buf(n + 8, BF16)
    xd = x.to(DEV)
    assert lib.lib().eamd_cast_bf16(lib.ptr(xd), lib.ptr(yb), n, stream(lib)) == 0
    got = ibits(yb[:n]).int() & 0xffff
    # RNE on the bit pattern (exact for denormals: same exponent field, 16 mantissa bits dropped)
    u = xi.long() & 0xffffffff
    rne = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).int() & 0xffff
    zero = ((u >> 16) & 0x8000).int()
    is_rne, is_zero = got == rne, got == zero
    print(f"[elementwise] cast_bf16 denormals: {int(is_rne.sum())} of {n} RNE, {int((is_zero & ~is_rne).sum())} flushed to a signed zero")
    bad = ~(is_rne | is_zero)
    assert not bool(bad.any()), f"denormal 0x{int(u[bad][0]):08x} -> 0x{int(got[bad][0]):04x}: neither RNE nor a signed zero"
    assert_guards("cast_bf16 denormals", yb, torch.arange(n + 8) < n)


# =============================================================================================
# 2. pure copies / zeroing: bit equality against index arithmetic
# =============================================================================================
def rand_bits(shape, dtype, seed):
    """arbitrary bit patterns (NaNs and infinities included): a copy has to carry them all"""
    if dtype == BF16:
        return torch.randint(-32768, 32768, shape, generator=gen(seed), dtype=torch.int16).view(BF16)
    return torch.randint(-2 ** 31, 2 ** 31, shape, generator=gen(seed), dtype=torch.int64).int().view(F32)


@pytest.mark.parametrize("rows,D", [(1, 1), (7, 5), (300, 257), (2100, 256)])
def test_mask_rows_bits(lib, rows, D):
    """y[r] = keep[r] ? x[r] : +0 (also where x is inf or NaN); the last shape runs the grid-stride second trip"""
    assert past_cap(rows * D) == (rows == 2100)
    x = rand_bits((rows, D), F32, rows + D)
    keep = (torch.rand(rows, generator=gen(rows)) < 0.6).to(torch.uint8)
    if rows > 1:
        keep[0], keep[-1] = 0, 1
    yb = nan_buf(rows * D + 8)
    xd, kd = x.to(DEV), keep.to(DEV)
    rc = lib.lib().eamd_mask_rows(lib.ptr(xd), lib.ptr(kd), lib.ptr(yb), rows, D, stream(lib))
    assert rc == 0
    ref = torch.where(keep.bool().unsqueeze(1), x.view(torch.int32), torch.zeros((), dtype=torch.int32)).view(F32)
    assert_bits(f"mask_rows {rows}x{D}", yb[:rows * D].view(rows, D), ref)
    assert_guards("mask_rows", yb, torch.arange(rows * D + 8) < rows * D)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,T,C", [(3, 7, 5), (4, 300, 450)])
def test_mask_time_bits(lib, B, T, C, dtype):
    """rows with time index >= bound[0] zeroed in place, everything else bit-identical; bound 0, a middle value, T"""
    rows = B * T
    assert past_cap(rows * C) == (T == 300)
    x = rand_bits((B, T, C), dtype, B + T + C)
    for bound in (0, T // 2 + 1, T):
        xb = nan_buf(rows * C + 8, dtype)
        xb[:rows * C].copy_(x.reshape(-1))
        bd = torch.tensor([bound], dtype=torch.int32, device=DEV)
        rc = lib.lib().eamd_mask_time(lib.ptr(xb), rows, C, T, lib.ptr(bd), 1 if dtype == BF16 else 0, stream(lib))
        assert rc == 0
        ref = ibits(x).clone()
        ref[:, bound:, :] = 0
        assert_bits(f"mask_time {dtype} bound={bound}", xb[:rows * C].view(B, T, C), ref.view(dtype))
        assert_guards("mask_time", xb, torch.arange(rows * C + 8) < rows * C)


UNFOLD_SHAPES = [(2, 5, 6, 3), (1, 1, 4, 5), (3, 37, 10, 31), (2, 700, 64, 7)]


def unfold_ref(xi, k):
    """col[b, t, kk, c] = x[b, t + kk - p, c], 0 outside the sequence; on integer bit patterns"""
    p = (k - 1) // 2
    T = xi.shape[1]
    xp = F.pad(xi, (0, 0, p, p))
    return torch.stack([xp[:, kk:kk + T] for kk in range(k)], dim=2)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,T,C,k", UNFOLD_SHAPES)
def test_unfold1d_bits(lib, B, T, C, k, dtype):
    """im2col along time; T < (k - 1) / 2 (every tap but the centre outside), and past the grid cap in fp32"""
    CW = C // 2 if dtype == BF16 else C
    n_words = B * T * k * CW
    assert past_cap(n_words) == ((B, T, C, k) == UNFOLD_SHAPES[-1] and dtype == F32)
    assert any(t < (kk - 1) // 2 for _, t, _, kk in UNFOLD_SHAPES)
    x = rand_bits((B, T, C), dtype, B * T + C + k)
    n = B * T * k * C
    colb = nan_buf(n + 8, dtype)
    xd = x.to(DEV)
    assert aligned(4, xd, colb)
    rc = lib.lib().eamd_unfold1d(lib.ptr(xd), lib.ptr(colb), B, T, C, k, 1 if dtype == BF16 else 0, stream(lib))
    assert rc == 0
    ref = unfold_ref(ibits(x), k).view(dtype)
    assert_bits(f"unfold1d {dtype} {(B, T, C, k)}", colb[:n].view(B, T, k, C), ref)
    assert_guards("unfold1d", colb, torch.arange(n + 8) < n)


def test_unfold_fold_refusals(lib):
    """even k -> EINVAL (both entry points); bf16 with odd C -> EUNSUPPORTED; nothing is launched"""
    L, p = lib.lib(), lib.ptr
    x, col = torch.zeros(2 * 5 * 6, device=DEV), nan_buf(2 * 5 * 6 * 4)
    assert L.eamd_unfold1d(p(x), p(col), 2, 5, 6, 4, 0, stream(lib)) == EINVAL
    assert L.eamd_fold1d(p(col), p(x), 2, 5, 6, 4, stream(lib)) == EINVAL
    x16, col16 = torch.zeros(2 * 5 * 5, device=DEV, dtype=BF16), nan_buf(2 * 5 * 5 * 3, BF16)
    assert L.eamd_unfold1d(p(x16), p(col16), 2, 5, 5, 3, 1, stream(lib)) == EUNSUPPORTED
    assert_guards("refused unfold1d", col, torch.zeros(col.numel(), dtype=torch.bool))
    assert_guards("refused unfold1d", col16, torch.zeros(col16.numel(), dtype=torch.bool))


def conv_weight_strides(d0, d1, d2, d3):
    """the two destination stride sets of the implicit-GEMM conv weight layouts (functional.py: [Co][Ci][kh][kw] ->
    [tap][ci][co] and [tap][co][ci], tap = kh * kw_n + kw)"""
    return {"tap_ci_co": (1, d0, d3 * d0 * d1, d0 * d1), "tap_co_ci": (d1, 1, d3 * d0 * d1, d0 * d1)}


def permute_index(dims, strides):
    d0, d1, d2, d3 = dims
    i0, i1, i2, i3 = torch.meshgrid(*(torch.arange(d) for d in dims), indexing="ij")
    return (i0 * strides[0] + i1 * strides[1] + i2 * strides[2] + i3 * strides[3]).reshape(-1)


@pytest.mark.parametrize("layout", ["tap_ci_co", "tap_co_ci"])
@pytest.mark.parametrize("dims", [(3, 5, 2, 7), (64, 33, 3, 3)])
def test_permute4_bits(ops, dims, layout):
    """plain: dst[perm(i)] = src[i] bit for bit; accumulate: twice onto a non-zero dst = (dst0 + src) + src in fp32"""
    strides = conv_weight_strides(*dims)[layout]
    n = math.prod(dims)
    o = permute_index(dims, strides)
    assert sorted(o.tolist()) == list(range(n))                     # a bijection: every address inside dst
    src = rand_bits(dims, F32, n)
    dst = nan_buf(n + 8)
    ops.permute4(src.to(DEV), dst, dims, strides)
    ref = torch.empty(n, dtype=torch.int32)
    ref[o] = ibits(src).reshape(-1)
    assert_bits(f"permute4 {dims} {layout}", dst[:n], ref.view(F32))
    assert_guards("permute4", dst, torch.arange(n + 8) < n)
    g = gen(n)
    srcf, dst0 = torch.randn(dims, generator=g), torch.randn(n + 8, generator=g)
    dsta = dst0.to(DEV)
    for _ in range(2):
        ops.permute4(srcf.to(DEV), dsta, dims, strides, accumulate=True)
    refa = dst0.clone()
    perm = torch.empty(n)
    perm[o] = srcf.reshape(-1)
    refa[:n] = (dst0[:n] + perm) + perm
    assert_bits(f"permute4 accumulate {dims} {layout}", dsta, refa)


# =============================================================================================
# 3. dropout: the mask is the restatement's, bit for bit
# =============================================================================================
DROP_PS = [0.1, 0.5, 3 / 65536, 0.99999]
DROP_SALTS = [11, 2 ** 40 + 3]
DROP_STEPS = [0, 5, 2 ** 33]
DROP_COMBOS = [(p, sa, st) for p in DROP_PS for sa in DROP_SALTS for st in DROP_STEPS]
# at the second-trip sizes: every p, both salts and every step once
DROP_DIAGONAL = [(0.1, 11, 0), (0.5, 2 ** 40 + 3, 5), (3 / 65536, 11, 2 ** 33), (0.99999, 2 ** 40 + 3, 2 ** 33)]
DROP_VEC4_TRIP2 = 4 * 2048 * 256 + 4 * 256 * 3
DROP_SCALAR_TRIP2 = 2048 * 256 + 777
# name: (input dtype, output dtype, element offset of the views, sizes)
DROP_PATHS = {
    "vec4_f32_f32": (F32, F32, 0, (1024, DROP_VEC4_TRIP2)),
    "vec4_bf16_bf16": (BF16, BF16, 0, (1024, DROP_VEC4_TRIP2)),
    "vec4_f32_bf16": (F32, BF16, 0, (1024, DROP_VEC4_TRIP2)),
    "vec4_bf16_f32": (BF16, F32, 0, (1024, DROP_VEC4_TRIP2)),
    "scalar_n_mod_4": (F32, F32, 0, (5, DROP_SCALAR_TRIP2)),
    "scalar_offset_view": (F32, F32, 1, (5, 1024, DROP_SCALAR_TRIP2 - 1)),
}


@functools.lru_cache(maxsize=None)
def drop_bits(step, salt, n):
    return dr.keep_bits(step, salt, n)


def drop_keep(step, salt, n, p):
    return torch.from_numpy(drop_bits(step, salt, n) >= np.uint32(dr.drop_thr16(p)))


def drop_call(lib, xd, yd, n, p, step, salt, act=0):
    """eamd_dropout on (views of) device buffers with a step counter of its own; returns the branch taken (vec4?)"""
    st = torch.tensor([step], dtype=torch.int64, device=DEV)
    vec4 = n % 4 == 0 and aligned(16, xd, yd)
    rc = lib.lib().eamd_dropout(lib.ptr(xd), lib.ptr(yd), n, p, lib.ptr(st), salt, act, 1 if xd.dtype == BF16 else 0,
                                1 if yd.dtype == BF16 else 0, stream(lib))
    assert rc == 0
    return vec4


def drop_buffers(x, off, out_dtype):
    """device input view at element offset `off`, NaN-filled output buffer and its view at the same offset"""
    n = x.numel()
    xb = torch.zeros(n + off, device=DEV, dtype=x.dtype)
    xb[off:].copy_(x)
    yb = nan_buf(n + off + 8, out_dtype)
    return xb[off:], yb, yb[off:off + n], (torch.arange(n + off + 8) >= off) & (torch.arange(n + off + 8) < off + n)


@pytest.mark.parametrize("path", list(DROP_PATHS))
def test_dropout_mask_and_scale(lib, path):
    """kept positions == keep_mask(...) and survivors == fp32(x * inv) (then RNE for a bf16 output), inv = 65536 / (65536 - thr)
    in fp32: all 24 (p, salt, step) at the small sizes, the diagonal at the grid-stride second trip.  In the offset-view
    case the mask index is the view's logical index."""
    in_dt, out_dt, off, sizes = DROP_PATHS[path]
    for n in sizes:
        big = n > 4096
        if big:
            assert past_cap(n // 4 if path.startswith("vec4") else n)
        x = (torch.randn(n, generator=gen(n)) + 0.01).to(in_dt)      # bf16 input: the bf16 values are the input
        x32 = x.float()
        xd, yb, yd, written = drop_buffers(x, off, out_dt)
        for p, salt, step in (DROP_DIAGONAL if big else DROP_COMBOS):
            yb.copy_(nan_buf(yb.numel(), out_dt))
            vec4 = drop_call(lib, xd, yd, n, p, step, salt)
            assert vec4 == path.startswith("vec4"), f"{path} n={n}: wrong branch"
            keep = drop_keep(step, salt, n, p)
            inv = torch.tensor(float(dr.drop_inv(dr.drop_thr16(p))), dtype=F32)
            ref = torch.where(keep, x32 * inv, torch.zeros(())).to(out_dt)      # one fp32 product, RNE for bf16
            name = f"dropout {path} n={n} p={p:g} salt={salt} step={step}"
            got = yd.cpu()
            assert torch.equal(got != 0, keep), f"{name}: kept set differs from the restatement"
            assert_bits(name, got, ref)
            assert_guards(name, yb, written)


@pytest.mark.parametrize("path", list(DROP_PATHS))
def test_dropout_p0_identity(lib, path):
    in_dt, out_dt, off, sizes = DROP_PATHS[path]
    n = sizes[0]
    x = torch.randn(n, generator=gen(3)).to(in_dt)
    x[0], x[-1] = -0.0, INF
    xd, yb, yd, written = drop_buffers(x, off, out_dt)
    assert drop_call(lib, xd, yd, n, 0.0, 5, 11) == path.startswith("vec4")
    assert_bits(f"dropout p=0 {path}", yd, x.float().to(out_dt))
    assert_guards("dropout p=0", yb, written)


def test_dropout_rng_advance(ops):
    """eamd_rng_advance takes the device counter k -> k + 1 and the next mask is the restatement's at k + 1"""
    dev = torch.zeros(1, device=DEV).device          # the device tensors report (the counter is kept per torch.device)
    st = ops.rng_state(dev)
    saved = int(st)
    try:
        k, n, p, salt = 41, 1024, 0.3, 17
        ops.manual_seed(k, dev)
        x = torch.randn(n, generator=gen(9)) + 3.0
        y0 = ops.dropout(x.to(DEV), p, salt).cpu()
        ops.rng_advance(dev)
        assert ops.rng_state(dev) is st and int(st) == k + 1
        y1 = ops.dropout(x.to(DEV), p, salt).cpu()
        assert torch.equal(y0 != 0, drop_keep(k, salt, n, p)) and torch.equal(y1 != 0, drop_keep(k + 1, salt, n, p))
        assert not torch.equal(y0 != 0, y1 != 0)
    finally:
        st.fill_(saved)


# =============================================================================================
# 4. embedding + positional encoding
# =============================================================================================
EMBED_TOL = 2.3e-07       # table[tok] * scale + pe, relative to |table * scale| + |pe|; observed 5.96e-8


@pytest.mark.parametrize("U,D", [(1, 16), (5, 16), (1, 256), (5, 256)])
def test_embed_pe_vs_float64(ops, U, D):
    """table[tok] * scale + pe[r % U + pos_offset (+ pos_dev)]: within one rounding of the product and of the sum; pe = None
    is the fp32 product bit for bit; a strided token column ([n, 1] of an [n, 5] buffer); rows past the grid cap"""
    g = gen(U * 1000 + D)
    V, scale = 23, math.sqrt(D)
    table, pe = torch.randn(V, D, generator=g), torch.randn(U + 6, D, generator=g)
    for B in (3, cdiv(GRID_CAP // D + 1, U)):
        rows = B * U
        assert past_cap(rows * D) == (B != 3)
        tok = torch.randint(0, V, (rows,), generator=g)
        t64 = table.double()[tok] * float(np.float32(scale))
        pos_dev = torch.tensor([2], dtype=torch.int32, device=DEV)
        wide = torch.randint(0, V, (rows, 5), generator=g)
        wide[:, 2] = tok
        col = wide.to(DEV)[:, 2:3]
        assert rows == 1 or (not col.is_contiguous() and col.stride(0) == 5)
        for name, kw, shift, tk in (("plain", {}, 0, tok.to(DEV)), ("pos_offset=3", dict(pos_offset=3), 3, tok.to(DEV)),
                                    ("pos_dev", dict(pos_offset=1, pos_dev=pos_dev), 3, tok.to(DEV)),
                                    ("strided tokens", dict(pos_offset=3), 3, col)):
            out = ops.embed_pe(tk, table.to(DEV), pe.to(DEV), U, scale, **kw)
            pos = torch.arange(rows) % U + shift
            ref = t64 + pe.double()[pos]
            check("EMBED_TOL", f"embed_pe U={U} D={D} rows={rows} {name}", out, ref, t64.abs() + pe.double()[pos].abs(), n_terms=2)
        out = ops.embed_pe(tok.to(DEV), table.to(DEV), None, U, scale)
        assert_bits(f"embed_pe pe=None U={U} D={D} rows={rows}", out, table[tok] * torch.tensor(scale, dtype=F32))


EMBED_BWD_TOL = 8.4e-07   # dtable += scale * sum of dout rows, relative to |dtable0| + sum |terms|; observed 2.42e-7


@pytest.mark.parametrize("V,rows,D", [(11, 40, 16), (50, 2100, 256)])
def test_embed_bwd_vs_float64(ops, V, rows, D):
    """repeated tokens, pad_idx among them: the padded row and the rows of unused tokens stay bit-identical; accumulates
    onto non-zero values, called twice; the second shape runs the grid-stride second trip"""
    assert past_cap(rows * D) == (rows == 2100)
    g = gen(V + rows)
    pad, unused = 3, 7
    tok = torch.randint(0, V, (rows,), generator=g)
    tok[tok == unused] = 0
    tok[::5] = pad
    dout, dt0 = torch.randn(rows, D, generator=g), torch.randn(V + 1, D, generator=g)
    dtable, scale = dt0.to(DEV), 1.7
    for _ in range(2):
        ops.embed_bwd(tok.to(DEV), dout.to(DEV), dtable, scale, pad_idx=pad)
    s32 = float(np.float32(scale))
    live = tok != pad
    ref, mag = dt0.double().clone(), dt0.double().abs()
    ref.index_add_(0, tok[live], 2 * s32 * dout.double()[live])
    mag.index_add_(0, tok[live], 2 * s32 * dout.double()[live].abs())
    count = int(torch.bincount(tok[live], minlength=V).max())
    check("EMBED_BWD_TOL", f"embed_bwd V={V} rows={rows} D={D}", dtable, ref, mag, n_terms=2 * count + 1)
    for r in (pad, unused, V):
        assert_bits(f"embed_bwd untouched row {r}", dtable[r], dt0[r])
    # no padding index: pad_idx = -1 matches no token
    dtable2 = dt0.to(DEV)
    ops.embed_bwd(tok.to(DEV), dout.to(DEV), dtable2, scale)
    ref2 = dt0.double().clone()
    ref2.index_add_(0, tok, s32 * dout.double())
    mag2 = dt0.double().abs().index_add_(0, tok, s32 * dout.double().abs())
    check("EMBED_BWD_TOL", f"embed_bwd no pad V={V} rows={rows}", dtable2, ref2, mag2, n_terms=int(torch.bincount(tok).max()) + 1)


# =============================================================================================
# 5. add / multiply kernels
# =============================================================================================
AXPBY_TOL = 4.5e-07       # a x + b y, relative to |a x| + |b y|; observed 1.14e-7
SCALE_DEV_TOL = 2.8e-07   # (scale * extra) * x, relative; observed 7.04e-8
ADD_TOL = 2.3e-07         # one fp32 addition (add_block_f32, add_bias2, add_colsum2 out), relative to |a| + |b|; observed 5.96e-8
COLSUM_TOL = 6.6e-07      # column sums (colsum, add_cast_colsum2 sums), relative to |out0| + sum |terms|; observed 1.67e-7
POSENC_TOL = 4.1e-07      # x scale + alpha pe, relative to |x scale| + |alpha pe|; observed 1.04e-7
POSENC_BWD_TOL = 1.1e-07  # dalpha, relative to |dalpha0| + sum |dout pe|; observed 2.95e-8
FOLD_TOL = 6.9e-07        # fold1d: a sum of at most k terms, relative to the sum of their moduli; observed 1.74e-7

AXPBY_SIZES = [1, 3, 1001, 4 * 2048 * 256 + 4 * 256 + 3]


@pytest.mark.parametrize("views", ["aligned", "offset", "y_offset", "y_none", "y_none_offset"])
@pytest.mark.parametrize("n", AXPBY_SIZES)
def test_axpby_vs_float64(lib, n, views):
    """float4 body + scalar tail where x, y and out are 16-byte aligned (y = NULL counts as aligned), the scalar loop alone
    from offset views; the last size runs the second grid-stride trip of both"""
    g = gen(n)
    a, b = 0.37, -1.9
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ox = 1 if views in ("offset", "y_none_offset") else 0
    oy = 1 if views in ("offset", "y_offset") else 0
    xb, yb_, ob = torch.zeros(n + 1, device=DEV), torch.zeros(n + 1, device=DEV), nan_buf(n + 9)
    xd, yd, od = xb[ox:ox + n], yb_[oy:oy + n], ob[ox:ox + n]
    xd.copy_(x)
    yd.copy_(y)
    if views.startswith("y_none"):
        yd = None
    vec = aligned(16, xd, yd, od)
    assert vec == (views in ("aligned", "y_none"))
    if n == AXPBY_SIZES[-1]:
        assert past_cap(n // 4 + 1 if vec else n) and n % 4 == 3
    rc = lib.lib().eamd_axpby(lib.ptr(xd), lib.ptr(yd), lib.ptr(od), n, a, b, stream(lib))
    assert rc == 0
    a64, b64 = float(np.float32(a)), float(np.float32(b))
    t1, t2 = a64 * x.double(), (b64 * y.double() if yd is not None else torch.zeros(n, dtype=torch.float64))
    check("AXPBY_TOL", f"axpby n={n} {views}", od, t1 + t2, t1.abs() + t2.abs(), n_terms=2)
    assert_guards("axpby", ob, (torch.arange(n + 9) >= ox) & (torch.arange(n + 9) < ox + n))


@pytest.mark.parametrize("n", [1, 1001, 2048 * 256 + 777])
def test_scale_dev_vs_float64(lib, n):
    assert past_cap(n) == (n > 1001)
    x = torch.randn(n, generator=gen(n))
    s, extra = torch.tensor([0.731]), 1.0 / 3.0
    ob = nan_buf(n + 8)
    xd, sd = x.to(DEV), s.to(DEV)
    rc = lib.lib().eamd_scale_dev(lib.ptr(xd), lib.ptr(sd), lib.ptr(ob), n, extra, stream(lib))
    assert rc == 0
    ref = float(s[0]) * float(np.float32(extra)) * x.double()
    check("SCALE_DEV_TOL", f"scale_dev n={n}", ob[:n], ref, ref.abs(), n_terms=2)
    assert_guards("scale_dev", ob, torch.arange(n + 8) < n)


ADD_SHAPES = [(1, 2), (33, 48), (70, 321), (2100, 256)]


@pytest.mark.parametrize("rows,cols", ADD_SHAPES)
def test_add_block_f32_vs_float64(ops, rows, cols):
    """out[r * ld + c] = a + b into a column block (ld_out > cols, offset 7) of a NaN-filled matrix; b = None is a copy"""
    assert past_cap(rows * cols) == (rows == 2100)
    g = gen(rows + cols)
    a, b = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    ld, off = cols + 52, 7
    total = off + rows * ld + 8
    written = block_mask(total, off, rows, cols, ld)
    out = nan_buf(total)
    ops.add_cast(a.to(DEV), b.to(DEV), out=out, out_off=off, ld_out=ld)
    check("ADD_TOL", f"add_block_f32 {rows}x{cols}", block_of(out, off, rows, cols, ld), a.double() + b.double(),
          a.double().abs() + b.double().abs(), n_terms=2)
    assert_guards("add_block_f32", out, written)
    out = nan_buf(total)
    ops.add_cast(a.to(DEV), None, out=out, out_off=off, ld_out=ld)
    assert_bits(f"add_block_f32 b=None {rows}x{cols}", block_of(out, off, rows, cols, ld), a)
    assert_guards("add_block_f32 b=None", out, written)


def add_cast_x2(a, b, out, out_off, cols, ld):
    """the dispatch predicate of eamd_add_cast_bf16"""
    return cols % 2 == 0 and ld % 2 == 0 and aligned(8, a, b) and (out.data_ptr() + 2 * out_off) % 4 == 0


@pytest.mark.parametrize("variant", ["x2", "odd_ld", "odd_off", "b_none", "b_none_odd_off"])
@pytest.mark.parametrize("rows,cols", ADD_SHAPES)
def test_add_cast_bf16_vs_float64(ops, rows, cols, variant):
    """bf16(a + b) into a column block: the dword-pair kernel (even cols and ld_out, 4-byte aligned destination) and the
    scalar kernel by odd cols (70 x 321), odd ld_out, or an out_off that leaves the destination 2-byte aligned"""
    g = gen(rows * 7 + cols)
    a, b = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    ld = cols + 52
    if variant == "odd_ld" and ld % 2 == 0:
        ld += 1
    off = 7 if variant.endswith("odd_off") else 6
    total = off + rows * ld + 8
    out = nan_buf(total, BF16)
    ad, bd = a.to(DEV), (None if variant.startswith("b_none") else b.to(DEV))
    x2 = add_cast_x2(ad, bd, out, off, cols, ld)
    assert x2 == (cols % 2 == 0 and variant in ("x2", "b_none")), f"{variant} {rows}x{cols}: wrong branch"
    assert past_cap(rows * cols // 2 if x2 else rows * cols) == (rows == 2100 and not x2)
    ops.add_cast(ad, bd, out=out, out_off=off, ld_out=ld)
    got = block_of(out, off, rows, cols, ld)
    if bd is None:
        assert_bits(f"add_cast_bf16 {variant} {rows}x{cols}", got, a.to(BF16))
    else:
        check_bf16("ADD_TOL", f"add_cast_bf16 {variant} {rows}x{cols}", got, a.double() + b.double(),
                   a.double().abs() + b.double().abs(), n_terms=2)
    assert_guards("add_cast_bf16", out, block_mask(total, off, rows, cols, ld))


# (D, rows, ldq, q_off, bf16) -> branch
ADD_BIAS2_CASES = [
    ("fp32_dense", 64, 33, 64, 0, False, "scalar"), ("fp32_qkv_block", 256, 2100, 768, 256, False, "scalar"),
    ("fp32_odd_D", 7, 33, 21, 7, False, "scalar"),
    ("bf16_x2_q", 256, 4100, 768, 0, True, "x2"), ("bf16_x2_k", 256, 33, 768, 256, True, "x2"),
    ("bf16_x2_D64", 64, 70, 192, 64, True, "x2"),
    ("bf16_odd_q_off", 256, 2100, 768, 257, True, "scalar"), ("bf16_odd_q_off_D64", 64, 33, 194, 1, True, "scalar"),
    ("bf16_odd_D", 7, 33, 21, 7, True, "scalar"), ("bf16_odd_ldq", 64, 33, 193, 0, True, "scalar"),
]


@pytest.mark.parametrize("name,D,rows,ldq,q_off,bf16,branch", ADD_BIAS2_CASES, ids=[c[0] for c in ADD_BIAS2_CASES])
def test_add_bias2_vs_float64(lib, name, D, rows, ldq, q_off, bf16, branch):
    """qu = q + u, qv = q + v from a column block (q_off, ldq) of the fused projection: fp32, the bf16 dword-pair kernel and the
    bf16 scalar kernel (odd q_off, odd D, odd ldq); fp32_qkv_block, bf16_x2_q and bf16_odd_q_off run past the grid cap"""
    g = gen(D + rows + q_off)
    dt = BF16 if bf16 else F32
    q = torch.randn(q_off + rows * ldq + 8, generator=g).to(dt)
    u, v = torch.randn(D, generator=g), torch.randn(D, generator=g)
    qd = q.to(DEV)
    qub, qvb = nan_buf(rows * D + 8, dt), nan_buf(rows * D + 8, dt)
    x2 = bf16 and D % 2 == 0 and ldq % 2 == 0 and (qd.data_ptr() + 2 * q_off) % 4 == 0 and aligned(4, qub, qvb)
    assert x2 == (branch == "x2")
    assert past_cap(rows * D // 2 if x2 else rows * D) == (rows >= 2100)
    ud, vd = u.to(DEV), v.to(DEV)
    rc = lib.lib().eamd_add_bias2(lib.ptr(qd, q_off), ldq, lib.ptr(ud), lib.ptr(vd), lib.ptr(qub), lib.ptr(qvb),
                                  rows, D, 1 if bf16 else 0, stream(lib))
    assert rc == 0
    q64 = block_of(q, q_off, rows, D, ldq).double()
    for what, buf, bias in (("qu", qub, u), ("qv", qvb, v)):
        ref, mag = q64 + bias.double(), q64.abs() + bias.double().abs()
        if bf16:
            check_bf16("ADD_TOL", f"add_bias2 {name} {what}", buf[:rows * D].cpu().view(rows, D), ref, mag, n_terms=2)
        else:
            check("ADD_TOL", f"add_bias2 {name} {what}", buf[:rows * D].view(rows, D), ref, mag, n_terms=2)
        assert_guards(f"add_bias2 {name} {what}", buf, torch.arange(rows * D + 8) < rows * D)


def colsum_geom(rows, D, ld, bf16, base_aligned4):
    """eamd_colsum's host code: (pair, gx, rows per block, gy)"""
    pair = bf16 and D % 2 == 0 and ld % 2 == 0 and base_aligned4
    ncol = D // 2 if pair else D
    gx = cdiv(ncol, 256)
    want = max(1024 // gx, 1)
    rpb = max(cdiv(rows, want), 64 if pair else 128, 8)
    return pair, gx, rpb, cdiv(rows, rpb)


COLSUM_SHAPES = [(1, 1), (7, 70), (8, 256), (9, 513), (500, 70), (500, 513), (70000, 256)]
# name: (bf16, extra leading dimension, element offset of the base)
COLSUM_VARIANTS = {"fp32": (False, 0, 0), "fp32_ld": (False, 3, 0), "bf16_auto": (True, 0, 0), "bf16_ld2": (True, 2, 0),
                   "bf16_odd_ld": (True, 1, 0), "bf16_2byte_view": (True, 2, 1)}


@pytest.mark.parametrize("variant", list(COLSUM_VARIANTS))
@pytest.mark.parametrize("rows,D", COLSUM_SHAPES)
def test_colsum_vs_float64(ops, rows, D, variant):
    """out[D] += scale * column sums: fp32 and strided fp32, the bf16 dword-pair kernel (even D and ld, 4-byte aligned base) and
    the bf16 scalar kernel by odd D, odd ld or a 2-byte-aligned view; 8-row trips with a row tail, several row slabs (gy > 1,
    the last one short), up to three column blocks.  Accumulates onto non-zero values, called twice; the atomic order varies,
    so the error is judged against |out0| + the sum of the moduli of the terms."""
    bf16, dld, off = COLSUM_VARIANTS[variant]
    ld = D + dld
    g = gen(rows + D)
    dt = BF16 if bf16 else F32
    buf = torch.randn(off + rows * ld + 8, generator=g).to(dt)
    bd = buf.to(DEV)
    xd = bd[off:]
    pair, gx, rpb, gy = colsum_geom(rows, D, ld, bf16, xd.data_ptr() % 4 == 0)
    assert pair == (bf16 and D % 2 == 0 and variant in ("bf16_auto", "bf16_ld2")), f"{variant} {rows}x{D}: wrong branch"
    assert gx == (3 if D == 513 else 1)
    if rows >= 500:
        assert gy > 1 and rows % rpb != 0
    scale = 0.37
    out0 = torch.randn(D + 8, generator=g)
    out = out0.to(DEV)
    for _ in range(2):
        ops.colsum(xd, out, scale=scale, rows=rows, D=D, ld=ld)
    x64 = block_of(buf, off, rows, D, ld).double()
    s32 = float(np.float32(scale))
    ref = out0[:D].double() + 2 * s32 * x64.sum(0)
    mag = out0[:D].double().abs() + 2 * s32 * x64.abs().sum(0)
    check("COLSUM_TOL", f"colsum {variant} {rows}x{D} (rpb {rpb}, grid {gx}x{gy})", out[:D], ref, mag, n_terms=min(rows, rpb) + gy + 2)
    assert_bits(f"colsum {variant} guard", out[D:], out0[D:])


ACC_RPB = 64             # rows per block of add_cast_colsum2_kernel


def colsum2_supported(a, b, out, out_off, D, ld, f32out):
    """the predicates of eamd_add_cast_colsum2 / eamd_add_colsum2_f32"""
    o = out.data_ptr() + out_off * out.element_size()
    return D % 2 == 0 and D <= 512 and ld % 2 == 0 and aligned(8, a, b) and o % (8 if f32out else 4) == 0


def colsum2_case(ops, lib, rows, D, out_dt, ld, off, fused):
    g = gen(rows * 3 + D)
    a, b = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    sa0, sb0 = torch.randn(D + 8, generator=g), torch.randn(D + 8, generator=g)
    ad, bd, sa, sb = a.to(DEV), b.to(DEV), sa0.to(DEV), sb0.to(DEV)
    total = off + rows * ld + 8
    out = nan_buf(total, out_dt)
    f32out = out_dt == F32
    assert colsum2_supported(ad, bd, out, off, D, ld, f32out) == fused, f"rows={rows} D={D} ld={ld} off={off}: wrong branch"
    if not fused:       # the entry point refuses before any launch
        fn = lib.lib().eamd_add_colsum2_f32 if f32out else lib.lib().eamd_add_cast_colsum2
        assert fn(lib.ptr(ad), lib.ptr(bd), lib.ptr(out, off), ld, lib.ptr(sa), lib.ptr(sb), rows, D, stream(lib)) == EUNSUPPORTED
    for _ in range(2):
        ops.add_cast_colsum2(ad, bd, sa[:D], sb[:D], out=out, out_off=off, ld_out=ld)
    name = f"add_cast_colsum2 {'f32' if f32out else 'bf16'} {rows}x{D} ld={ld} off={off}"
    got = block_of(out, off, rows, D, ld)
    ref, mag = a.double() + b.double(), a.double().abs() + b.double().abs()
    if f32out:
        check("ADD_TOL", name + " out", got, ref, mag, n_terms=2)
    else:
        check_bf16("ADD_TOL", name + " out", got, ref, mag, n_terms=2)
    assert_guards(name, out, block_mask(total, off, rows, D, ld))
    if fused:
        ngrp = 256 // (D // 2)
        n_terms = cdiv(min(rows, ACC_RPB), ngrp) + ngrp + cdiv(rows, ACC_RPB) + 2
    else:
        n_terms = min(rows, 128) + cdiv(rows, 128) + 2
    for what, s, s0, t in (("suma", sa, sa0, a), ("sumb", sb, sb0, b)):
        check("COLSUM_TOL", f"{name} {what}", s[:D], s0[:D].double() + 2 * t.double().sum(0),
              s0[:D].double().abs() + 2 * t.double().abs().sum(0), n_terms=n_terms)
        assert_bits(f"{name} {what} guard", s[D:], s0[D:])


@pytest.mark.parametrize("out_dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("D", [2, 64, 320, 512])
def test_add_cast_colsum2_fused(ops, lib, D, out_dt):
    """both template forms of add_cast_colsum2_kernel: 256 row groups of one column pair (D = 2), 8 and 1 row groups, D = 320
    with ngrp = 1 and 96 idle threads; rows around one block's 64, the four-row trips and their tail; dense and as a column block"""
    assert (256 // (D // 2), 256 - (256 // (D // 2)) * (D // 2)) == {2: (256, 0), 64: (8, 0), 320: (1, 96), 512: (1, 0)}[D]
    for rows in (1, 63, 64, 65, 64 * 7 + 5):
        colsum2_case(ops, lib, rows, D, out_dt, D, 0, True)
    colsum2_case(ops, lib, 65, D, out_dt, D + 52, 6, True)


@pytest.mark.parametrize("out_dt", [BF16, F32], ids=["bf16", "f32"])
def test_add_cast_colsum2_fallback(ops, lib, out_dt):
    """D = 514 (> 512) and a misaligned destination are refused with EUNSUPPORTED; ops.add_cast_colsum2 then computes the same
    with add_cast + two colsum launches"""
    for rows in (1, 65, 64 * 7 + 5):
        colsum2_case(ops, lib, rows, 514, out_dt, 514, 0, False)
    colsum2_case(ops, lib, 65, 64, out_dt, 64 + 52, 7, False)


@pytest.mark.parametrize("B,T,D", [(3, 7, 16), (5, 411, 256)])
def test_posenc_vs_float64(lib, B, T, D):
    """x * scale + pe[r % T] and x * scale + alpha[0] * pe[r % T] over rows = B * T (r % T wraps B - 1 times); the second shape
    runs the grid-stride second trip"""
    rows = B * T
    assert past_cap(rows * D) == (T == 411) and rows > T
    g = gen(B + T + D)
    x, pe, alpha, scale = torch.randn(rows, D, generator=g), torch.randn(T + 2, D, generator=g), torch.tensor([0.77]), math.sqrt(D)
    L, p = lib.lib(), lib.ptr
    xs = float(np.float32(scale)) * x.double()
    pr = pe.double()[torch.arange(rows) % T]
    ob = nan_buf(rows * D + 8)
    xd, ped, ad = x.to(DEV), pe.to(DEV), alpha.to(DEV)
    assert L.eamd_posenc(p(xd), p(ped), p(ob), rows, T, D, scale, stream(lib)) == 0
    check("POSENC_TOL", f"posenc {B}x{T}x{D}", ob[:rows * D].view(rows, D), xs + pr, xs.abs() + pr.abs(), n_terms=2)
    assert_guards("posenc", ob, torch.arange(rows * D + 8) < rows * D)
    ob = nan_buf(rows * D + 8)
    assert L.eamd_posenc_scaled(p(xd), p(ped), p(ad), p(ob), rows, T, D, scale, stream(lib)) == 0
    ap = float(alpha[0]) * pr
    check("POSENC_TOL", f"posenc_scaled {B}x{T}x{D}", ob[:rows * D].view(rows, D), xs + ap, xs.abs() + ap.abs(), n_terms=2)
    assert_guards("posenc_scaled", ob, torch.arange(rows * D + 8) < rows * D)


@pytest.mark.parametrize("B,T,D", [(1, 5, 20), (16, 256, 256), (14, 300, 256)])
def test_posenc_scaled_bwd_vs_float64(ops, B, T, D):
    """dalpha += sum dout * pe[t]: below one block, exactly 256 * 8 * 512 elements (the 512-block cap reached) and beyond it
    (more than 8 elements per thread); accumulates onto a non-zero value, called twice"""
    rows = B * T
    n = rows * D
    blocks = max(1, min(512, cdiv(n, 256 * 8)))
    assert (blocks, n) == {5: (1, 100), 256: (512, 256 * 8 * 512), 300: (512, 1075200)}[T]
    g = gen(T)
    dout, pe = torch.randn(rows, D, generator=g), torch.randn(T + 1, D, generator=g)
    da0 = torch.tensor([0.625, 3.0])
    da = da0.to(DEV)
    for _ in range(2):
        ops.posenc_scaled_bwd(dout.to(DEV), pe.to(DEV), da, T)
    prod = dout.double() * pe.double()[torch.arange(rows) % T]
    ref = da0[:1].double() + 2 * prod.sum()
    mag = da0[:1].double().abs() + 2 * prod.abs().sum()
    check("POSENC_BWD_TOL", f"posenc_scaled_bwd n={n}", da[:1], ref, mag, n_terms=cdiv(n, blocks * 256) + 10 + blocks)
    assert float(da[1]) == 3.0


@pytest.mark.parametrize("B,T,C,k", UNFOLD_SHAPES)
def test_fold1d_vs_float64(lib, B, T, C, k):
    """dx[b, t, c] = sum over the taps whose source row lies inside the sequence: the adjoint of unfold1d"""
    g = gen(B * T + C + k)
    dcol = torch.randn(B, T, k, C, generator=g)
    n = B * T * C
    dxb = nan_buf(n + 8)
    dcd = dcol.to(DEV)
    assert lib.lib().eamd_fold1d(lib.ptr(dcd), lib.ptr(dxb), B, T, C, k, stream(lib)) == 0
    p = (k - 1) // 2
    ref, mag = torch.zeros(B, T + 2 * p, C, dtype=torch.float64), torch.zeros(B, T + 2 * p, C, dtype=torch.float64)
    for kk in range(k):          # col[b, ts, kk] = x[b, ts + kk - p]  =>  dx[b, ts + kk - p] += dcol[b, ts, kk]
        ref[:, kk:kk + T] += dcol[:, :, kk].double()
        mag[:, kk:kk + T] += dcol[:, :, kk].double().abs()
    check("FOLD_TOL", f"fold1d {(B, T, C, k)}", dxb[:n].view(B, T, C), ref[:, p:p + T], mag[:, p:p + T].clamp_min(1e-30), n_terms=k)
    assert_guards("fold1d", dxb, torch.arange(n + 8) < n)


# =============================================================================================
# 6. transcendental kernels
# =============================================================================================
def act_ids():
    """the activation ids of the C ABI (the EAMD_ACT_* enum shared by host and device)"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "espnet_amd", "csrc", "common.h")
    with open(path) as f:
        ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"EAMD_ACT_(\w+) = (\d+)", f.read())}
    assert sorted(ids) == ["hardtanh", "none", "relu", "selu", "swish", "tanh"]
    return ids


ACTS = act_ids()
SELU_ALPHA, SELU_SCALE = 1.6732632423543772, 1.0507009873554805
# forward values relative to max(|ref|, 1), backward values to max(|dact ref|, 1) * |dy|
ACT_EXACT_TOL = 0.0       # none / relu / hardtanh and their derivatives (a derivative at a kink: either one-sided value)
ACT_SWISH_TOL = 5.1e-07   # observed 1.29e-7
ACT_TANH_TOL = 2.3e-07    # observed 5.98e-8
ACT_SELU_TOL = 5.4e-07    # observed 1.36e-7
DACT_SWISH_TOL = 3.8e-06  # observed 1.02e-6
DACT_TANH_TOL = 4.9e-07   # observed 1.23e-7
DACT_SELU_TOL = 6.8e-07   # observed 1.71e-7
GLU_FWD_TOL = 7.6e-07     # a * sigmoid(g); observed 1.92e-7
GLU_BWD_TOL = 3.8e-06     # dy * s and dy * a * s * (1 - s); observed 9.73e-7
DROPOUT_ACT_TOL = 6.8e-07 # act(x) * inv of eamd_dropout's activation branch (swish; relu is exact); observed 1.71e-7
ACT_TOLS = {"none": "ACT_EXACT_TOL", "relu": "ACT_EXACT_TOL", "hardtanh": "ACT_EXACT_TOL", "swish": "ACT_SWISH_TOL",
            "tanh": "ACT_TANH_TOL", "selu": "ACT_SELU_TOL"}
DACT_TOLS = {"none": "ACT_EXACT_TOL", "relu": "ACT_EXACT_TOL", "hardtanh": "ACT_EXACT_TOL", "swish": "DACT_SWISH_TOL",
             "tanh": "DACT_TANH_TOL", "selu": "DACT_SELU_TOL"}


def act_ref(x, act):
    """float64 activation and its derivative(s): (a, d, d_other), d_other the other one-sided derivative at a kink"""
    s = torch.sigmoid(x)
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    if act == "none":
        return x, one, one
    if act == "relu":
        return F.relu(x), (x > 0).double(), torch.where(x == 0, one, (x > 0).double())
    if act == "swish":
        d = s * (1 + x * (1 - s))
        return x * s, d, d
    if act == "tanh":
        t = torch.tanh(x)
        return t, 1 - t * t, 1 - t * t
    if act == "hardtanh":
        d = ((x > -1) & (x < 1)).double()
        return F.hardtanh(x), d, torch.where(x.abs() == 1, one, d)
    if act == "selu":
        d = SELU_SCALE * torch.where(x > 0, one, SELU_ALPHA * torch.exp(x))
        return F.selu(x), d, torch.where(x == 0, SELU_SCALE * one, d)
    raise KeyError(act)


def act_inputs(n):
    """+-0, +-1 exactly (hardtanh's kinks), +-88, +-inf, then a grid over [-30, 30], tiled up to n"""
    sp = torch.tensor([0.0, -0.0, 1.0, -1.0, 88.0, -88.0, INF, -INF])
    grid = torch.cat([sp, torch.linspace(-30, 30, 6001), torch.linspace(-2, 2, 4001)])
    return grid.repeat(cdiv(n, grid.numel()))[:n].clone()


@pytest.mark.parametrize("n", [37, 2048 * 256 + 1])
@pytest.mark.parametrize("act", sorted(ACTS, key=ACTS.get))
def test_act_fwd_bwd_vs_float64(lib, act, n):
    """eamd_act_fwd / eamd_act_bwd for the six ids; n one past the grid cap runs the grid-stride second trip"""
    assert past_cap(n) == (n > 37)
    x = act_inputs(n)
    dy = torch.randn(n, generator=gen(n)) + 0.1
    L, p = lib.lib(), lib.ptr
    yb, dxb = nan_buf(n + 8), nan_buf(n + 8)
    xd = x.to(DEV)
    assert L.eamd_act_fwd(p(xd), p(yb), n, ACTS[act], stream(lib)) == 0
    dyd = dy.to(DEV)
    assert L.eamd_act_bwd(p(dyd), p(xd), p(dxb), n, ACTS[act], stream(lib)) == 0
    a, d, d2 = act_ref(x.double(), act)
    check(ACT_TOLS[act], f"act_fwd {act} n={n}", yb[:n], a, a.abs().clamp_min(1.0).nan_to_num(1.0, 1.0, 1.0))
    sc = d.abs().clamp_min(1.0).nan_to_num(1.0, 1.0, 1.0) * dy.double().abs()
    check(DACT_TOLS[act], f"act_bwd {act} n={n}", dxb[:n], dy.double() * d, sc, either=dy.double() * d2)
    assert_guards("act_fwd", yb, torch.arange(n + 8) < n)
    assert_guards("act_bwd", dxb, torch.arange(n + 8) < n)


GLU_SHAPES = [(5, 3), (33, 48), (1100, 480)]


def glu_ref(x, dy, C):
    a, gt = x.double()[:, :C], x.double()[:, C:]
    s = torch.sigmoid(gt)
    d = dy.double()
    return a * s, torch.cat([d * s, d * a * s * (1 - s)], 1), torch.cat([s.clamp_min(1.0) * d.abs(), (a * s * (1 - s)).abs().clamp_min(1.0) * d.abs()], 1)


@pytest.mark.parametrize("rows,C", GLU_SHAPES)
def test_glu_fwd_bwd_vs_float64(lib, rows, C):
    """glu_fwd; glu_bwd to fp32, to bf16 by the dword-pair kernel (even C, 8-byte aligned dy / x, 4-byte aligned dx) and to bf16
    by the scalar kernel (odd C, or a dy view offset by one element); 1100 x 480 runs past the grid cap"""
    assert past_cap(rows * C) == (rows == 1100)
    g = gen(rows + C)
    x, dy = torch.randn(rows, 2 * C, generator=g) * 3, torch.randn(rows, C, generator=g)
    L, p = lib.lib(), lib.ptr
    xd = x.to(DEV)
    dyb = torch.zeros(rows * C + 1, device=DEV)
    y, dx, scale = glu_ref(x, dy, C)
    yb = nan_buf(rows * C + 8)
    assert L.eamd_glu_fwd(p(xd), p(yb), rows, C, stream(lib)) == 0
    check("GLU_FWD_TOL", f"glu_fwd {rows}x{C}", yb[:rows * C].view(rows, C), y, y.abs().clamp_min(1.0))
    assert_guards("glu_fwd", yb, torch.arange(rows * C + 8) < rows * C)
    for name, out_dt, off in (("fp32", F32, 0), ("bf16", BF16, 0), ("bf16_dy_offset", BF16, 1)):
        dyd = dyb[off:off + rows * C]
        dyd.copy_(dy.reshape(-1))
        dxb = nan_buf(rows * 2 * C + 8, out_dt)
        x2 = out_dt == BF16 and C % 2 == 0 and aligned(8, dyd, xd) and aligned(4, dxb)
        assert x2 == (name == "bf16" and C % 2 == 0), f"glu_bwd {name} {rows}x{C}: wrong branch"
        d32, d16 = (p(dxb), None) if out_dt == F32 else (None, p(dxb))
        assert L.eamd_glu_bwd(p(dyd), p(xd), d32, d16, rows, C, stream(lib)) == 0
        got = dxb[:rows * 2 * C].view(rows, 2 * C)
        if out_dt == F32:
            check("GLU_BWD_TOL", f"glu_bwd {name} {rows}x{C}", got, dx, scale)
        else:
            check_bf16("GLU_BWD_TOL", f"glu_bwd {name} {rows}x{C} ({'x2' if x2 else 'scalar'})", got.cpu(), dx, scale)
        assert_guards(f"glu_bwd {name}", dxb, torch.arange(rows * 2 * C + 8) < rows * 2 * C)


@pytest.mark.parametrize("path", ["vec4_f32_f32", "vec4_f32_bf16", "scalar_n_mod_4", "scalar_offset_view"])
@pytest.mark.parametrize("act", ["swish", "relu"])
def test_dropout_activation_branch(lib, act, path):
    """drop(act(x)): the kept set is the plain mask (the activation comes before it) and the survivors are act(x) * inv"""
    in_dt, out_dt, off, _ = DROP_PATHS[path]
    n = 1025 if path == "scalar_n_mod_4" else 1024
    p_, salt, step = 0.3, 11, 5
    x = torch.randn(n, generator=gen(n)) * 3
    x[x == 0] = 1.0
    xd, yb, yd, written = drop_buffers(x, off, out_dt)
    assert drop_call(lib, xd, yd, n, p_, step, salt, act=ACTS[act]) == path.startswith("vec4")
    keep = drop_keep(step, salt, n, p_)
    inv = float(dr.drop_inv(dr.drop_thr16(p_)))
    a = act_ref(x.double(), act)[0]
    ref = torch.where(keep, a * inv, torch.zeros((), dtype=torch.float64))
    got = yd.cpu()
    live = keep & (x > 0) if act == "relu" else keep
    assert torch.equal(got.float() != 0, live), f"dropout {act} {path}: kept set changed"
    name = f"dropout act={act} {path}"
    if act == "relu":       # one fp32 product (then RNE for a bf16 output): bit for bit
        assert_bits(name, got, torch.where(live, x * torch.tensor(inv, dtype=F32), torch.zeros(())).to(out_dt))
    elif out_dt == BF16:
        check_bf16("DROPOUT_ACT_TOL", name, got, ref, ref.abs().clamp_min(1.0))
    else:
        check("DROPOUT_ACT_TOL", name, got, ref, ref.abs().clamp_min(1.0))
    assert_guards(name, yb, written)


# above 64 * 2^-24: grad_noise_kernel's __sincosf is one v_sin_f32 / v_cos_f32 on the angle in revolutions (an absolute error of
# a few 1e-7 that does not shrink with the result) and its __logf one v_log_f32; the radius sqrt(-2 log u0), up to 5.6 at
# these sizes, multiplies the former
NOISE_TOL = 7.2e-06       # |g - (g0 + sigma z)| / sigma: __logf, __sincosf and the fp32 sum; observed 1.81e-6
NOISE_SIZES = [1, 2, 7, 2 * 4096 * 256 + 2 * 256 * 5 + 1]


@pytest.mark.parametrize("n", NOISE_SIZES)
def test_gradient_noise_vs_restatement(lib, n):
    """g += sigma * N(0, 1), element-wise against the float64 Box-Muller restatement from the same two hashes; the last size
    runs the second trip of the 4096-block grid and the odd tail (no sine half for the last pair); sigma = 0 leaves g alone"""
    pairs = (n + 1) // 2
    assert (pairs > 4096 * 256) == (n == NOISE_SIZES[-1])
    salt, sigma = 0x6e6f697365, 0.5
    g0 = torch.randn(n + 9, generator=gen(n))
    for step in ((7, 2 ** 33) if n < 100 else (7,)):
        gd = g0.to(DEV)
        st = torch.tensor([step], dtype=torch.int64, device=DEV)
        assert lib.lib().eamd_add_gradient_noise(lib.ptr(gd), n, sigma, lib.ptr(st), salt, stream(lib)) == 0
        z = torch.from_numpy(dr.gradient_noise(step, salt, n))
        ref = g0[:n].double() + float(np.float32(sigma)) * z
        check("NOISE_TOL", f"gradient noise n={n} step={step}", gd[:n], ref, torch.full((1,), sigma, dtype=torch.float64))
        assert_bits("gradient noise guard", gd[n:], g0[n:])
    gd = g0.abs().to(DEV)           # (a -0 would become +0)
    st = torch.tensor([7], dtype=torch.int64, device=DEV)
    assert lib.lib().eamd_add_gradient_noise(lib.ptr(gd), n, 0.0, lib.ptr(st), salt, stream(lib)) == 0
    assert_bits("gradient noise sigma=0", gd, g0.abs())


# =============================================================================================
# 7. optimizer
# =============================================================================================
NORM_TOL = 7.8e-08        # ||g||, relative; observed 1.96e-8
SCHED_LR_TOL = 4.7e-07    # state[1], relative (rsqrtf, powf); observed 1.20e-7
SCHED_BC_TOL = 1.6e-06    # state[2], state[3] = 1 - beta^step, relative (powf, then the subtraction); observed 4.09e-7
SCHED_COEF_TOL = 2.2e-07  # state[6] = max_norm / (norm + 1e-6), relative; observed 5.65e-8
ADAM_P_TOL = 1.3e-06      # p after 3 steps, relative to max(|ref|, lr); observed 3.32e-7
ADAM_M_TOL = 7.3e-07      # m, relative to the same recursion on the moduli of its terms; observed 1.85e-7
ADAM_V_TOL = 8.4e-07      # v, relative; observed 2.11e-7
ADADELTA_P_TOL = 6.9e-07  # p after 3 steps, relative to max(|ref|, lr); observed 1.74e-7
ADADELTA_SQ_TOL = 1.1e-06 # square_avg, relative; observed 2.76e-7
ADADELTA_ACC_TOL = 2.4e-06# acc_delta, relative; observed 6.13e-7
NORM_SIZES = [1, 5, 10007, 4 * 1024 * 256 + 4 * 256 * 2 + 3]


def f32v(v):
    """the value a float argument has once it is an fp32"""
    return float(np.float32(v))


@pytest.mark.parametrize("n", NORM_SIZES)
def test_grad_norm_vs_float64(lib, n):
    """float4 body + scalar tail (n unpadded), the 1024-block cap with its second trip; inf / NaN propagate; a 16-byte
    misaligned g is refused"""
    want = cdiv(n // 4, 256)
    assert (want > 1024) == (n == NORM_SIZES[-1]) and (n % 4 != 0)
    g = torch.randn(n, generator=gen(n)) * 0.3
    L, p = lib.lib(), lib.ptr
    gd, ws, out = g.to(DEV), nan_buf(1024), nan_buf(4)
    assert aligned(16, gd)
    assert L.eamd_grad_norm(p(gd), n, p(ws), p(out), stream(lib)) == 0
    ref = g.double().norm().reshape(1)
    check("NORM_TOL", f"grad_norm n={n}", out[:1], ref, ref)
    assert_guards("grad_norm", out, torch.arange(4) < 1)
    for bad in (INF, -INF, NAN):
        g2 = g.clone()
        g2[n - 1] = bad
        out = nan_buf(4)
        g2d = g2.to(DEV)
        assert L.eamd_grad_norm(p(g2d), n, p(ws), p(out), stream(lib)) == 0
        assert float(out[0]) == INF if math.isinf(bad) else math.isnan(float(out[0]))
    if n > 1:
        gb = torch.zeros(n + 1, device=DEV)
        out = nan_buf(4)
        assert not aligned(16, gb[1:])
        assert L.eamd_grad_norm(p(gb[1:]), n, p(ws), p(out), stream(lib)) == EINVAL
        assert_guards("refused grad_norm", out, torch.zeros(4, dtype=torch.bool))


def sched_ref(mode, step, base, factor, dmodel, warmup, b1, b2):
    lr = base
    if mode == 1:
        lr = factor * dmodel ** -0.5 * min(step ** -0.5, step * warmup ** -1.5)
    elif mode == 2:
        lr = base * warmup ** 0.5 * min(step ** -0.5, step * warmup ** -1.5)
    return lr, 1 - b1 ** step, 1 - b2 ** step


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_sched_step_vs_float64(ops, lib, mode):
    """constant / Noam / WarmupLR over steps 1..40 with warmup 25 (the warm-up is crossed), every state entry after every step;
    the clip coefficient without a bound, under it and over it; a non-finite norm skips; mode 3 is refused"""
    base, factor, dmodel, warm, b1, b2, max_norm = f32v(1e-3), f32v(2.5), 256.0, 25.0, f32v(0.9), f32v(0.98), 5.0
    state = torch.zeros(8, device=DEV)
    gn = torch.zeros(1, device=DEV)
    got, ref = [], []
    for step in range(1, 41):
        norm = f32v(0.5 + 0.37 * step)            # crosses max_norm at step 13
        gn.fill_(norm)
        ops.sched_step(state, gn, mode, base, factor, dmodel, warm, b1, b2, max_norm)
        got.append(state.cpu())
        lr, bc1, bc2 = sched_ref(mode, step, base, factor, dmodel, warm, b1, b2)
        ref.append([step, lr, bc1, bc2, norm, 0.0, min(1.0, max_norm / (norm + f32v(1e-6)))])
    got, ref = torch.stack(got), torch.tensor(ref, dtype=torch.float64)
    assert torch.equal(got[:, 0].double(), ref[:, 0]) and torch.equal(got[:, 4].double(), ref[:, 4]) and not bool(got[:, 5].any())
    assert bool((ref[:12, 6] == 1).all()) and bool((ref[12:, 6] < 1).all())
    check("SCHED_LR_TOL", f"sched mode {mode} lr", got[:, 1], ref[:, 1], ref[:, 1])
    check("SCHED_BC_TOL", f"sched mode {mode} bias corrections", got[:, 2:4], ref[:, 2:4], ref[:, 2:4])
    check("SCHED_COEF_TOL", f"sched mode {mode} clip coef", got[:, 6], ref[:, 6], ref[:, 6])
    # no bound (max_norm = 0) and no norm at all: coef 1
    ops.sched_step(state, gn, mode, base, factor, dmodel, warm, b1, b2, 0.0)
    assert float(state[6]) == 1.0 and float(state[0]) == 41.0
    ops.sched_step(state, None, mode, base, factor, dmodel, warm, b1, b2, max_norm)
    assert float(state[6]) == 1.0 and float(state[4]) == 0.0 and float(state[0]) == 42.0
    # a non-finite norm: state[0..3] untouched, state[6] = 0, state[5] counts
    for k, bad in enumerate((INF, NAN)):
        before = state.cpu()
        gn.fill_(bad)
        ops.sched_step(state, gn, mode, base, factor, dmodel, warm, b1, b2, max_norm)
        after = state.cpu()
        assert_bits("sched skip state[0..3]", after[:4], before[:4])
        assert float(after[6]) == 0.0 and float(after[5]) == k + 1 and float(after[7]) == 0.0
        assert (float(after[4]) == INF) if k == 0 else math.isnan(float(after[4]))
    before = state.cpu()
    assert lib.lib().eamd_sched_step(lib.ptr(state), lib.ptr(gn), 3, base, factor, dmodel, warm, b1, b2, max_norm, stream(lib)) == EINVAL
    assert_bits("refused sched_step", state, before)


OPT_SIZES = [3, 10007, 4 * 2048 * 256 + 4 * 256 + 2]
B1, B2, ADAM_EPS, RHO = f32v(0.9), f32v(0.98), f32v(1e-9), f32v(0.95)
# (weight decay, bf16 shadow); the size past the grid cap takes the first and the last
OPT_OPTIONS = [(0.0, False), (0.0, True), (0.01, False), (0.01, True)]


def opt_state(step, lr, coef, norm, eps=0.0):
    """the 8 floats eamd_sched_step leaves (written directly: these tests isolate the update kernels)"""
    return torch.tensor([step, lr, 1 - B1 ** step, 1 - B2 ** step, norm, 0.0, coef, eps], dtype=F32)


def opt_buffers(n, names, seed, p16):
    """16-byte aligned device buffers of n + 8 elements each: the 8 guard elements must come back bit-identical"""
    g = gen(seed)
    host = {k: (torch.randn(n + 8, generator=g) if k in ("p", "g0") else torch.zeros(n + 8)) for k in names}
    dev = {k: v.to(DEV) for k, v in host.items()}
    assert aligned(16, *dev.values())
    shadow = nan_buf(n + 8, BF16) if p16 else None
    return host, dev, shadow


def opt_finish(name, host, dev, shadow, n):
    for k in dev:
        assert_bits(f"{name} {k} guard", dev[k][n:], host[k][n:])
    if shadow is not None:
        assert_bits(f"{name} bf16 shadow", shadow[:n], dev["p"][:n].cpu().to(BF16))     # RNE of the p the device holds
        assert_guards(f"{name} bf16 shadow", shadow, torch.arange(n + 8) < n)


@pytest.mark.parametrize("n", OPT_SIZES)
def test_adam_step_vs_float64(ops, n):
    """torch.optim.Adam (L2 weight decay added to the gradient) restated in float64 from the same fp32 inputs, 3 steps: the
    float4 body, the scalar tail (n unpadded), the 2048-block cap with its second trip; weight decay 0 / 0.01, with and without
    the bf16 shadow, a clip coefficient below 1 on the second step; a non-finite norm leaves everything bit-identical"""
    assert n % 4 != 0 and (cdiv(n // 4, 256) > 2048) == (n == OPT_SIZES[-1])
    for wd, p16 in (OPT_OPTIONS if n < 10 ** 6 else OPT_OPTIONS[::3]):
        host, dev, shadow = opt_buffers(n, ("p", "m", "v"), n + int(wd * 100), p16)
        p, m, v = (host[k][:n].double() for k in ("p", "m", "v"))
        wd64 = f32v(wd)
        m_mag = torch.zeros(n, dtype=torch.float64)
        for step in (1, 2, 3):
            lr, coef = f32v(1e-3 * step), (f32v(0.4) if step == 2 else 1.0)
            st = opt_state(step, lr, coef, 1.0)
            gr = torch.randn(n + 8, generator=gen(1000 * step + n)) * (5.0 if step == 2 else 0.3)
            ops.adam_step(dev["p"][:n], gr.to(DEV)[:n], dev["m"][:n], dev["v"][:n], st.to(DEV), B1, B2, ADAM_EPS, wd, p16=None if shadow is None else shadow[:n])
            lr64, bc1, bc2 = float(st[1]), float(st[2]), float(st[3])
            gg = gr[:n].double() * coef + wd64 * p
            m_mag = B1 * m_mag + (1 - B1) * (gr[:n].double().abs() * coef + wd64 * p.abs())
            m = B1 * m + (1 - B1) * gg
            v = B2 * v + (1 - B2) * gg * gg
            p = p - (lr64 / bc1) * m / (v.sqrt() / math.sqrt(bc2) + ADAM_EPS)
        name = f"adam n={n} wd={wd} p16={p16}"
        check("ADAM_P_TOL", name + " p", dev["p"][:n], p, p.abs().clamp_min(lr64))
        check("ADAM_M_TOL", name + " m", dev["m"][:n], m, m_mag.clamp_min(1e-30))
        check("ADAM_V_TOL", name + " v", dev["v"][:n], v, v.clamp_min(1e-30))
        opt_finish(name, host, dev, shadow, n)
        # skip: a non-finite norm in state[4]
        snap = {k: t.clone() for k, t in dev.items()}
        snap16 = None if shadow is None else shadow.clone()
        ops.adam_step(dev["p"][:n], gr.to(DEV)[:n], dev["m"][:n], dev["v"][:n], opt_state(4, 1e-3, 0.0, INF).to(DEV), B1, B2,
                      ADAM_EPS, wd, p16=None if shadow is None else shadow[:n])
        for k in dev:
            assert_bits(f"{name} skipped {k}", dev[k], snap[k])
        if shadow is not None:
            assert_bits(f"{name} skipped shadow", shadow, snap16)


@pytest.mark.parametrize("n", OPT_SIZES)
def test_adadelta_step_vs_float64(ops, n):
    """torch.optim.Adadelta restated in float64 from the same fp32 inputs, 3 steps, eps from state[7]: the same paths and
    options as the Adam test"""
    assert n % 4 != 0 and (cdiv(n // 4, 256) > 2048) == (n == OPT_SIZES[-1])
    eps = f32v(1e-6)
    for wd, p16 in (OPT_OPTIONS if n < 10 ** 6 else OPT_OPTIONS[::3]):
        host, dev, shadow = opt_buffers(n, ("p", "sq", "acc"), n + 7 + int(wd * 100), p16)
        p, sq, acc = (host[k][:n].double() for k in ("p", "sq", "acc"))
        wd64 = f32v(wd)
        for step in (1, 2, 3):
            lr, coef = f32v(1.0 / step), (f32v(0.4) if step == 2 else 1.0)
            st = opt_state(step, lr, coef, 1.0, eps)
            gr = torch.randn(n + 8, generator=gen(2000 * step + n)) * (5.0 if step == 2 else 0.3)
            ops.adadelta_step(dev["p"][:n], gr.to(DEV)[:n], dev["sq"][:n], dev["acc"][:n], st.to(DEV), RHO, wd,
                              p16=None if shadow is None else shadow[:n])
            gg = gr[:n].double() * coef + wd64 * p
            sq = RHO * sq + (1 - RHO) * gg * gg
            delta = (acc + eps).sqrt() / (sq + eps).sqrt() * gg
            acc = RHO * acc + (1 - RHO) * delta * delta
            p = p - lr * delta
        name = f"adadelta n={n} wd={wd} p16={p16}"
        check("ADADELTA_P_TOL", name + " p", dev["p"][:n], p, p.abs().clamp_min(lr))
        check("ADADELTA_SQ_TOL", name + " square_avg", dev["sq"][:n], sq, sq.clamp_min(1e-30))
        check("ADADELTA_ACC_TOL", name + " acc_delta", dev["acc"][:n], acc, acc.clamp_min(1e-30))
        opt_finish(name, host, dev, shadow, n)
        snap = {k: t.clone() for k, t in dev.items()}
        snap16 = None if shadow is None else shadow.clone()
        ops.adadelta_step(dev["p"][:n], gr.to(DEV)[:n], dev["sq"][:n], dev["acc"][:n], opt_state(4, 1.0, 0.0, NAN, eps).to(DEV),
                          RHO, wd, p16=None if shadow is None else shadow[:n])
        for k in dev:
            assert_bits(f"{name} skipped {k}", dev[k], snap[k])
        if shadow is not None:
            assert_bits(f"{name} skipped shadow", shadow, snap16)
