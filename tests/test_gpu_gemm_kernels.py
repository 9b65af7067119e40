"""eamd_gemm on every dispatch path (csrc/gemm.hip, gemm_f32.hip, gemm_bf16.hip, gemm_direct.hip, gemm_persist.hip and
the shared epilogue store_c_tile of gemm_bf16_common.h), element-wise against float64.

route(desc) restates gemm_check's tile choice, eamd_gemm's branching, eamd_gemm_f32_dispatch and eamd_gemm_bf16_dispatch from
the descriptor that is launched (actual addresses, leading dimensions, strides, dtype, K, tile, tile count); every case names
the route it is meant to take and asserts it before the launch.

Operands are views inside larger NaN-filled allocations (bf16: 0x7FC0) with more than a row of slack on either side: the
columns between the extent and the leading dimension, the rows between batches and the slack stay NaN, and the result must be
finite and right.  Outputs are pre-filled (NaN where the launch overwrites, known non-zero values where it accumulates), have
ldc > N in most cases, and every element outside the [M, N] blocks must come back bit-identical.  Misalignment comes from
offset views of live allocations only.

The reference is float64 on the CPU from the same operand values (fp32 operands on the bf16 matrix cores: rounded to bf16
first; staged activations: float64 activation of the stored value, rounded to bf16 on the bf16 paths; gathers and row maps:
an index restatement of eamd_gather_t / eamd_rowmap_t as the header describes them).  The measured quantity per element is
|got - ref| / scale with scale = |alpha| sum_k |a_k| |b_k| + |alpha bias| + |R| + |beta C0| (times the activation's Lipschitz
factor where an epilogue applies one).  A contraction that only multiplies and adds in fp32 must sit under the a-priori
ceiling (K + splitk + 8) * 2^-23 of scale; above that every path family has a named constant, at most 4x the largest value
observed under its name on an MI355X (noted beside it), and every check prints an "[gemm] <constant> <route> <case>" line.
A bf16 output must be the RNE rounding of some fp32 value within the bound; fused-dropout keep patterns are judged bit for bit
against tests/dropout_restatement.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dropout_restatement as dr


pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
INF = float("inf")
U23 = 2.0 ** -23
EINVAL, EUNSUPPORTED = -1, -2
BF16, F32 = torch.bfloat16, torch.float32
ACT_NONE, ACT_RELU, ACT_SWISH, ACT_TANH, ACT_HARDTANH, ACT_SELU = range(6)
SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
LAYOUTS = {"NN": (0, 1), "NT": (0, 0), "TN": (1, 1), "TT": (1, 0)}      # name -> (transA, transB); B stored [N, K] is "T"

# ---- named bounds: |got - ref| / scale; observed = the largest value seen under the name on an MI355X -----------------
TOL_F32 = 1.2e-6            # pipelined fp32 kernel, no activation                           observed 3.25e-7
TOL_GENERIC = 1.2e-6        # generic kernel, either precision, no activation                observed 3.12e-7
TOL_BF16 = 5e-7             # bf16-operand kernel (products exact, fp32 accumulation)        observed 1.38e-7
TOL_DIRECT = 3e-7           # register-direct short-K kernel                                 observed 7.7e-8
TOL_PERSIST = 5e-7          # persistent kernel                                              observed 1.36e-7
TOL_SPLITK = 7.5e-7         # split-K atomics and accumulating launches, all three kernels   observed 1.94e-7
TOL_EPI_ACT = 7e-7          # swish / dswish epilogues and the h_act of the second output    observed 1.83e-7
TOL_STAGED_F32 = 1.7e-6     # staged relu / swish / tanh / hardtanh / selu, fp32 arithmetic  observed 4.34e-7
TOL_STAGED_BF16 = 8.5e-7    # staged relu / swish rounded to bf16                            observed 2.15e-7
TOL_ROWSTAT = 1.8e-7        # epilogue 7: tile sums of exp                                   observed 4.57e-8
TOL_ROWGRAD = 4.8e-7        # epilogue 8: softmax-gradient rows                              observed 1.22e-7

OBSERVED = {}


@pytest.fixture(scope="module")
def lib():
    from espnet_amd import _lib
    _lib.lib()
    yield _lib
    for k in sorted(OBSERVED):
        print(f"[gemm] largest observed under {k}: {OBSERVED[k]:.3e} (constant {globals()[k]:g})")
    print("[gemm] routes reached:", ", ".join(sorted(ROUTES_SEEN)))


def cdiv(a, b):
    return -(-a // b)


def rup(a, m):
    return cdiv(a, m) * m


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ibits(t):
    """the bit patterns of an fp32 / bf16 tensor, on the CPU"""
    t = t.detach().contiguous().cpu()
    return t.view({F32: torch.int32, BF16: torch.int16}[t.dtype])


def unravel(i, shape):
    idx = []
    for n in reversed(shape):
        idx.insert(0, i % n)
        i //= n
    return tuple(idx)


def rne_bf16(x64):
    """float64 -> bf16 by round-to-nearest-even (through fp32: both roundings are monotonic)"""
    return x64.float().to(BF16)


def ceiling(K, splitk=1):
    """one ulp of error per multiply-add and per atomic add, in any order, plus the epilogue's handful of operations"""
    return (K + splitk + 8) * U23


def check(tolname, route_name, name, got, ref, scale, ceil=None):
    """max over elements of |got - ref| / scale in float64 with the worst element's index; a NaN in the result (an unwritten
    element, or poison that reached it) is an infinite error.  ceil: also assert the a-priori ceiling."""
    tol = globals()[tolname]
    g = got.detach().double().cpu().reshape(ref.shape)
    r = ref.detach().double()
    assert bool(torch.isfinite(r).all()), f"{name}: the reference is not finite"
    d = (g - r).abs()
    d = torch.where(torch.isfinite(g), d, torch.full_like(d, INF))
    s = scale.detach().double().expand_as(d)
    e = torch.where(d == 0, torch.zeros_like(d), d / s).reshape(-1)
    i = int(e.argmax()) if e.numel() else 0
    worst = float(e[i]) if e.numel() else 0.0
    idx = unravel(i, tuple(ref.shape))
    extra = "" if ceil is None else f", ceiling {ceil:.3g}"
    print(f"[gemm] {tolname} {route_name} {name}: max err/scale {worst:.3e} at {idx} (tol {tol:g}{extra})")
    if math.isfinite(worst):
        OBSERVED[tolname] = max(OBSERVED.get(tolname, 0.0), worst)
    assert worst <= tol, f"{name} [{route_name}]: element {idx} error/scale {worst:.3e} > {tolname} = {tol:g}"
    if ceil is not None:
        assert worst <= ceil, f"{name} [{route_name}]: element {idx} error/scale {worst:.3e} above the a-priori ceiling {ceil:.3g}"
    return worst


def check_bf16(tolname, route_name, name, got, ref, scale, ceil=None):
    """a bf16 output is the RNE rounding of an fp32 value within the bound of the float64 reference: by monotonicity it lies
    between RNE(ref - bound * scale) and RNE(ref + bound * scale)"""
    tol = globals()[tolname]
    bound = tol if ceil is None else min(tol, ceil)
    assert got.dtype == BF16
    g = got.detach().double().cpu().reshape(ref.shape)
    r = ref.detach().double()
    s = scale.detach().double().expand_as(r)
    lo, hi = rne_bf16(r - bound * s).double(), rne_bf16(r + bound * s).double()
    bad = ~((g >= lo) & (g <= hi))
    e = torch.where(bad, torch.where(torch.isfinite(g), (g - r).abs() / s, torch.full_like(r, INF)), torch.zeros_like(r)).reshape(-1)
    i = int(e.argmax()) if e.numel() else 0
    idx = unravel(i, tuple(ref.shape))
    print(f"[gemm] {tolname} {route_name} {name}: bf16 RNE interval at bound {bound:.3g}: {int(bad.sum())} of {r.numel()} outside, "
          f"{int((lo != hi).sum())} near a tie; worst outside at {idx}")
    assert not bool(bad.any()), (f"{name} [{route_name}]: element {idx} = {float(g.reshape(-1)[i])!r} is not the bf16 rounding of an "
                                 f"fp32 value within {bound:.3g} * scale of {float(r.reshape(-1)[i])!r}")


def assert_untouched(name, after, before, written):
    """every element of the flat buffer outside `written` (bool, CPU) holds the bits it held before the launch"""
    a, b = ibits(after).reshape(-1), ibits(before).reshape(-1)
    bad = (~written.reshape(-1)) & (a != b)
    assert not bool(bad.any()), f"{name}: guard element {int(bad.nonzero()[0])} of {a.numel()} was overwritten"


# ---- float64 activations ---------------------------------------------------------------------------------------------
def act64(x, act):
    if act == ACT_RELU:
        return x.clamp(min=0)
    if act == ACT_SWISH:
        return x * torch.sigmoid(x)
    if act == ACT_TANH:
        return torch.tanh(x)
    if act == ACT_HARDTANH:
        return x.clamp(-1, 1)
    if act == ACT_SELU:
        return SELU_SCALE * torch.where(x > 0, x, SELU_ALPHA * torch.expm1(x))
    return x


def dswish64(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def dact64(x, act):
    if act == ACT_RELU:
        return (x > 0).double()
    if act == ACT_SWISH:
        return dswish64(x)
    if act == ACT_TANH:
        return 1 - torch.tanh(x) ** 2
    if act == ACT_HARDTANH:
        return ((x > -1) & (x < 1)).double()
    if act == ACT_SELU:
        return SELU_SCALE * torch.where(x > 0, torch.ones_like(x), SELU_ALPHA * torch.exp(x))
    return torch.ones_like(x)


LIP = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_SWISH: 1.1, ACT_TANH: 1.0, ACT_HARDTANH: 1.0, ACT_SELU: SELU_SCALE * SELU_ALPHA}


# ---- the dispatcher, restated -----------------------------------------------------------------------------------------
def al16(addr):
    return addr is not None and addr % 16 == 0


def layout_of(p):
    return ("T" if p.transA else "N") + ("N" if p.transB else "T")


def tile_of(p):
    """gemm_check (gemm.hip): the tile of a descriptor with tile = 0"""
    if p.tile:
        return p.tile
    splitk = max(p.splitk, 1)
    t128 = cdiv(p.M, 128) * cdiv(p.N, 128) * p.batch1 * p.batch2 * splitk
    if p.in_dtype == 1:
        return 128 if (t128 >= 1024 and p.K >= 320 and p.M >= 2048 and p.N >= 256) else 64
    tile = 128 if (t128 >= (240 if p.precision == 0 else 512) and p.M >= 128 and p.N >= 128) else 64
    if p.precision == 0 and tile == 128 and 256 < t128 < 400 and splitk == 1:
        tile = 64
    return tile


def taps_fit(g):
    """gather_taps_small (gemm_f32.hip) / gather_taps_fit (gemm_bf16_common.h): the tap offsets travel as 4-bit fields"""
    return all(-8 <= g.dh[t] <= 7 and -8 <= g.dw[t] <= 7 for t in range(g.ntap))


def gather_nopad(g):
    """gather_nopad (gemm_f32.hip): no tap of any output pixel leaves the source"""
    return all(g.dh[t] >= 0 and (g.Ho - 1) * g.sh + g.dh[t] < g.Hin and g.dw[t] >= 0 and (g.Wo - 1) * g.sw + g.dw[t] < g.Win
               for t in range(g.ntap))


def stage_ok(p, unit):
    """a_ok, b_ok of eamd_gemm_f32_dispatch (unit 4) / eamd_gemm_bf16_dispatch (unit 8): 16-byte aligned chunk starts that stay
    inside the operand"""
    a_ok = (al16(p.A) and p.lda % unit == 0 and p.sA1 % unit == 0 and p.sA2 % unit == 0 and
            p.lda >= rup(p.M if p.transA else p.K, unit))
    b_ok = (al16(p.B) and p.ldb % unit == 0 and p.sB1 % unit == 0 and p.sB2 % unit == 0 and
            p.ldb >= rup(p.N if p.transB else p.K, unit))
    return a_ok, b_ok


def route_f32(p, tile):
    """eamd_gemm_f32_dispatch, launch_f, launch_f2 (gemm_f32.hip): the instantiation, or None for EAMD_EUNSUPPORTED"""
    if p.Cb or (p.Hb and not p.h_dtype) or p.aux_dtype or (not p.C and p.epilogue != 7):
        return None
    a_ok, b_ok = stage_ok(p, 4)
    act = 2 if (p.a_act > ACT_SWISH or p.b_act > ACT_SWISH) else (1 if (p.a_act or p.b_act) else 0)
    if p.gather.enabled:
        g = p.gather
        if g.C % 32 != 0 or not p.transB or not al16(p.A) or not b_ok or act or not taps_fit(g):
            return None
        if p.transA:
            return None if (g.C % tile != 0 or p.epilogue >= 7) else f"f32/{tile}/gatT"
        if gather_nopad(g) and p.epilogue < 7:                 # launch_f
            return f"f32/{tile}/gat/nopad"
        return None if p.epilogue >= 7 else f"f32/{tile}/gat"  # launch_f2: row epilogues for plain products only
    if not (a_ok and b_ok):
        return None
    if p.epilogue >= 7:                                        # launch_f2
        return f"f32/{tile}/NT/rowepi" if (layout_of(p) == "NT" and not act) else None
    return f"f32/{tile}/{layout_of(p)}/act{act}"


def route_bf16(p, tile):
    """eamd_gemm_bf16_dispatch, launch_b, launch_b2 (gemm_bf16.hip): the kernel, or the error code"""
    a_ok, b_ok = stage_ok(p, 8)
    act = bool(p.a_act or p.b_act)
    nb = p.batch1 * p.batch2
    if p.gather.enabled:
        g = p.gather
        if g.C % 64 != 0 or not p.transB or not al16(p.A) or not b_ok or act:
            return EINVAL
        if not taps_fit(g):
            return EUNSUPPORTED
        if p.transA and g.C % tile != 0:
            return EINVAL
        return f"bf16/{tile}/gatT" if p.transA else f"bf16/{tile}/gat"
    plain = (not p.bias and not p.aux and not p.R and not p.colsum and p.epilogue == 0 and p.beta == 0.0 and p.drop_p <= 0.0 and
             not act and not p.cmap.enabled)
    if (a_ok and b_ok and tile == 64 and not p.transA and not p.transB and p.K in (64, 128) and p.splitk == 1 and p.C and
            not p.Cb and not p.Hb and plain):
        return f"direct/K{p.K}"                                # eamd_gemm_bf16_direct
    if a_ok and b_ok and tile == 64:
        ntiles = cdiv(p.M, 64) * cdiv(p.N, 64)
        if (ntiles >= 512 and p.K > 0 and p.K % 256 == 0 and p.splitk == 1 and nb == 1 and not p.colsum and not act and
                not p.cmap.enabled and not p.transB and not p.aux and p.epilogue < 7):
            return f"persist/{layout_of(p)}"                   # eamd_gemm_bf16_persist
    fast = a_ok and b_ok
    if p.epilogue >= 7:                                        # launch_b2
        return f"bf16/{tile}/NT/rowepi" if (layout_of(p) == "NT" and fast and not act) else EUNSUPPORTED
    return f"bf16/{tile}/{layout_of(p)}/{'fast' if fast else 'slow'}" + ("/act" if act else "")


def route(p):
    """eamd_gemm (gemm.hip) behind gemm_check: the kernel a valid descriptor leaves through, or the code it returns"""
    tile = tile_of(p)
    if p.gather.enabled and p.colsum and (not p.transA or not p.transB or p.in_dtype != 0 or p.batch1 * p.batch2 != 1 or
                                          p.a_act or p.b_act):
        return EUNSUPPORTED                                    # gemm_check
    if p.in_dtype == 1:
        return route_bf16(p, tile)
    if p.precision == 1 and p.gather.enabled and p.transA and not p.Hb and p.drop_p == 0.0:
        r = route_f32(p, tile)                                 # eamd_gemm: gathered weight gradients keep exact fp32
        if r is not None:
            return r
    if p.precision == 0:
        r = route_f32(p, tile)
        if r is not None:
            return r
        if p.drop_p != 0.0 or p.Hb or p.a_act > ACT_SWISH or p.b_act > ACT_SWISH:
            return EUNSUPPORTED
    if p.epilogue >= 7 or (p.colsum and p.gather.enabled):
        return EUNSUPPORTED                                    # the generic kernel has neither
    return f"generic{tile}/p{p.precision}"


def store_path(p, coffs):
    """store_c_tile (gemm_bf16_common.h): which of its store loops a pipelined / bf16 launch with splitk = 1 runs"""
    hb_al = 16 if p.h_dtype else 8
    cvec = (p.ldc % 4 == 0 and all(c % 4 == 0 for c in coffs) and (not p.C or p.C % 16 == 0) and (not p.Cb or p.Cb % 8 == 0) and
            (not p.Hb or p.Hb % hb_al == 0) and (not p.R or (p.ldr % 4 == 0 and p.R % 16 == 0)) and
            (not p.aux or (p.ldaux % 4 == 0 and p.aux % 16 == 0)))
    if not cvec:
        return "scalar"
    general = (p.C and p.beta != 0.0) or p.cmap.enabled
    return ("vector" if general else "prefetch") + ("+tail" if p.N % 4 else "")


# ---- index restatements of eamd_gather_t / eamd_rowmap_t (include/espnet_amd.h) ----------------------------------------
def gather_matrix(src, g, nrows):
    """src [B, Hin, Win, C] float64 -> the [nrows, ntap * C] matrix whose row (b * Ho + i) * Wo + j holds, tap after tap, the
    C channels of source pixel (i * sh + dh[tap], j * sw + dw[tap]); out of range -> 0"""
    col = torch.zeros(nrows, g["ntap"] * g["C"], dtype=torch.float64)
    for r in range(nrows):
        j, t = r % g["Wo"], r // g["Wo"]
        i, b = t % g["Ho"], t // g["Ho"]
        for tap in range(g["ntap"]):
            hh, ww = i * g["sh"] + g["dh"][tap], j * g["sw"] + g["dw"][tap]
            if 0 <= hh < g["Hin"] and 0 <= ww < g["Win"]:
                col[r, tap * g["C"]:(tap + 1) * g["C"]] = src[b, hh, ww]
    return col


def rowmap_rows(cm, M):
    """physical row of every logical row m = (b * Ho + i) * Wo + j: (b * Hc + i * sh + oh) * Wc + j * sw + ow"""
    m = torch.arange(M)
    j, t = m % cm["Wo"], m // cm["Wo"]
    i, b = t % cm["Ho"], t // cm["Ho"]
    return (b * cm["Hc"] + i * cm["sh"] + cm["oh"]) * cm["Wc"] + j * cm["sw"] + cm["ow"]


# ---- buffers ----------------------------------------------------------------------------------------------------------
class Buf:
    """a flat allocation with the view at element `off`: host = the contents before the launch (CPU, fp32 values; NaN = poison)"""

    def __init__(self, host, off, dtype):
        self.off, self.dtype = off, dtype
        self.host = host.to(dtype)
        self.dev = self.host.to(DEV)
        self.before = self.host.clone()

    @property
    def addr(self):
        return self.dev.data_ptr() + self.off * self.dev.element_size()

    def cpu(self):
        return self.dev.detach().cpu()


def operand(g, rows, cols, ld, dtype, batch, strides, mis):
    """[b1, b2, rows, cols] N(0, 1) values (rounded to bf16 for bf16) stored with row stride ld and the batch strides inside a
    NaN-filled allocation: more than a row of slack before and after, `mis` elements off 32-byte alignment"""
    b1, b2 = batch
    s1, s2 = strides
    vals = torch.randn(b1, b2, rows, cols, generator=g)
    if dtype == BF16:
        vals = vals.to(BF16).float()
    slack = rup(max(ld, cols, 1) + 8, 8)
    span = (b1 - 1) * s1 + (b2 - 1) * s2 + (max(rows, 1) - 1) * ld + cols
    off = slack + mis
    host = torch.full((off + span + slack,), NAN)
    idx = (off + torch.arange(b1).view(-1, 1, 1, 1) * s1 + torch.arange(b2).view(1, -1, 1, 1) * s2 +
           torch.arange(rows).view(1, 1, -1, 1) * ld + torch.arange(cols).view(1, 1, 1, -1))
    host[idx.reshape(-1)] = vals.reshape(-1)
    return Buf(host, off, dtype), vals.double()


def result_buf(g, idx, span, dtype, mis, known, slack=72):
    """a result / residual / aux allocation: the elements `idx` (relative to the view) inside `span`, slack either side;
    known: N(0, 1) values everywhere (an accumulating output, a residual, aux), otherwise NaN everywhere"""
    off = slack + mis
    total = off + span + slack
    host = torch.randn(total, generator=g) if known else torch.full((total,), NAN)
    if dtype == BF16 and known:
        host = host.to(BF16).float()
    written = torch.zeros(total, dtype=torch.bool)
    written[off + idx.reshape(-1)] = True
    return Buf(host, off, dtype), written


def poison_outside(buf, written):
    """an input read only at `written`: everything else becomes NaN"""
    h = buf.host.float()
    h[~written] = NAN
    buf.host = h.to(buf.dtype)
    buf.dev = buf.host.to(DEV)
    buf.before = buf.host.clone()


def launch(lib, p, name):
    """eamd_gemm on the current stream, waited for; a device fault ends the session (nothing more may run on a faulted device)"""
    rc = lib.lib().eamd_gemm(C.byref(p), lib.stream_ptr())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{name}: the device reported {e}", returncode=3)
    return rc


# ---- one case ---------------------------------------------------------------------------------------------------------
def run_case(lib, name, expect, tolname, *, M, N, K, lay="NT", bf=False, precision=None, tile=64, batch=(1, 1), lda=None,
             ldb=None, a_mis=0, b_mis=0, sA=None, sB=None, ldc=None, c_mis=0, sC=None, alpha=1.0, beta=0.0, bias=False,
             R=False, r_mis=0, ldr=None, epilogue=0, aux=None, ldaux=None, aux_mis=0, a_act=0, b_act=0, splitk=1, colsum=False,
             out="C", cmap=None, gather=None, drop=None, Hb=False, h_act=0, ceil=True, seed=0, expect_store=None,
             expect_rc=0):
    """build the operands and outputs, assert the route, launch, compare every output element-wise with the float64
    reference and every other element of every output allocation bit for bit with what it held before"""
    from espnet_amd._lib import GemmT
    g = gen(seed * 7919 + M * 131 + N * 17 + K)
    ta, tb = LAYOUTS[lay]
    dt = BF16 if bf else F32
    unit = 8 if bf else 4
    if precision is None:
        precision = 1 if bf else 0
    b1, b2 = batch
    nb = b1 * b2

    p = GemmT()
    # ---- operands ----
    if gather is None:
        ar, ac = (K, M) if ta else (M, K)
        lda = rup(ac, unit) + unit if lda is None else lda
        sA = (b2 * (ar * lda + 2 * unit), ar * lda + 2 * unit) if sA is None else sA
        A, a_st = operand(g, ar, ac, lda, dt, batch, sA, a_mis)
        a64 = a_st.transpose(2, 3) if ta else a_st                        # [b1, b2, M, K]
    else:
        gt = gather
        nimg = gt["nb"]
        A, src = operand(g, nimg * gt["Hin"] * gt["Win"], gt["C"], gt["C"], dt, (1, 1), (0, 0), a_mis)
        src = src.reshape(nimg, gt["Hin"], gt["Win"], gt["C"])
        col = gather_matrix(src, gt, K if ta else M)
        a64 = (col.t() if ta else col).reshape(1, 1, M, K)
        lda, sA = gt["C"] * gt["ntap"], (0, 0)
        pg = p.gather
        pg.enabled, pg.C, pg.ntap, pg.Ho, pg.Wo, pg.Hin, pg.Win, pg.sh, pg.sw = (1, gt["C"], gt["ntap"], gt["Ho"], gt["Wo"],
                                                                                gt["Hin"], gt["Win"], gt["sh"], gt["sw"])
        for t in range(gt["ntap"]):
            pg.dh[t], pg.dw[t] = gt["dh"][t], gt["dw"][t]
    br, bc = (K, N) if tb else (N, K)
    ldb = rup(bc, unit) + unit if ldb is None else ldb
    sB = (b2 * (br * ldb + 2 * unit), br * ldb + 2 * unit) if sB is None else sB
    Bm, b_st = operand(g, br, bc, ldb, dt, batch, sB, b_mis)
    b64 = b_st if tb else b_st.transpose(2, 3)                             # [b1, b2, K, N]

    # ---- result geometry ----
    ldc = rup(N, 4) + 4 if ldc is None else ldc
    ldr = ldc + 4 if ldr is None else ldr
    ldaux = ldc + 8 if ldaux is None else ldaux
    if cmap is not None:
        prow = rowmap_rows(cmap, M)
        nphys = (M // (cmap["Ho"] * cmap["Wo"])) * cmap["Hc"] * cmap["Wc"]
        pm = p.cmap
        pm.enabled, pm.Ho, pm.Wo, pm.Hc, pm.Wc, pm.sh, pm.oh, pm.sw, pm.ow = (1, cmap["Ho"], cmap["Wo"], cmap["Hc"], cmap["Wc"],
                                                                              cmap["sh"], cmap["oh"], cmap["sw"], cmap["ow"])
    else:
        prow, nphys = torch.arange(M), M
    ldmax = max(ldc, ldr if R else 0, ldaux if aux else 0)
    sC = (b2 * (nphys * ldmax + 4), nphys * ldmax + 4) if sC is None else sC
    coffs = [i1 * sC[0] + i2 * sC[1] for i1 in range(b1) for i2 in range(b2)]
    coff_t = torch.tensor(coffs).view(nb, 1, 1)

    def block_idx(ld):
        return coff_t + prow.view(1, M, 1) * ld + torch.arange(N).view(1, 1, N)

    def span_of(ld):
        return coffs[-1] + (nphys - 1) * ld + N

    accumulate = splitk > 1 or beta != 0.0
    outs = {}
    if out in ("C", "both"):
        outs["C"] = result_buf(g, block_idx(ldc), span_of(ldc), F32, c_mis, accumulate)
    if out in ("Cb", "both"):
        outs["Cb"] = result_buf(g, block_idx(ldc), span_of(ldc), BF16, c_mis, False)
    if Hb:
        outs["Hb"] = result_buf(g, block_idx(ldc), span_of(ldc), BF16 if bf else F32, 0, False)
    c0 = torch.zeros(nb, M, N, dtype=torch.float64)
    if accumulate and "C" in outs:
        c0 = outs["C"][0].host[outs["C"][0].off + block_idx(ldc)].double()
    r64 = torch.zeros(nb, M, N, dtype=torch.float64)
    if R:
        Rb, rw = result_buf(g, block_idx(ldr), span_of(ldr), F32, r_mis, True)
        poison_outside(Rb, rw)
        r64 = Rb.host[Rb.off + block_idx(ldr)].double()
    x64 = None
    if aux:
        Xb, xw = result_buf(g, block_idx(ldaux), span_of(ldaux), BF16 if aux == "bf16" else F32, aux_mis, True)
        poison_outside(Xb, xw)
        x64 = Xb.host[Xb.off + block_idx(ldaux)].double()
    bias64 = torch.zeros(N, dtype=torch.float64)
    if bias:
        Bi, bw = result_buf(g, torch.arange(N), N, F32, 1, True)
        poison_outside(Bi, bw)
        bias64 = Bi.host[Bi.off:Bi.off + N].double()
    ncs = N if gather is not None else nb * M
    if colsum:
        Cs, csw = result_buf(g, torch.arange(ncs), ncs, F32, 1, True, slack=264)      # two 128-row tiles of guard
        cs0 = Cs.host[Cs.off:Cs.off + ncs].double()

    # ---- descriptor ----
    p.A, p.B = A.addr, Bm.addr
    p.C = outs["C"][0].addr if "C" in outs else None
    p.Cb = outs["Cb"][0].addr if "Cb" in outs else None
    p.bias = Bi.addr if bias else None
    p.R = Rb.addr if R else None
    p.aux = Xb.addr if aux else None
    p.aux_dtype = 1 if aux == "bf16" else 0
    p.colsum = Cs.addr if colsum else None
    p.M, p.N, p.K, p.transA, p.transB = M, N, K, ta, tb
    p.lda, p.ldb, p.ldc, p.ldaux, p.ldr = lda, ldb, ldc, ldaux, ldr
    p.batch1, p.batch2 = b1, b2
    p.sA1, p.sA2 = sA
    p.sB1, p.sB2 = sB
    p.sC1, p.sC2 = sC
    p.alpha, p.beta = alpha, beta
    p.a_act, p.b_act, p.epilogue, p.splitk = a_act, b_act, epilogue, splitk
    p.in_dtype, p.precision, p.tile = int(bf), precision, tile
    step = None
    if drop is not None:
        step = torch.tensor([drop[2]], dtype=torch.int64, device=DEV)
        p.drop_p, p.drop_salt, p.drop_step = drop[0], drop[1], step.data_ptr()
        if Hb:
            p.Hb, p.h_act, p.h_dtype = outs["Hb"][0].addr, h_act, 0 if bf else 1

    got_route = route(p)
    assert got_route == expect, f"{name}: the dispatcher takes {got_route!r}, the case is written for {expect!r}"
    rname = str(got_route)
    pipelined = isinstance(got_route, str) and not got_route.startswith("generic") and not got_route.startswith("direct")
    if expect_store is not None and pipelined and splitk == 1:
        sp = store_path(p, coffs)
        assert sp == expect_store, f"{name}: store_c_tile takes its {sp} path, the case is written for {expect_store}"

    rc = launch(lib, p, name)
    assert rc == expect_rc, f"{name}: eamd_gemm returned {rc}, expected {expect_rc}"
    if expect_rc != 0:
        for k, (buf, written) in outs.items():
            assert_untouched(f"{name} {k}", buf.cpu(), buf.before, torch.zeros_like(written))
        return None

    # ---- reference ----
    round_ops = bf or (rname.startswith("generic") and rname.endswith("p1"))
    a = a64.reshape(nb, M, K)
    b = b64.reshape(nb, K, N)
    a_raw = a
    if a_act:
        a = act64(a, a_act)
    if b_act:
        b = act64(b, b_act)
    if round_ops:
        a, b = rne_bf16(a).double(), rne_bf16(b).double()
    acc = torch.bmm(a, b) if K else torch.zeros(nb, M, N, dtype=torch.float64)
    unrounded = torch.bmm(act64(a_raw, a_act), act64(b64.reshape(nb, K, N), b_act)) if (round_ops and not bf and K) else None
    mag = torch.bmm(a.abs(), b.abs()) if K else torch.zeros(nb, M, N, dtype=torch.float64)
    v = acc + bias64
    fac = torch.ones_like(v)
    if splitk > 1:
        ref = c0 + alpha * v + r64
        scale = abs(alpha) * (mag + bias64.abs()) + r64.abs() + c0.abs()
    else:
        if epilogue == 1:
            v = v.clamp(min=0)
        elif epilogue == 2:
            v, fac = act64(v, ACT_SWISH), fac * LIP[ACT_SWISH]
        elif epilogue == 3:
            v = torch.where(x64 > 0, v, torch.zeros_like(v))
        elif epilogue == 4:
            v, fac = v * dswish64(x64), fac * 1.1
        elif epilogue == 5:
            v, fac = v * x64, fac * x64.abs()
        h64 = None
        if drop is not None:
            thr = dr.drop_thr16(drop[0])
            inv = float(dr.drop_inv(thr))
            keep = torch.from_numpy(dr.keep_bits(drop[2], drop[1], M * N) >= np.uint32(thr)).view(1, M, N)
            if Hb:
                h64 = torch.where(keep, act64(v, h_act) * inv, torch.zeros_like(v))
                if epilogue == 6:
                    v, fac = torch.where(keep, dact64(v, h_act) * inv, torch.zeros_like(v)), None
            else:
                v, fac = torch.where(keep, v * inv, torch.zeros_like(v)), fac * inv
        ref = alpha * v + r64 + beta * c0
        if fac is None:        # epilogue 6: the stored factor is O(1 / (1 - p)) whatever the product's magnitude
            scale = abs(alpha) * inv * LIP[h_act] * (1 + mag + bias64.abs()) + r64.abs() + (beta * c0).abs()
        else:
            scale = abs(alpha) * fac * (mag + bias64.abs()) + r64.abs() + (beta * c0).abs()
    scale = scale.clamp(min=1e-30)
    cl = ceiling(K, splitk) if ceil else None

    for k, (buf, written) in outs.items():
        after = buf.cpu()
        assert_untouched(f"{name} {k}", after, buf.before, written)
        got = after[buf.off + block_idx(ldc)]
        if k == "Hb":
            hs = (abs(inv) * LIP[h_act] * (mag + bias64.abs())).clamp(min=1e-30)
            (check_bf16 if bf else check)("TOL_EPI_ACT" if h_act else tolname, rname, f"{name} Hb", got, h64, hs)
            assert bool(((got.double() == 0) | keep).all()), f"{name}: Hb has a value where the restated mask drops"
        elif k == "Cb":
            check_bf16(tolname, rname, f"{name} Cb", got, ref, scale, cl)
        else:
            check(tolname, rname, f"{name} C", got, ref, scale, cl)
            if unrounded is not None and epilogue == 0 and splitk == 1:
                # witness of the route: fp32 operands that went through the bf16 matrix cores were rounded on the way (2^-9
                # per operand), so the result is NOT the un-rounded product to fp32 accuracy
                far = ((got.double().reshape(nb, M, N) - (alpha * (unrounded + bias64) + r64 + beta * c0)).abs() / scale).max()
                assert float(far) > 1e-5, f"{name} [{rname}]: the operands were not rounded to bf16 ({float(far):.2e})"
        if drop is not None and k != "Hb" and not R and beta == 0.0 and (not Hb or epilogue == 6):
            # the keep pattern bit for bit: a dropped element is exactly zero, a kept one is not (values are never 0 here)
            z = got.double().reshape(1, M, N) == 0
            ok = (z == ~keep) | (ref == 0)
            assert bool(ok.all()), f"{name}: keep pattern differs from the restatement at {unravel(int((~ok).reshape(-1).nonzero()[0]), (M, N))}"
    if colsum:
        after = Cs.cpu()
        assert_untouched(f"{name} colsum", after, Cs.before, csw)
        if gather is not None:      # column sums of B
            s_ref, s_mag = b64.reshape(K, N).sum(0), b64.reshape(K, N).abs().sum(0)
        else:                       # of A as stored, before a_act
            s_ref, s_mag = a_raw.sum(2).reshape(-1), a_raw.abs().sum(2).reshape(-1)
        check(tolname, rname, f"{name} colsum", after[Cs.off:Cs.off + ncs], cs0 + alpha * s_ref,
              (abs(alpha) * s_mag + cs0.abs()).clamp(min=1e-30), ceiling(K, splitk) if ceil else None)
    return got_route


ROUTES_SEEN = set()


def case(lib, name, expect, tolname, **kw):
    r = run_case(lib, name, expect, tolname, **kw)
    ROUTES_SEEN.add(str(expect))
    return r


# =============================================================================================
# 1. K-loop depth: every tail phase of every ring, ragged last tiles, all four layouts, K = 0
# =============================================================================================
def depth_ks(bk, unit, nkts):
    """K values for `nkt` K-tiles: whole tiles, 1 short, a multiple of the chunk short, 1 element into the last tile, and
    K % chunk != 0 (the chunk that straddles K is masked, not dropped: the default leading dimension is round(K) + chunk, the
    straddling one is stored with ld = round(K) exactly by the caller)"""
    ks = []
    for nkt in nkts:
        if nkt == 0:
            ks.append((0, False))
            continue
        ks += [(nkt * bk, False), (nkt * bk - 1, False), (nkt * bk - 3 * unit, False), ((nkt - 1) * bk + 1, False),
               (nkt * bk - unit - 2, True)]
    return ks


DEPTH_ROUTES = [
    # id, bf16 operands, tile, elements A is off alignment, route (layout to fill in), constant
    ("f32-64", False, 64, 0, "f32/64/{}/act0", "TOL_F32"),
    ("f32-128", False, 128, 0, "f32/128/{}/act0", "TOL_F32"),
    ("bf16-64", True, 64, 0, "bf16/64/{}/fast", "TOL_BF16"),
    ("bf16-128", True, 128, 0, "bf16/128/{}/fast", "TOL_BF16"),
    ("generic64", False, 64, 1, "generic64/p0", "TOL_GENERIC"),
]


@pytest.mark.parametrize("rid,bf,tile,mis,stem,tol", DEPTH_ROUTES, ids=[r[0] for r in DEPTH_ROUTES])
def test_k_loop_depth(lib, rid, bf, tile, mis, stem, tol):
    bk, unit = (64, 8) if bf else (32, 4)
    nkts = list(range(0, 11)) + ([14, 15] if bf else [14, 15, 16])
    M = N = tile + 1
    for K, tight in depth_ks(bk, unit, nkts):
        ld = {"lda": max(rup(K, unit), unit), "ldb": max(rup(K, unit), unit)} if tight or K == 0 else {}
        # direct kernel: a plain NT product at K = 64 / 128 on the 64 tile; a bias keeps the case on the general kernel
        bias = bf and tile == 64 and K in (64, 128)
        case(lib, f"depth {rid} K={K}", stem.format("NT"), tol, M=M, N=N, K=K, bf=bf, tile=tile, a_mis=mis, bias=bias,
             alpha=1.0 if K else 0.75, R=(K == 0), beta=0.5 if K == 0 else 0.0, **ld)
    for lay in ("NN", "TN", "TT"):
        for nkt in (3, 7, 9):
            K = nkt * bk - unit - 1
            case(lib, f"depth {rid} {lay} K={K}", stem.format(lay), tol, M=M, N=N, K=K, lay=lay, bf=bf, tile=tile, a_mis=mis)


def test_k_zero_is_the_epilogue_alone(lib):
    """K = 0: the result is alpha * bias + R + beta * C0 on every route (the persistent kernel must not take it)"""
    for bf, tile, mis, expect, tol in ((False, 64, 0, "f32/64/NT/act0", "TOL_F32"), (False, 128, 0, "f32/128/TN/act0", "TOL_F32"),
                                       (True, 64, 0, "bf16/64/NT/fast", "TOL_BF16"), (True, 128, 1, "bf16/128/TN/slow", "TOL_BF16"),
                                       (False, 64, 1, "generic64/p0", "TOL_GENERIC"), (False, 128, 1, "generic128/p1", "TOL_GENERIC")):
        lay = expect.split("/")[2] if expect.count("/") > 1 else "NT"
        case(lib, f"K=0 {expect}", expect, tol, M=tile + 1, N=tile + 1, K=0, lay=lay, bf=bf, tile=tile, a_mis=mis,
             precision=1 if (bf or expect.endswith("p1")) else 0, bias=True, R=True, alpha=-1.5, beta=0.5,
             lda=rup(tile + 1, 8) if lay == "TN" else 8, ldb=rup(tile + 1, 8) if lay == "TN" else 8)
    # 36 x 16 = 576 tiles of 64 x 64, K = 0 is a multiple of 256: the plain kernel, not the persistent one
    case(lib, "K=0 576 tiles", "bf16/64/NT/fast", "TOL_BF16", M=36 * 64 - 3, N=16 * 64 - 5, K=0, bf=True, tile=0, bias=True,
         lda=8, ldb=8)


# =============================================================================================
# 2. M / N edges, tile counts (XCD permutation), batches
# =============================================================================================
EDGES = [1, 3, 15, 16, 17, 61, 62, 63, 64, 65, 127, 129]
EDGE_ROUTES = [("f32", False, 0, "f32/64/{}/act0", "TOL_F32"), ("bf16", True, 0, "bf16/64/{}/fast", "TOL_BF16"),
               ("generic", False, 1, "generic64/p0", "TOL_GENERIC")]


@pytest.mark.parametrize("rid,bf,mis,stem,tol", EDGE_ROUTES, ids=[r[0] for r in EDGE_ROUTES])
def test_mn_edges(lib, rid, bf, mis, stem, tol):
    """every edge size as M and as N; the k-strided layouts with the leading dimension exactly round4 / round8 of the extent
    (the clamp (M - 1) & ~3)"""
    unit = 8 if bf else 4
    K = 64 + unit + 3 if bf else 32 + unit + 3
    for i, e in enumerate(EDGES):
        o = EDGES[(i * 5 + 3) % len(EDGES)]
        for lay in ("NT", "TN", "NN", "TT"):
            ta, tb = LAYOUTS[lay]
            for M, N in ((e, o), (o, e)):
                ld = {}
                if ta:
                    ld["lda"] = rup(M, unit)
                if tb:
                    ld["ldb"] = rup(N, unit)
                case(lib, f"edge {rid} {lay} {M}x{N}", stem.format(lay), tol, M=M, N=N, K=K, lay=lay, bf=bf, a_mis=mis, bias=True, **ld)


@pytest.mark.parametrize("rid,bf,mis,stem,tol", EDGE_ROUTES[:2], ids=[r[0] for r in EDGE_ROUTES[:2]])
def test_tile_counts_fill_the_result(lib, rid, bf, mis, stem, tol):
    """1..9, 15, 17 and 23 tiles at one K-tile: the XCD tile permutation must visit every tile (the result is pre-filled with NaN)"""
    for nt in list(range(1, 10)) + [15, 17, 23]:
        tm, tn = (nt, 1) if nt in (2, 3, 5, 7, 17, 23) else ((3, nt // 3) if nt % 3 == 0 else (2, nt // 2))
        if nt == 1:
            tm, tn = 1, 1
        case(lib, f"tiles {rid} {tm}x{tn}", stem.format("NT"), tol, M=tm * 64 - 5, N=tn * 64 - 3, K=31, bf=bf, R=bf)
        case(lib, f"tiles {rid} TN {tn}x{tm}", stem.format("TN"), tol, M=tn * 64 - 2, N=tm * 64 - 7, K=31, lay="TN", bf=bf)
    case(lib, f"tiles {rid} 128: 3x3", stem.format("NT").replace("64", "128"), tol, M=3 * 128 - 5, N=3 * 128 - 3, K=31, bf=bf, tile=128)
    case(lib, f"tiles {rid} 128: 5x1", stem.format("NT").replace("64", "128"), tol, M=5 * 128 - 5, N=100, K=31, bf=bf, tile=128)


def test_batches(lib):
    """(1,1), (3,1), (2,5) with operand strides that keep or break the % 4 / % 8 staging condition and sC % 4 both ways"""
    M, N = 65, 35
    for batch in ((1, 1), (3, 1), (2, 5)):
        b1, b2 = batch
        for bf in (False, True):
            unit = 8 if bf else 4
            K = 75 if bf else 43
            lda = rup(K, unit) + unit
            even = (b2 * (M * lda + 2 * unit), M * lda + 2 * unit)
            odd = (b2 * (M * lda + 2 * unit + 1), M * lda + 2 * unit + 1)
            ldc = 36
            for sAk, sCk in (("even", 0), ("even", 1), ("odd", 0)):
                sC = (b2 * (M * 44 + 4 + sCk), M * 44 + 4 + sCk)
                if batch == (1, 1) and (sAk, sCk) != ("even", 0):
                    continue
                fast = sAk == "even"
                if bf:
                    expect, tol = f"bf16/64/NT/{'fast' if fast else 'slow'}", "TOL_BF16"
                else:
                    expect, tol = ("f32/64/NT/act0", "TOL_F32") if fast else ("generic64/p0", "TOL_GENERIC")
                case(lib, f"batch {batch} {'bf16' if bf else 'f32'} sA {sAk} sC%4={sCk}", expect, tol, M=M, N=N, K=K, bf=bf,
                     batch=batch, lda=lda, sA=even if fast else odd, sC=sC, ldc=ldc, ldr=40, R=True, bias=True)


# =============================================================================================
# 3. Fallbacks: anything short of the 16-byte staging conditions
# =============================================================================================
def test_fallbacks(lib):
    """each of A and B: pointer off by one element, leading dimension not a multiple of 4 / 8, leading dimension below the
    rounded extent, odd batch stride -> generic kernel (fp32) / slow instantiation (bf16), still exact"""
    M, N = 67, 66
    for bf in (False, True):
        unit = 8 if bf else 4
        K = 64 + 13 if bf else 32 + 7           # K % unit != 0: the extent itself is a legal, shorter leading dimension
        for lay in ("NT", "TN"):
            ta, tb = LAYOUTS[lay]
            ea, eb = (M if ta else K), (N if tb else K)
            ra, rb = (K if ta else M), (K if tb else N)
            breaks = [("A ptr", dict(a_mis=1)), ("B ptr", dict(b_mis=1)),
                      ("lda % unit", dict(lda=rup(ea, unit) + unit + 1)), ("ldb % unit", dict(ldb=rup(eb, unit) + unit + 1)),
                      ("lda short", dict(lda=ea)), ("ldb short", dict(ldb=eb)),
                      ("sA odd", dict(batch=(2, 1), sA=(ra * (rup(ea, unit) + unit) + 2 * unit + 1, 0), lda=rup(ea, unit) + unit)),
                      ("sB odd", dict(batch=(2, 1), sB=(rb * (rup(eb, unit) + unit) + 2 * unit + 1, 0), ldb=rup(eb, unit) + unit))]
            for what, kw in breaks:
                if what.endswith("short") and (ea if what[2] == "a" else eb) % unit == 0:
                    continue
                expect, tol = (f"bf16/64/{lay}/slow", "TOL_BF16") if bf else ("generic64/p0", "TOL_GENERIC")
                case(lib, f"fallback {'bf16' if bf else 'f32'} {lay} {what}", expect, tol, M=M, N=N, K=K, lay=lay, bf=bf, **kw)
    for lay in LAYOUTS:      # all four slow layouts on either tile
        for tile in (64, 128):
            case(lib, f"fallback bf16 {tile} {lay}", f"bf16/{tile}/{lay}/slow", "TOL_BF16", M=tile + 2, N=tile + 1, K=150, lay=lay,
                 bf=True, tile=tile, b_mis=1)


def test_fp32_operands_on_bf16_matrix_cores(lib):
    """precision 1 with fp32 operands: the generic kernel rounds both operands to bf16 while staging (all four layouts, both
    tiles) - the reference rounds them first, so the fp32 bound applies; an aligned operand changes nothing"""
    for lay in LAYOUTS:
        for tile, mis in ((64, 0), (128, 1)):
            case(lib, f"p1 {lay} {tile}", f"generic{tile}/p1", "TOL_GENERIC", M=tile + 3, N=tile + 2, K=77, lay=lay, tile=tile,
                 precision=1, a_mis=mis, bias=True, alpha=0.5)
    case(lib, "p0 generic128", "generic128/p0", "TOL_GENERIC", M=131, N=130, K=77, tile=128, b_mis=1)


# =============================================================================================
# 4. Split-K
# =============================================================================================
def test_split_k(lib):
    """2, 3 and 4 slices over 5 and 7 ragged K-tiles (4 over 5: the last slice is empty), bias / R / alpha from the lead slice
    only, accumulated into a non-zero C; with colsum every slice adds its share"""
    for rid, bf, mis, stem, tol in (("f32", False, 0, "f32/64/{}/act0", "TOL_SPLITK"), ("bf16", True, 0, "bf16/64/{}/fast", "TOL_SPLITK"),
                                     ("generic", False, 1, "generic64/p0", "TOL_SPLITK")):
        bk = 64 if bf else 32
        for nkt in (5, 7):
            for sk in (2, 3, 4):
                K = nkt * bk - 5
                case(lib, f"splitk {rid} {sk} over {nkt}", stem.format("NT"), tol, M=65, N=70, K=K, bf=bf, b_mis=mis, splitk=sk,
                     bias=True, R=True, alpha=0.5)
                case(lib, f"splitk {rid} TN colsum {sk} over {nkt}", stem.format("TN"), tol, M=65, N=70, K=K, lay="TN", bf=bf,
                     b_mis=mis, splitk=sk, bias=True, alpha=0.5, colsum=True)
    case(lib, "splitk f32 128", "f32/128/TN/act0", "TOL_SPLITK", M=130, N=129, K=5 * 32 - 5, lay="TN", tile=128, splitk=4, colsum=True)
    case(lib, "splitk bf16 128", "bf16/128/TN/fast", "TOL_SPLITK", M=130, N=129, K=5 * 64 - 5, lay="TN", bf=True, tile=128, splitk=4,
         colsum=True)


# =============================================================================================
# 5. colsum
# =============================================================================================
COLSUM_ROUTES = [("f32", False, 0, "f32/{}/TN/act{}", "TOL_F32"), ("bf16", True, 0, "bf16/{}/TN/fast{}", "TOL_BF16"),
                 ("generic", False, 1, "generic{}/p0", "TOL_GENERIC")]


@pytest.mark.parametrize("rid,bf,mis,stem,tol", COLSUM_ROUTES, ids=[r[0] for r in COLSUM_ROUTES])
def test_colsum_of_a_as_stored(lib, rid, bf, mis, stem, tol):
    """transposed A, both tiles: M not a multiple of 4 / 8 with NaN in the padding columns, alpha != 1, two batches, a
    non-zero initial colsum; with a_act the sums are still those of A as stored (include/espnet_amd.h) on every kernel"""
    for tile in (64, 128):
        M = tile + 3
        K = 150 if bf else 75
        for a_act in (ACT_NONE, ACT_RELU, ACT_SWISH):
            if rid == "f32":
                expect = stem.format(tile, 1 if a_act else 0)
            elif rid == "bf16":
                expect = stem.format(tile, "/act" if a_act else "")
            else:
                expect = stem.format(tile)
            t = tol if not a_act else ("TOL_STAGED_BF16" if bf else "TOL_STAGED_F32")
            case(lib, f"colsum {rid} {tile} a_act={a_act}", expect, t, M=M, N=tile + 1, K=K, lay="TN", bf=bf, tile=tile, b_mis=mis,
                 alpha=-0.75, batch=(2, 1), colsum=True, a_act=a_act, ceil=not a_act)
    if rid == "f32":
        case(lib, "colsum f32 64 a_act=tanh", "f32/64/TN/act2", "TOL_STAGED_F32", M=67, N=65, K=75, lay="TN", alpha=-0.75,
             colsum=True, a_act=ACT_TANH, ceil=False)


# =============================================================================================
# 6. Epilogues
# =============================================================================================
EPI_ROUTES = [("f32", False, 0, "f32/64/NT/act0", "TOL_F32"), ("bf16", True, 0, "bf16/64/NT/fast", "TOL_BF16"),
              ("generic", False, 1, "generic64/p0", "TOL_GENERIC")]


@pytest.mark.parametrize("rid,bf,mis,expect,tol", EPI_ROUTES, ids=[r[0] for r in EPI_ROUTES])
def test_epilogues_and_store_paths(lib, rid, bf, mis, expect, tol):
    """epilogues 0..5 x {bias, residual with its own ldr, alpha, beta} through all four store loops of store_c_tile (and the
    generic kernel's scalar epilogue); aux in fp32 and bf16 with ldaux != ldc; C only, Cb only, both; stride-2 row maps"""
    M, K = 70, 100 if bf else 50
    paths = [("prefetch", dict(N=68, ldc=72)), ("prefetch+tail", dict(N=67, ldc=72)), ("vector", dict(N=68, ldc=72, beta=0.5)),
             ("vector+tail", dict(N=66, ldc=72, beta=-0.25)), ("scalar", dict(N=68, ldc=71)), ("scalar", dict(N=67, ldc=72, c_mis=1)),
             ("scalar", dict(N=68, ldc=72, r_mis=1, R=True)), ("scalar", dict(N=68, ldc=72, aux_mis=1, force_aux=True))]
    n = 0
    for epi in range(6):
        for path, kw in paths:
            kw = dict(kw)
            force_aux = kw.pop("force_aux", False)
            if force_aux and epi < 3:
                continue
            n += 1
            auxk = None if epi < 3 else ("bf16" if (bf and n % 2) else "f32")
            outk = "C" if not bf else ("C", "Cb", "both")[n % 3]
            if kw.get("beta") and outk == "Cb":
                outk = "both"
            kw.setdefault("R", n % 2 == 0)
            t = "TOL_EPI_ACT" if epi in (2, 4) else tol
            case(lib, f"epi {rid} {epi} {path} #{n}", expect, t, M=M, K=K, bf=bf, a_mis=mis, epilogue=epi, aux=auxk, out=outk,
                 bias=n % 3 != 0, alpha=1.0 if n % 4 == 0 else 0.75, ceil=epi not in (2, 4), expect_store=path, seed=n, **kw)
    # stride-2 scatter of the rows (the general vector loop), rows the map skips stay as they were
    cm = dict(Ho=5, Wo=7, Hc=11, Wc=15, sh=2, oh=1, sw=2, ow=0)
    for epi, N in ((0, 68), (3, 67), (1, 68)):
        case(lib, f"epi {rid} {epi} rowmap", expect, tol, M=2 * 35, N=N, ldc=72, K=K, bf=bf, a_mis=mis, epilogue=epi,
             aux="f32" if epi == 3 else None, cmap=cm, R=True, bias=True, expect_store="vector" + ("+tail" if N % 4 else ""),
             out="both" if bf else "C")
    case(lib, f"epi {rid} rowmap splitk", expect, "TOL_SPLITK", M=70, N=67, ldc=72, K=5 * (64 if bf else 32) - 3, bf=bf, a_mis=mis,
         cmap=cm, R=True, bias=True, splitk=2)
    if rid != "generic":
        e128 = expect.replace("64", "128")
        for path, kw in (("prefetch+tail", dict(N=131, ldc=136)), ("vector", dict(N=132, ldc=136, beta=0.5)), ("scalar", dict(N=131, ldc=135))):
            case(lib, f"epi {rid} 128 {path}", e128, "TOL_EPI_ACT", M=133, K=K, bf=bf, tile=128, epilogue=4, aux="bf16" if bf else "f32",
                 R=True, bias=True, alpha=0.75, out="both" if bf else "C", ceil=False, expect_store=path, **kw)


def row_case(lib, name, expect, tolname, *, bf, tile, M, N, K, epilogue, with_col, seed=0):
    """epilogues 7 (row statistics) and 8 (softmax-gradient rows): plain x W^T products with a bias"""
    from espnet_amd._lib import GemmT
    g = gen(1000 + seed + N)
    dt, unit = (BF16, 8) if bf else (F32, 4)
    lda = rup(K, unit) + unit
    A, a64 = operand(g, M, K, lda, dt, (1, 1), (0, 0), 0)
    Bm, b64 = operand(g, N, K, lda, dt, (1, 1), (0, 0), 0)
    a64, b64 = a64.reshape(M, K), b64.reshape(N, K)
    Bi, bw = result_buf(g, torch.arange(N), N, F32, 1, True)
    poison_outside(Bi, bw)
    bias64 = Bi.host[Bi.off:Bi.off + N].double()
    v = a64 @ b64.t() + bias64
    vs = (a64.abs() @ b64.abs().t() + bias64.abs()).clamp(min=1e-30)
    tn = cdiv(N, tile)
    fix = (0, N - 1, (N - 1) // 4 * 4)[seed % 3]            # the first column, the last, the start of the tail column group
    # labelled columns: the first, the last, one in the tail column group, none
    col = torch.randint(0, N, (M,), generator=g, dtype=torch.int32)
    col[0], col[1 % M], col[2 % M], col[3 % M] = 0, N - 1, (N - 1) // 4 * 4, -1
    cold = col.to(DEV)
    p = GemmT()
    p.A, p.B, p.bias = A.addr, Bm.addr, Bi.addr
    p.M, p.N, p.K, p.lda, p.ldb = M, N, K, lda, lda
    p.batch1 = p.batch2 = p.splitk = 1
    p.alpha, p.epilogue, p.tile, p.in_dtype, p.precision = 1.0, epilogue, tile, int(bf), int(bf)
    p.stats.fix = fix
    p.stats.col = cold.data_ptr() if with_col else None
    cl = ceiling(K)
    if epilogue == 7:
        part, pw = result_buf(g, torch.arange(M * tn * 2), M * tn * 2, F32, 1, False)
        zcol, zcw = result_buf(g, torch.arange(M)[col >= 0] if with_col else torch.arange(0), M, F32, 1, False)
        zfix, zfw = result_buf(g, torch.arange(M), M, F32, 1, False)
        p.stats.part, p.stats.zcol, p.stats.zfix = part.addr, zcol.addr, zfix.addr
        p.ldc = N
    else:
        ldc = rup(N, 4) + 4
        idx = torch.arange(M).view(M, 1) * ldc + torch.arange(N).view(1, N)
        Cf, cw = result_buf(g, idx, (M - 1) * ldc + N, F32, 0, False)
        outs = [(Cf, cw)]
        p.C, p.ldc = Cf.addr, ldc
        if bf:
            Cb, cbw = result_buf(g, idx, (M - 1) * ldc + N, BF16, 0, False)
            outs.append((Cb, cbw))
            p.Cb = Cb.addr
        rowc = torch.randn(M, 3, generator=g)
        rowc[:, 0] -= 4.0
        rowc[M // 2, 0] = -INF                    # a lattice node nothing passes through: a row of zeros
        rowcd, gsc = rowc.to(DEV), torch.tensor([0.5], device=DEV)
        p.stats.rowc, p.stats.gscale, p.stats.scale = rowcd.data_ptr(), gsc.data_ptr(), -1.25
    got_route = route(p)
    assert got_route == expect, f"{name}: the dispatcher takes {got_route!r}, the case is written for {expect!r}"
    ROUTES_SEEN.add(expect)
    rc = launch(lib, p, name)
    assert rc == 0, f"{name}: eamd_gemm returned {rc}"
    lc = col.long() if with_col else torch.full((M,), -1, dtype=torch.long)
    if epilogue == 7:
        for b, w, nm in ((part, pw, "part"), (zcol, zcw, "zcol"), (zfix, zfw, "zfix")):
            assert_untouched(f"{name} {nm}", b.cpu(), b.before, w)
        got = part.cpu()[part.off:part.off + M * tn * 2].reshape(M, tn, 2)
        for j in range(tn):
            vt, st = v[:, j * tile:(j + 1) * tile], vs[:, j * tile:(j + 1) * tile]
            mx, am = vt.max(1)
            check(tolname, expect, f"{name} max tile {j}", got[:, j, 0], mx, st.max(1).values, cl)
            se = torch.exp(vt - mx.view(-1, 1)).sum(1)
            # every exponent carries its logit's error; the sum is of positive terms
            check("TOL_ROWSTAT", expect, f"{name} sum exp tile {j}", got[:, j, 1], se, se * (1 + 2 * st.max(1).values))
        check(tolname, expect, f"{name} zfix", zfix.cpu()[zfix.off:zfix.off + M], v[:, fix], vs[:, fix], cl)
        if with_col:
            has = lc >= 0
            check(tolname, expect, f"{name} zcol", zcol.cpu()[zcol.off:zcol.off + M][has], v[has, lc[has]], vs[has, lc[has]], cl)
    else:
        tot, gb, gl = rowc[:, 0:1].double(), rowc[:, 1:2].double(), rowc[:, 2:3].double()
        sc = -1.25 * 0.5
        n = torch.arange(N).view(1, N)
        isfix, islc = (n == fix).double(), (n == lc.view(M, 1)).double()
        live = torch.isfinite(tot)
        ex = torch.where(live, torch.exp(v + torch.where(live, tot, torch.zeros_like(tot))), torch.zeros_like(v))
        ref = torch.where(live, sc * (ex - isfix * gb - islc * gl), torch.zeros_like(v))
        scale = (abs(sc) * (ex * (1 + 2 * vs) + isfix * gb.abs() + islc * gl.abs())).clamp(min=1e-30)
        for b, w in outs:
            after = b.cpu()
            assert_untouched(f"{name} C", after, b.before, w)
            got = after[b.off + idx]
            (check_bf16 if b.dtype == BF16 else check)("TOL_ROWGRAD", expect, name, got, ref, scale)
            assert bool((got[M // 2].double() == 0).all()), f"{name}: the row with tot = -inf is not zero"


def test_row_epilogues(lib):
    """epilogues 7 and 8 at N = tile - 1, tile + 1 and 2 tile + 3: the labelled column and `fix` in the first, the last and a
    tail column group; col = NULL; a row whose tot is -inf"""
    for bf in (False, True):
        for tile in (64, 128):
            expect = f"{'bf16' if bf else 'f32'}/{tile}/NT/rowepi"
            for i, N in enumerate((tile - 1, tile + 1, 2 * tile + 3)):
                for epi in (7, 8):
                    row_case(lib, f"epi {epi} {expect} N={N}", expect, "TOL_BF16" if bf else "TOL_F32", bf=bf, tile=tile,
                             M=tile + 5, N=N, K=150 if bf else 75, epilogue=epi, with_col=i != 1, seed=i)


def test_fused_dropout(lib):
    """fused dropout with N % 4 == 0 (eamd_drop_keep4) and N % 4 != 0 (the scalar eamd_drop_keep in the tail column group), with
    and without the second output, epilogue 6, fp32 (h_dtype 1) and bf16: keep patterns bit for bit against the restatement"""
    for bf, expect, tol in ((False, "f32/64/NT/act0", "TOL_F32"), (True, "bf16/64/NT/fast", "TOL_BF16")):
        K = 100 if bf else 50
        for N in (68, 67):
            base = dict(M=70, N=N, ldc=N, K=K, bf=bf, bias=True, alpha=0.75)
            case(lib, f"drop {expect} N={N}", expect, tol, drop=(0.1, 77, 5), out="both" if bf else "C", **base)
            case(lib, f"drop {expect} N={N} R", expect, tol, drop=(0.3, 78, 2 ** 33 + 5), R=True, ldr=N + 4, **base)
            case(lib, f"drop {expect} N={N} Hb", expect, tol, drop=(0.1, 79, 5), Hb=True, h_act=ACT_SWISH, **base)
            case(lib, f"drop {expect} N={N} Hb none", expect, tol, drop=(0.5, 80, 6), Hb=True, h_act=ACT_NONE, **base)
            case(lib, f"drop {expect} N={N} epi 6", expect, "TOL_EPI_ACT", drop=(0.1, 81, 7), Hb=True, h_act=ACT_SWISH, epilogue=6,
                 ceil=False, **base)


# =============================================================================================
# 7. Staged activations
# =============================================================================================
def test_staged_activations(lib):
    """relu and swish on A, on B and on both, all three kernels; tanh, hardtanh and selu on the pipelined fp32 kernel: ragged
    last K-tile (the masked zeros stay zero through the activation) and NaN padding"""
    for rid, bf, mis, stem in (("f32", False, 0, "f32/{}/{}/act1"), ("bf16", True, 0, "bf16/{}/{}/fast/act"), ("generic", False, 1, "generic{}/p0")):
        K = 3 * 64 - 11 if bf else 3 * 32 - 5
        for act in (ACT_RELU, ACT_SWISH):
            for which in ("a", "b", "ab"):
                for lay, tile in (("NT", 64), ("TN", 64), ("NN", 128), ("TT", 128), ("TN", 128), ("NT", 128)):
                    tol = "TOL_STAGED_BF16" if bf else "TOL_STAGED_F32"
                    case(lib, f"staged {rid} {lay} {tile} act {act} on {which}", stem.format(tile, lay), tol, M=tile + 2, N=tile + 1, K=K,
                         lay=lay, bf=bf, tile=tile, b_mis=mis, a_act=act if "a" in which else 0, b_act=act if "b" in which else 0,
                         ceil=False)
    case(lib, "staged generic p1 swish", "generic64/p1", "TOL_STAGED_BF16", M=66, N=65, K=91, precision=1, a_act=ACT_SWISH,
         b_act=ACT_RELU, ceil=False)
    for act in (ACT_TANH, ACT_HARDTANH, ACT_SELU):
        for lay, tile in (("NT", 64), ("TN", 128), ("NN", 64), ("TT", 64), ("NT", 128), ("TN", 64)):
            case(lib, f"staged f32 {lay} {tile} act {act}", f"f32/{tile}/{lay}/act2", "TOL_STAGED_F32", M=tile + 2, N=tile + 1, K=91,
                 lay=lay, tile=tile, a_act=act, b_act=ACT_RELU if lay == "NT" else act, ceil=False)
    # off the staging conditions there is no kernel for them
    case(lib, "staged tanh misaligned", EUNSUPPORTED, "TOL_F32", M=66, N=65, K=91, a_act=ACT_TANH, a_mis=1, expect_rc=EUNSUPPORTED)


# =============================================================================================
# 8. Gathers
# =============================================================================================
def conv_gather(C, nb, Hin, Win, pad, dh=None, dw=None):
    """3 x 3 stride-2 taps; pad: the taps start at -1 (negative and overhanging taps read as zero)"""
    o = -1 if pad else 0
    Ho = (Hin + 2 * pad - 3) // 2 + 1 + (1 if pad else 0)
    Wo = (Win + 2 * pad - 3) // 2 + 1 + (1 if pad else 0)
    return dict(C=C, ntap=9, nb=nb, Ho=Ho, Wo=Wo, Hin=Hin, Win=Win, sh=2, sw=2,
                dh=dh or [o + t // 3 for t in range(9)], dw=dw or [o + t % 3 for t in range(9)])


def test_gathers(lib):
    """implicit convolution: C = tile channels, a 3 x 3 stride-2 gather without padding (nopad), with negative and overhanging
    taps, row counts that are no multiple of the tile; the transposed form with split-K and more than 8 K-tiles (the poff
    ring wraps); tap offsets at the edges of the 4-bit packing, and one beyond them"""
    for bf in (False, True):
        for tile in (64, 128):
            fam, tol = ("bf16", "TOL_BF16") if bf else ("f32", "TOL_F32")
            for pad in (0, 1):
                gt = conv_gather(tile, 2, 11, 13, pad)
                rows = gt["nb"] * gt["Ho"] * gt["Wo"]
                expect = f"{fam}/{tile}/gat" + ("/nopad" if (not pad and not bf) else "")
                case(lib, f"gather {expect} pad={pad} rows={rows}", expect, tol, M=rows, N=tile + 3, K=9 * tile, lay="NN", bf=bf,
                     tile=tile, gather=gt, bias=True, R=True, epilogue=1)
                # transposed: the reduction runs over the rows (9+ K-tiles of 32 / 64), M = 9 C
                gt = conv_gather(tile, 7 if bf else 3, 23, 17, pad)
                rows = gt["nb"] * gt["Ho"] * gt["Wo"]
                assert cdiv(rows, 64 if bf else 32) > 8
                for sk in (1, 3):
                    case(lib, f"gatherT {fam}/{tile} pad={pad} K={rows} splitk={sk}", f"{fam}/{tile}/gatT", "TOL_SPLITK" if sk > 1 else tol,
                         M=9 * tile, N=70, K=rows, lay="TN", bf=bf, tile=tile, gather=gt, splitk=sk, beta=0.0 if sk > 1 else 1.0)
    # column sums of B (the convolution's bias gradient): pipelined fp32 kernel only, with and without split-K
    gt = conv_gather(64, 2, 11, 13, 1)
    rows = gt["nb"] * gt["Ho"] * gt["Wo"]
    for sk in (1, 2):
        case(lib, f"gatherT colsum splitk={sk}", "f32/64/gatT", "TOL_SPLITK", M=9 * 64, N=70, K=rows, lay="TN", gather=gt, splitk=sk,
             colsum=True, alpha=0.5, beta=1.0 if sk == 1 else 0.0)
    case(lib, "gatherT colsum bf16", EUNSUPPORTED, "TOL_BF16", M=9 * 64, N=70, K=rows, lay="TN", bf=True, gather=gt, colsum=True,
         expect_rc=EUNSUPPORTED)
    # fp32 operands asked for the bf16 matrix cores: the gathered weight gradient still takes the pipelined fp32 kernel, and
    # the numbers show it - they match the un-rounded product to fp32 accuracy
    case(lib, "gatherT precision 1", "f32/64/gatT", "TOL_F32", M=9 * 64, N=70, K=rows, lay="TN", gather=gt, precision=1, beta=1.0)
    case(lib, "gather precision 1", "generic64/p1", "TOL_GENERIC", M=rows, N=67, K=9 * 64, lay="NN", gather=gt, precision=1)
    # the edges of the 4-bit packing
    dh = [-8, 7, 0, -8, 7, 0, -8, 7, 0]
    dw = [-8, -8, -8, 7, 7, 7, 0, 0, 0]
    for bf in (False, True):
        gt = dict(C=64, ntap=9, nb=2, Ho=5, Wo=6, Hin=17, Win=19, sh=2, sw=2, dh=dh, dw=dw)
        fam, tol = ("bf16", "TOL_BF16") if bf else ("f32", "TOL_F32")
        case(lib, f"gather {fam} taps -8 / 7", f"{fam}/64/gat", tol, M=60, N=66, K=9 * 64, lay="NN", bf=bf, gather=gt)
        gt8 = dict(gt, dh=[8] + dh[1:])
        if bf:
            case(lib, "gather bf16 tap 8", EUNSUPPORTED, tol, M=60, N=66, K=9 * 64, lay="NN", bf=True, gather=gt8, expect_rc=EUNSUPPORTED)
        else:
            case(lib, "gather f32 tap 8", "generic64/p0", "TOL_GENERIC", M=60, N=66, K=9 * 64, lay="NN", gather=gt8)


# =============================================================================================
# 9. Direct and persistent kernels
# =============================================================================================
def test_direct_kernel(lib):
    """K = 64 and 128, M and N at the 32-row wave tile's and the 64 tile's edges, 1 / 7 / 8 / 9 batches (dealt to the XCDs
    eight at a time), alpha != 1; everything that must not take it, routed elsewhere and still right"""
    sizes = [1, 31, 32, 33, 64, 65, 130]
    for K in (64, 128):
        for i, M in enumerate(sizes):
            N = sizes[(i * 3 + 2) % len(sizes)]
            for M_, N_ in ((M, N), (N, M)):
                case(lib, f"direct K={K} {M_}x{N_}", f"direct/K{K}", "TOL_DIRECT", M=M_, N=N_, K=K, bf=True, alpha=-0.5)
        for batch in ((7, 1), (2, 4), (3, 3)):
            case(lib, f"direct K={K} batch {batch}", f"direct/K{K}", "TOL_DIRECT", M=33, N=65, K=K, bf=True, batch=batch, alpha=0.125)
    base = dict(M=65, N=33, K=64, bf=True)
    case(lib, "not direct: bias", "bf16/64/NT/fast", "TOL_BF16", bias=True, **base)
    case(lib, "not direct: beta", "bf16/64/NT/fast", "TOL_BF16", beta=0.5, **base)
    case(lib, "not direct: Cb", "bf16/64/NT/fast", "TOL_BF16", out="both", **base)
    case(lib, "not direct: transB", "bf16/64/NN/fast", "TOL_BF16", lay="NN", **base)
    case(lib, "not direct: K=96", "bf16/64/NT/fast", "TOL_BF16", **dict(base, K=96))
    case(lib, "not direct: tile 128", "bf16/128/NT/fast", "TOL_BF16", tile=128, **base)
    case(lib, "not direct: unaligned", "bf16/64/NT/slow", "TOL_BF16", a_mis=1, **base)


def test_persistent_kernel(lib):
    """more than 512 tiles of 64 x 64 with row and column remainders, K = 256 and 512, both operand layouts the dispatcher sends there (A as [M, K] and as [K, M]; B always [N, K]), a bias + residual + Cb
    epilogue; just below the thresholds (511 tiles; K = 320) the plain kernel runs"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # launch_persist: grid = CUs x occupancy, and 49 KiB of LDS per workgroup (SmemP) cap the occupancy at 3 of a CU's 160 KiB
    lds = 2 * 2 * 64 * 64 * 2 + 64 * 68 * 4
    grid_max = cus * ((160 * 1024) // lds)
    M, N = 2500, 2500
    assert cdiv(M, 64) * cdiv(N, 64) > grid_max, "no workgroup would walk a second tile"
    case(lib, "persist 2500x2500 K=512", "persist/NT", "TOL_PERSIST", M=M, N=N, K=512, bf=True, tile=0, bias=True, R=True, out="both")
    case(lib, "persist TT 2110x1100 K=256", "persist/TT", "TOL_PERSIST", M=2110, N=1100, K=256, lay="TT", bf=True, tile=0, alpha=0.5)
    case(lib, "persist NT 2110x1100 K=256", "persist/NT", "TOL_PERSIST", M=2110, N=1100, K=256, bf=True, tile=0, beta=0.5)
    case(lib, "persist TT 1100x2110 K=512", "persist/TT", "TOL_PERSIST", M=1100, N=2110, K=512, lay="TT", bf=True, tile=0, R=True,
         out="Cb")
    case(lib, "511 tiles", "bf16/64/NT/fast", "TOL_BF16", M=73 * 64 - 3, N=7 * 64 - 5, K=256, bf=True, tile=0)
    case(lib, "K=320", "bf16/64/NT/fast", "TOL_BF16", M=2110, N=1100, K=320, bf=True, tile=0)
