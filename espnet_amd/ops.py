"""Thin tensor-level wrappers over the C ABI (one Python function per kernel family).

No arithmetic happens here: every function validates shapes on the host (a faulting kernel can
take the whole GPU node down), fills the argument struct and launches on torch's current stream.
"""
import ctypes as C
import os
import math

import torch

from . import _lib
from ._lib import GatherT, GemmT, RowMapT, check, ptr, stream_ptr

ACT_NONE, ACT_RELU, ACT_SWISH = 0, 1, 2
EPI_NONE, EPI_RELU, EPI_SWISH, EPI_MUL_RELU_MASK, EPI_MUL_DSWISH, EPI_MUL_AUX, EPI_DACT_FACTOR, EPI_ROW_STATS, EPI_ROW_GRAD = 0, 1, 2, 3, 4, 5, 6, 7, 8

_PRECISIONS = {"fp32": 0, "bf16": 1}
_state = {"precision": 0}


def set_precision(name):
    """'fp32' -> v_mfma_f32_16x16x4_f32 (exact fp32 products, parity mode);
    'bf16' -> v_mfma_f32_16x16x32_bf16 (operands rounded to bf16 on load, fp32 accumulate)."""
    if name not in _PRECISIONS:
        raise ValueError(f"precision must be one of {list(_PRECISIONS)}")
    _state["precision"] = _PRECISIONS[name]


def get_precision():
    return [k for k, v in _PRECISIONS.items() if v == _state["precision"]][0]


def fast():
    """bf16 mode: GEMM operands (activations + weight shadows) live in HBM as bf16."""
    return _state["precision"] == 1


def f32_epilogue_drop():
    """fp32 mode: block-output dropout + residual ride in the epilogue of the pipelined fp32 GEMM (gemm_f32.hip); the
    operands of every block GEMM are 16-byte aligned with K % 4 == 0, which is all that kernel asks for"""
    return _state["precision"] == 0 and F32_EPILOGUE_DROP


F32_EPILOGUE_DROP = True     # tests flip this to compare against the stand-alone dropout kernel


def act_dtype():
    return torch.bfloat16 if fast() else torch.float32


def wshadow(p):
    """bf16 shadow of a parameter (fast mode) or the parameter itself (fp32 mode).
    FlatParams keeps an arena shadow that the Adam kernel refreshes; otherwise (or after an external
    in-place modification, detected through tensor._version) the shadow is re-cast on demand."""
    if not fast():
        return p
    sh = getattr(p, "_eamd_bf16", None)
    if sh is not None and getattr(p, "_eamd_bf16_ver", None) == p._version:
        return sh
    if sh is None:
        sh = torch.empty(p.shape, device=p.device, dtype=torch.bfloat16)
        p._eamd_bf16 = sh
    cast_bf16(p.detach().contiguous(), sh)
    p._eamd_bf16_ver = p._version
    return sh


def to_act(x):
    """fp32 activation -> GEMM operand dtype of the current mode"""
    if fast() and x.dtype == torch.float32:
        return cast_bf16(x.contiguous())
    return x


def to_act_shared(x):
    """to_act for a tensor that several consumers cast within one step (the encoder memory read by every decoder
    layer, the positional embedding read by every encoder layer): the bf16 copy rides on the tensor object"""
    if not (fast() and x.dtype == torch.float32):
        return x
    c = getattr(x, "_eamd_act", None)
    if c is not None and c[1] == x._version and c[0].shape == x.shape:
        return c[0]
    y = cast_bf16(x.contiguous())
    x._eamd_act = (y, x._version)
    return y


def _numel_from(t, off):
    return t.numel() - off


def _span(rows, ld, cols):
    """elements touched by a [rows, cols] matrix with leading dimension ld"""
    return (rows - 1) * ld + cols if rows > 0 else 0


# ---- time bound of a padded batch ---------------------------------------------------------------------------------
# A shape-bucketed graph (train.BucketedGraphStep) pads a batch's frame axis beyond its own longest utterance.  The
# reference never sees those frames, and three places of the Conformer encoder depend on the batch's own length: the
# legacy rel_shift (attention.py:160-171, taken over T' x T'), the depthwise convolution's zero padding and the BatchNorm
# statistics (convolution.py:56-79, over B x T' frames).  While a bound is set (device int32 scalar = the batch's own
# subsampled length, read by the kernels at run time, i.e. per graph replay) those three follow it.  The blocks read the
# bound in their FORWARD and keep it for their backward; the model clears it at the end of its forward pass.
_time_bound = {"t": None}


def set_time_bound(t):
    """t: int32 device tensor with one element, or None"""
    if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.numel() == 1):
        raise _lib.EamdError("time bound: one int32 element on the device")
    _time_bound["t"] = t


def time_bound():
    return _time_bound["t"]


def mask_time(x, T, bound):
    """rows (b, t) of the [B*T, C] tensor x with t >= bound[0] <- 0, in place"""
    rows = x.numel() // x.shape[-1]
    assert x.is_contiguous() and rows % T == 0 and x.dtype in (torch.float32, torch.bfloat16)
    check(_lib.lib().eamd_mask_time(ptr(x), rows, x.shape[-1], T, ptr(bound), x.dtype == torch.bfloat16,
                                    stream_ptr()), "eamd_mask_time")
    return x


# bench.py: list collecting every MFMA-contraction launch of one step as (descriptor or None, operand references,
# replay(stream_ptr)) - eamd_gemm descriptors and the fused attention kernels (descriptor None)
_gemm_record = None


def gemm(A, B, Cm, M, N, K, lda, ldb, ldc, *, transA=0, transB=0, bias=None, aux=None, ldaux=0, R=None,
         ldr=0, batch=(1, 1), sA=(0, 0), sB=(0, 0), sC=(0, 0), alpha=1.0, beta=0.0, a_act=0, b_act=0,
         epilogue=0, splitk=1, tile=0, gather=None, cmap=None, a_off=0, b_off=0, c_off=0, precision=None,
         colsum=None, Cb=None, drop=None, Hb=None, h_act=0, group=False, stats=None, defer=None):
    """A, B: both float32 or both bfloat16 (bf16 operands select the fast MFMA kernel).
    Cm: float32 result, or bfloat16 result (then no fp32 copy is written); Cb: extra bf16 copy.
    defer=list: the checked descriptor is appended to the list instead of being launched; gemm_multi(list) then issues
    all of them together (eamd_gemm_multi: independent products, e.g. the parity classes of a strided convolution's dX).
    group=True (weight gradients): while wgrad_group_begin() is in effect the launch is queued and leaves with all other
    queued ones as ONE grouped launch at wgrad_join() (eamd_gemm_group_*), if the library accepts it for that."""
    bf = A.dtype == torch.bfloat16
    if A.dtype != B.dtype or A.dtype not in (torch.float32, torch.bfloat16) or not (A.is_cuda and B.is_cuda):
        raise _lib.EamdError("gemm needs float32 or bfloat16 GPU operands of one dtype")
    if stats is not None:      # EPI_ROW_STATS: (part, col, zcol, zfix, fix), Cm = None;  EPI_ROW_GRAD: (rowc, col, fix, gscale, scale)
        assert epilogue in (EPI_ROW_STATS, EPI_ROW_GRAD) and tile in (64, 128) and splitk == 1
        assert (Cm is None and Cb is None) if epilogue == EPI_ROW_STATS else Cm is not None
    c32 = Cm if (Cm is not None and Cm.dtype == torch.float32) else None
    c16 = Cb if Cb is not None else (Cm if (Cm is not None and Cm.dtype == torch.bfloat16) else None)
    if c16 is not None and (c16.dtype != torch.bfloat16 or not bf):
        raise _lib.EamdError("gemm: bf16 outputs need bf16 operands")
    for tt in (R, bias, colsum):
        if tt is not None and tt.dtype != torch.float32:
            raise _lib.EamdError("gemm: bias / residual / colsum must be float32")
    b1, b2 = batch
    # ---- host-side bounds checks -------------------------------------------------------------
    if gather is None:
        a_span = _span(K, lda, M) if transA else _span(M, lda, K)
        a_need = a_off + (b1 - 1) * sA[0] + (b2 - 1) * sA[1] + a_span
        if a_need > A.numel():
            raise _lib.EamdError(f"gemm: A too small ({A.numel()} < {a_need})")
    b_span = _span(K, ldb, N) if transB else _span(N, ldb, K)
    b_need = b_off + (b1 - 1) * sB[0] + (b2 - 1) * sB[1] + b_span
    if b_need > B.numel():
        raise _lib.EamdError(f"gemm: B too small ({B.numel()} < {b_need})")
    if cmap is None:
        c_need = c_off + (b1 - 1) * sC[0] + (b2 - 1) * sC[1] + _span(M, ldc, N)
        for ct in (c32, c16):
            if ct is not None and c_need > ct.numel():
                raise _lib.EamdError(f"gemm: C too small ({ct.numel()} < {c_need})")
    if bias is not None and bias.numel() < N:
        raise _lib.EamdError("gemm: bias too small")

    p = GemmT()
    p.A, p.B = ptr(A, a_off), ptr(B, b_off)
    p.C = ptr(c32, c_off) if c32 is not None else None
    p.Cb = ptr(c16, c_off) if c16 is not None else None
    p.bias = ptr(bias)
    p.aux = ptr(aux, c_off) if aux is not None else None
    p.aux_dtype = 1 if (aux is not None and aux.dtype == torch.bfloat16) else 0
    p.R = ptr(R, c_off) if R is not None else None
    if colsum is not None:
        if gather is not None:       # gathered weight gradient: the column sums of B (eamd_gemm_t.colsum)
            if not (transA and transB) or bf or (b1, b2) != (1, 1) or colsum.numel() < N:
                raise _lib.EamdError("gemm: colsum with a gather needs transA, transB, float32 operands and N outputs")
        elif not transA or colsum.numel() < M * b1 * b2:
            raise _lib.EamdError("gemm: colsum needs transA and M outputs")
        p.colsum = ptr(colsum)
    p.M, p.N, p.K = M, N, K
    p.transA, p.transB = int(transA), int(transB)
    p.lda, p.ldb, p.ldc, p.ldaux, p.ldr = lda, ldb, ldc, ldaux or ldc, ldr or ldc
    p.batch1, p.batch2 = b1, b2
    p.sA1, p.sA2 = sA
    p.sB1, p.sB2 = sB
    p.sC1, p.sC2 = sC
    p.alpha, p.beta = alpha, beta
    p.a_act, p.b_act, p.epilogue = a_act, b_act, epilogue
    p.splitk = splitk
    p.in_dtype = 1 if bf else 0
    p.precision = 1 if bf else (_state["precision"] if precision is None else precision)
    p.tile = tile
    if stats is not None and epilogue == EPI_ROW_GRAD:
        rowc, col, fix, gscale, scale = stats
        if rowc.dtype != torch.float32 or rowc.numel() < 3 * M or col.dtype != torch.int32 or col.numel() < M or not (0 <= fix < N):
            raise _lib.EamdError("gemm: row-gradient coefficients too small or of the wrong dtype")
        p.stats.rowc, p.stats.col, p.stats.fix, p.stats.gscale, p.stats.scale = ptr(rowc), ptr(col), int(fix), ptr(gscale), float(scale)
    elif stats is not None:
        part, col, zcol, zfix, fix = stats
        tn = (N + tile - 1) // tile
        if part.dtype != torch.float32 or part.numel() < M * tn * 2 or zfix.numel() < M or not (0 <= fix < N) or \
                (col is not None and (col.dtype != torch.int32 or col.numel() < M or zcol is None or zcol.numel() < M)):
            raise _lib.EamdError("gemm: row-statistics buffers too small or of the wrong dtype")
        p.stats.part, p.stats.col, p.stats.zcol, p.stats.zfix, p.stats.fix = ptr(part), ptr(col), ptr(zcol), ptr(zfix), int(fix)
    if gather is not None:
        p.gather = gather
    if cmap is not None:
        p.cmap = cmap
    if drop is not None and drop[0] > 0.0:      # (p, salt): fused dropout, see include/espnet_amd.h
        if ldc != N or c_off != 0 or (not bf and p.precision != 0):
            raise _lib.EamdError("gemm: fused dropout needs a contiguous [M, N] result and bf16 or fp32-MFMA operands")
        p.drop_p, p.drop_salt = float(drop[0]), int(drop[1])
        p.drop_step = ptr(rng_state(A.device))
        if Hb is not None:
            if Hb.dtype != (torch.bfloat16 if bf else torch.float32) or Hb.numel() < M * N:
                raise _lib.EamdError("gemm: Hb must be an [M, N] buffer of the operand dtype")
            p.Hb, p.h_act, p.h_dtype = ptr(Hb), h_act, 0 if bf else 1
    if group and _wgroup["on"] and _in_grad_arena(Cm) and _wgroup_accepts(p):
        # Two queued problems that accumulate into the same dW may share one launch only if BOTH add with atomics:
        # splitk == 1 with beta == 1 is a plain read-modify-write of the tile, and workgroups of one launch are not
        # ordered (a weight used twice per backward pass with 65..511 reduction rows: per-step decoder cells, shared
        # parameters).  The earlier problems leave first (stream order keeps the sums exact); so does the queue when
        # the operands it keeps alive exceed GROUP_WGRAD_MAX_BYTES (streamed losses queue one weight gradient per chunk).
        lo = Cm.data_ptr() + 4 * c_off
        hi = lo + 4 * _span(M, ldc, N)
        nbytes = A.numel() * A.element_size() + B.numel() * B.element_size()
        clash = any(lo < qhi and qlo < hi and (splitk == 1 or qsk == 1) for qlo, qhi, qsk in _wgroup["ranges"])
        if clash or _wgroup["bytes"] + nbytes > GROUP_WGRAD_MAX_BYTES:
            wgrad_group_flush()
        _wgroup["items"].append((p, (A, B, Cm, colsum)))
        _wgroup["ranges"].append((lo, hi, splitk))
        _wgroup["bytes"] += nbytes
        return
    if defer is not None:
        defer.append((p, (A, B, Cm, bias, aux, R, colsum, Cb, Hb, stats)))
        return
    if _gemm_record is not None:
        _gemm_record.append((p, (A, B, Cm, bias, aux, R, colsum, Cb, Hb, stats),
                             lambda sp, p=p: check(_lib.lib().eamd_gemm(C.byref(p), sp), "eamd_gemm")))
    check(_lib.lib().eamd_gemm(C.byref(p), stream_ptr()), "eamd_gemm")


GEMM_MULTI_MAX = 4


def gemm_multi(items):
    """issue the products collected with gemm(..., defer=items) together: up to GEMM_MULTI_MAX per eamd_gemm_multi call (one
    launch where the library has a kernel for the combination, otherwise one launch each, in order)"""
    L = _lib.lib()
    for i0 in range(0, len(items), GEMM_MULTI_MAX):
        part = items[i0:i0 + GEMM_MULTI_MAX]
        arr = (GemmT * len(part))(*[it[0] for it in part])
        n = len(part)
        if _gemm_record is not None and any(it[0].in_dtype != 0 or it[0].precision != 0 for it in part):
            for p_, keep in part:          # no one-launch kernel for these operands: n launches, recorded as such
                _gemm_record.append((p_, keep, lambda sp, p_=p_: check(L.eamd_gemm(C.byref(p_), sp), "eamd_gemm")))
        elif _gemm_record is not None:
            _gemm_record.append((dict(kind="multi%d" % n, flop=sum(2.0 * it[0].M * it[0].N * it[0].K for it in part)),
                                 (arr, [it[1] for it in part]),
                                 lambda sp, arr=arr, n=n: check(L.eamd_gemm_multi(arr, n, sp), "eamd_gemm_multi")))
        check(L.eamd_gemm_multi(arr, n, stream_ptr()), "eamd_gemm_multi")


def conv2_bwd_x_conv1_bwd_w(items, x, dw, db):
    """the stride-parity classes of Conv2dSubsampling's second-convolution input gradient (collected with
    gemm(..., Cm=None, defer=items)) in one launch whose tiles are reduced to the FIRST convolution's weight / bias gradient
    instead of being stored (eamd_conv2_bwd_x_conv1_bwd_w).  x [B, T, F]: conv1's input; dw [C, 9] / db [C]: accumulated into."""
    L = _lib.lib()
    n = len(items)
    Bn, T, F = x.shape
    H1, W1 = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    Cc = items[0][0].N
    assert 1 <= n <= GEMM_MULTI_MAX and x.is_contiguous() and x.dtype == torch.float32
    assert dw.dtype == torch.float32 and db.dtype == torch.float32 and dw.numel() >= 9 * Cc and db.numel() >= Cc
    for p_, keep in items:            # rows of every class are (b, i, j) over the same B images; aux covers conv1's output
        assert p_.M == Bn * p_.cmap.Ho * p_.cmap.Wo and keep[4] is not None and keep[4].numel() >= Bn * H1 * W1 * p_.ldaux
    arr = (GemmT * n)(*[it[0] for it in items])
    part = torch.empty(sum((it[0].M + 127) // 128 for it in items) * 10 * Cc, device=x.device, dtype=torch.float32)
    args = (arr, n, ptr(x), T, F, ptr(part), ptr(dw), ptr(db))
    if _gemm_record is not None:
        _gemm_record.append((dict(kind="multi%d_c1w" % n, flop=sum(2.0 * it[0].M * it[0].N * it[0].K for it in items)),
                             (arr, [it[1] for it in items], x, part, dw, db),
                             lambda sp, args=args: check(L.eamd_conv2_bwd_x_conv1_bwd_w(*args, sp), "eamd_conv2_bwd_x_conv1_bwd_w")))
    check(L.eamd_conv2_bwd_x_conv1_bwd_w(*args, stream_ptr()), "eamd_conv2_bwd_x_conv1_bwd_w")


# ---- grouped weight-gradient launches ------------------------------------------------------------
# dW = dY^T X of a small layer (256 x 256 ... 768 x 256 outputs) is 16-48 tiles: even with split-K such a launch runs
# at a quarter of what the chip can do and costs a launch slot.  Nothing in backward reads dW, so between
# wgrad_group_begin() and wgrad_join() every eligible one is queued (operands kept alive) and all of them leave as ONE
# launch whose workgroups look their problem up in a device table (eamd_gemm_group_plan / eamd_gemm_group_launch).
GROUP_WGRAD = True            # tests flip this to reach the one-launch-per-GEMM path
STACK_WGRAD_MAX_ROWS = 64     # weight gradients of at most this many rows are stacked along the reduction until the flush (0: off)
GROUP_WGRAD_MAX_TILES = 384    # 64x64 output tiles: larger weight gradients fill the chip on their own
# measured at config 2 (DESIGN_HISTORY.md §B): grouping everything up to 384 output tiles (all but the vocabulary-sized
# gradients) with half the stand-alone split count is best in both precisions - 34.09 ms fp32 / 14.20 ms bf16 against
# 35.0 / 15.04 ungrouped; the queue supplies the parallelism the extra splits (and their atomics) bought before
GROUP_WGRAD_SK_DIV = 2
# fp32 operands only (measured: 33.45 -> 32.80 ms; with bf16 operands the 128x128 tile loses, 14.17 -> 14.3+ ms): problems
# of at least this many 64x64 tiles - the FFN weights - take 128x128 tiles in a second grouped launch, with about
# GROUP_WGRAD_T128_WGS workgroups (tiles x K-splits) each
GROUP_WGRAD_TILE128_MIN = 100
GROUP_WGRAD_T128_WGS = 96
# operand bytes the queue may keep alive before it is flushed early (the operands of every queued problem stay
# allocated until the grouped launch has been issued)
GROUP_WGRAD_MAX_BYTES = 16 << 30     # config 2 queues 4.6 GB per backward pass
_wgroup = {"on": False, "items": [], "ranges": [], "bytes": 0, "stack": {}, "pinned": [], "reserve": [], "arenas": {}}


def register_grad_arena(t):
    """only GEMMs that accumulate into a registered gradient arena (espnet_amd.train.FlatParams.grad) are queued: a
    temporary result (tap-major weight gradients that are permuted into the arena next, gradients handed back to
    autograd) is read by its consumer long before the grouped launch runs"""
    import weakref
    key = t.untyped_storage().data_ptr()
    _wgroup["arenas"][key] = weakref.ref(t)


def _in_grad_arena(t):
    """True if `t` lives in a registered gradient arena that is still alive (a freed arena's address may be handed to
    any later allocation)"""
    key = t.untyped_storage().data_ptr()
    ref = _wgroup["arenas"].get(key)
    if ref is None:
        return False
    a = ref()
    if a is None or a.untyped_storage().data_ptr() != key:
        del _wgroup["arenas"][key]
        return False
    return True


def wgrad_group_begin():
    _wgroup["on"] = GROUP_WGRAD
    _wgroup["items"], _wgroup["stack"] = [], {}      # nothing queued by a backward pass that ended in an exception survives
    _wgroup["ranges"], _wgroup["bytes"] = [], 0


def _wgroup_accepts(p):
    if ((p.M + 63) // 64) * ((p.N + 63) // 64) > GROUP_WGRAD_MAX_TILES:
        return False
    first = (C.c_int32 * 2)()
    return _lib.lib().eamd_gemm_group_plan(C.byref(p), 1, first) > 0


def _wgroup_staging(nbytes):
    """pinned host buffer for one descriptor table.  A captured graph copies from its buffer again at every replay, so
    a capture takes a buffer for good out of a small reserve that eager flushes (every capture is preceded by eager
    warm-up steps) keep topped up - pinned memory cannot be allocated while a stream is capturing."""
    if torch.cuda.is_current_stream_capturing():
        for i, h in enumerate(_wgroup["reserve"]):
            if h.numel() >= nbytes:
                _wgroup["pinned"].append(_wgroup["reserve"].pop(i))
                return _wgroup["pinned"][-1][:nbytes]
        return None
    want = (nbytes + 4095) // 4096 * 4096 * 2
    _wgroup["reserve"] = [h for h in _wgroup["reserve"] if h.numel() >= want]
    while len(_wgroup["reserve"]) < 16:
        _wgroup["reserve"].append(torch.empty(want, dtype=torch.uint8, pin_memory=True))
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)


def wgrad_group_flush():
    """launch everything queued so far: one grouped launch per tile size (a single queued GEMM goes out on its own)"""
    stack, _wgroup["stack"] = _wgroup["stack"], {}
    for dW, db, dys, xs in stack.values():          # stacked small-M weight gradients: one product per weight
        if len(dys) == 1:
            dyc, xc = dys[0], xs[0]
        else:
            dyc, xc = torch.cat(dys, 0), torch.cat(xs, 0)
        if dyc.shape[0] <= STACK_WGRAD_MAX_ROWS:    # still a handful of rows: straight to the GEMM
            sk = auto_splitk(dyc.shape[1], xc.shape[1], dyc.shape[0])
            gemm(dyc, xc, dW, dyc.shape[1], xc.shape[1], dyc.shape[0], dyc.shape[1], xc.shape[1], xc.shape[1], transA=1,
                 transB=1, splitk=sk, beta=1.0 if sk == 1 else 0.0, colsum=db, group=True)
        else:
            _linear_bwd_w(dyc, xc, dW, db=db)
    items = _wgroup["items"]
    if not items:
        return
    _wgroup["items"], _wgroup["ranges"], _wgroup["bytes"] = [], [], 0
    for tile in (64, 128):
        part = [it for it in items if (128 if it[0].tile == 128 else 64) == tile]
        if part:
            _wgroup_launch(part, tile)


def _wgroup_launch(items, tile):
    L = _lib.lib()

    def separately():
        for p, keep in items:
            if _gemm_record is not None:
                _gemm_record.append((p, keep, lambda sp, p=p: check(L.eamd_gemm(C.byref(p), sp), "eamd_gemm")))
            check(L.eamd_gemm(C.byref(p), stream_ptr()), "eamd_gemm")

    if len(items) == 1:
        return separately()
    n = len(items)
    dev = items[0][1][0].device
    arr = (GemmT * n)(*[it[0] for it in items])
    first = (C.c_int32 * (n + 1))()
    total = L.eamd_gemm_group_plan(arr, n, first)
    check(min(total, 0), "eamd_gemm_group_plan")
    nb_desc, nb_first = C.sizeof(arr), C.sizeof(first)
    host = _wgroup_staging(nb_desc + nb_first)
    if host is None:          # capturing with no staging buffer in reserve: one launch per GEMM
        return separately()
    C.memmove(host.data_ptr(), arr, nb_desc)
    C.memmove(host.data_ptr() + nb_desc, first, nb_first)
    tab = torch.empty(nb_desc + nb_first, dtype=torch.uint8, device=dev)
    tab.copy_(host, non_blocking=True)
    in_dtype = int(arr[0].in_dtype)
    args = (ptr(tab), ptr(tab, nb_desc), n, total, in_dtype, tile)
    check(L.eamd_gemm_group_launch(*args, stream_ptr()), "eamd_gemm_group_launch")
    if _gemm_record is not None:
        _gemm_record.append((dict(kind="group%d" % tile, flop=sum(2.0 * it[0].M * it[0].N * it[0].K * it[0].batch1 * it[0].batch2 for it in items)),
                             (tab, [it[1] for it in items]),
                             lambda sp, args=args: check(L.eamd_gemm_group_launch(*args, sp), "eamd_gemm_group_launch")))


def cast_bf16(x, out=None):
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    assert x.dtype == torch.float32 and x.is_contiguous() and out.numel() == x.numel()
    check(_lib.lib().eamd_cast_bf16(ptr(x), ptr(out), x.numel(), stream_ptr()), "eamd_cast_bf16")
    return out


def auto_splitk(m_out, n_out, k_red):
    """split count for reduction-heavy GEMMs (dW = dY^T X).  Measured on MI355X (tools/gemm_probe2.py,
    K = 7968): 128 output tiles -> 4, 32 tiles -> 8, 16 tiles -> 16 are the fastest; more splits lose to
    the f32 atomics, fewer leave CUs idle.  Powers of two >= 8 keep whole K-slices per XCD (gemm_bf16.hip:
    split index = workgroup id mod splitk)."""
    tiles = ((m_out + 63) // 64) * ((n_out + 63) // 64)
    if tiles >= 512:
        return 1
    want = 4.0 * (128.0 / tiles) ** 0.5
    s = 1
    while s < want:
        s *= 2
    return max(1, min(s, 64, max(1, k_red // 128)))


# ---- nn.Linear pieces -------------------------------------------------------------------------
LINEAR_ROWS = True      # eamd_linear_rows_f32 for few rows without autograd
_infer = 0      # > 0 inside an explicit inference region (ops.inference / @ops.inference_call: searches, F_.run's direct forward)


class inference:
    """marks an inference region: products of a handful of rows take eamd_linear_rows_f32 there.  NOT keyed on
    torch.is_grad_enabled(): grad mode is also off inside every autograd.Function.forward of a TRAINING step, where the few-row
    products (a small batch through the RNN decoder) must keep the summation order of the GEMMs used for their gradients."""

    def __enter__(self):
        global _infer
        _infer += 1

    def __exit__(self, *exc):
        global _infer
        _infer -= 1
        return False


def inference_call(fn):
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **k):
        with inference():
            return fn(*a, **k)
    return wrapped
# rows up to which it is used.  Beyond 16 rows the library has a one-wave-per-16x16-tile MFMA form (direct global loads, no LDS).
# Measured in the replayed step of a batched beam search (M = 320 rows, tools/trace_decode_graph.sh, round 4): 7.0 us against
# 13.1 us of the 64 x 64 tiles for N = 256 / 768 at K = 256 (those are 20 / 60 workgroups walking K alone), the same for N = 2048,
# SLOWER for K = 2048 (33 against 26 us with split-K: every wave re-reads its 32 rows of both operands) and for the output
# layer (N = 5000: 29.7 against 17.8 us) - so it takes the narrow products only
LINEAR_ROWS_MAX = 16
LINEAR_ROWS_BLOCK_MAX = 1024      # ... up to this many rows, K <= 512, N <= 1024
# ... and the long reductions (K >= 1024: the waves of a workgroup split K, one 16 x 16 tile per workgroup) - A/B knob
LINEAR_ROWS_KSPLIT = True


def linear_fwd(x, W, b, out=None, *, act=EPI_NONE, R=None, alpha=1.0, a_act=ACT_NONE, out_dtype=torch.float32,
               drop=None, Hb=None, h_act=ACT_NONE):
    """out[M,N] = alpha * drop(act(a_act(x)[M,K] @ W[N,K]^T + b)) + R      (x, W: both fp32 or both bf16)
    drop = (p, salt): dropout fused in the epilogue (bf16 operands); with Hb the value itself is left
    alone and Hb <- dropout(h_act(value)) is written as a second bf16 output."""
    M, K = x.shape
    N = W.shape[0]
    assert W.shape[1] == K and W.is_contiguous() and x.stride(1) == 1 and (R is None or R.stride(-1) == 1)
    if (LINEAR_ROWS and (M <= LINEAR_ROWS_MAX or (M <= LINEAR_ROWS_BLOCK_MAX and (K <= 512 or (K >= 1024 and LINEAR_ROWS_KSPLIT)) and N <= 1024
                                                  and K % 16 == 0)) and out is None and out_dtype == torch.float32 and x.dtype == torch.float32 and W.dtype == torch.float32
            and act in (EPI_NONE, EPI_RELU, EPI_SWISH) and a_act in (ACT_NONE, ACT_RELU, ACT_SWISH) and drop is None and Hb is None
            and K % 4 == 0 and _state["precision"] == 0 and _infer > 0 and not torch.is_grad_enabled()
            and (R is None or (tuple(R.shape) == (M, N) and (M == 1 or R.stride(0) >= N))) and (M == 1 or x.stride(0) >= K)):
        # (an expanded, stride-0 operand with M > 1 would read as `dense` on the C side: those go to the GEMM below via .contiguous())
        # inference on a handful of rows (one utterance's hypotheses in a beam step): one wave per output column; x and R may be
        # row-strided views (the newest position of every prefix)
        y = torch.empty(M, N, device=x.device, dtype=torch.float32)
        rc = _lib.lib().eamd_linear_rows_f32(ptr(x), ptr(W), ptr(b), ptr(R), ptr(y), M, N, K, a_act, act, alpha,
                                             x.stride(0), R.stride(0) if R is not None else 0, stream_ptr())
        if rc == 0:
            return y
        if rc != _lib.EAMD_EUNSUPPORTED:
            check(rc, "eamd_linear_rows_f32")
    x = x.contiguous()
    R = R.contiguous() if R is not None else None
    sk = 1
    if (out_dtype if out is None else out.dtype) == torch.float32 and act == EPI_NONE and drop is None and Hb is None:
        if R is None and alpha == 1.0:
            sk = _skinny_splitk(M, N, K)
        elif K >= 1024 and M <= 512 and x.is_cuda and torch.cuda.is_current_stream_capturing():
            # a beam-search step being captured: the second feed-forward product of a few (hundred) hypotheses walks K = 2048 in
            # 4 .. 20 workgroups, 58 us; eagerly the extra zero-fill launch costs the host more than the device saves, in a graph it
            # does not.  Bias, alpha and the residual come with the first K slice.
            sk = _skinny_splitk(M, N, K, max_rows=512)
    if out is None:
        out = zeros(M, N, device=x.device) if sk > 1 else torch.empty(M, N, device=x.device, dtype=out_dtype)
    elif sk > 1:
        out.zero_()
    gemm(x, W, out, M, N, K, K, K, N, bias=b, epilogue=act, R=R, ldr=N, alpha=alpha, a_act=a_act, drop=drop, Hb=Hb,
         h_act=h_act, splitk=sk)
    return out


# ---- zero arena --------------------------------------------------------------------------------------------------
# A decoder loop asks for hundreds of small zero-filled buffers per training step (split-K results that accumulate
# through atomics, gradient accumulators of the attention steps): 716 fill launches of 4 us at BASELINE config 4.
# Between zero_arena_begin() (the model's forward in training mode) and the next one, zeros() hands out fresh
# slices of ONE buffer that a single fill zeroed at begin; its size is the previous step's demand (the first step,
# and anything beyond the buffer, falls back to torch.zeros).  Slices are never handed out twice.
class _ZeroArena:
    buf = None
    off = 0
    need = 0        # bytes asked for since the last begin, counted only between a begin and the next begin / off
    cap = 0         # bytes the next arena gets
    active = False
    tracking = False
    capture = 0     # id of the stream capture zero_arena_begin ran in (0 = eager)


_zarena = _ZeroArena()
ZERO_ARENA = True
ZERO_ARENA_MAX = 1024 << 20     # larger demands go to torch.zeros


def _capture_id():
    """0 when the current stream is not capturing, else a number that tells captures apart (the buffer an arena hands out
    was zeroed by a fill INSIDE one capture, or eagerly: a slice may only be used where that fill runs too)"""
    if not torch.cuda.is_available() or not torch.cuda.is_current_stream_capturing():
        return 0
    try:
        from . import graphs
        return graphs.capture_id()
    except Exception:  # noqa: BLE001 - no id available: "some capture"
        return -1


def zero_arena_begin(device):
    """a FRESH buffer per step (one allocation + one fill): slices a still-living autograd graph of an earlier forward
    holds keep their storage alive, so a second forward before that backward cannot clobber them.  Its size follows the
    demand of the step that just ended (up AND down), capped at ZERO_ARENA_MAX."""
    a = _zarena
    if a.tracking:
        a.cap = min(ZERO_ARENA_MAX, (int(a.need * 1.25) + 4095) // 4096 * 4096)
    a.off, a.need, a.tracking = 0, 0, True
    a.active = ZERO_ARENA and a.cap > 0
    a.capture = _capture_id() if (a.active and torch.device(device).type == "cuda") else 0
    a.buf = torch.zeros(a.cap // 4, device=device, dtype=torch.float32) if a.active else None


def zero_arena_off():
    """inference paths and everything else outside a training forward / backward: zeros() is torch.zeros again and its
    demand is not counted towards the next training step's arena"""
    a = _zarena
    a.active, a.tracking, a.buf, a.off, a.need, a.capture = False, False, None, 0, 0, 0


def zeros(*shape, device):
    """fp32 zeros: a slice of the step's zero arena when one is active, else torch.zeros"""
    if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
        shape = tuple(shape[0])
    n = 1
    for d in shape:
        n *= int(d)
    a = _zarena
    nb = (n * 4 + 255) // 256 * 256
    if a.tracking:
        a.need += nb
    if a.active and n > 0 and a.off + nb <= a.buf.numel() * 4 and a.buf.device == torch.device(device) \
            and (not a.buf.is_cuda or _capture_id() == a.capture):      # never a slice zeroed outside the capture that uses it
        t = a.buf[a.off // 4: a.off // 4 + n].view(shape)
        a.off += nb
        return t
    return torch.zeros(shape, device=device, dtype=torch.float32)


def _skinny_splitk(M, N, K, max_rows=64):
    """a product with a handful of rows (one decoder step: M = batch, or batch x beam) is one row of 64-wide tiles - 16 to
    64 workgroups, each walking the whole reduction alone while the weight matrix streams through a fraction of the
    chip: split the reduction until ~256 workgroups share it (f32 atomics into the zeroed result; config 4's decoder
    steps: 20 -> 9 us for the 32 x 2048 x 4096 input gradient)"""
    if M > max_rows or N * K < 512 * 512:       # small weights: nothing to stream, keep the single-pass summation order
        return 1
    tiles = (M + 63) // 64 * ((N + 63) // 64)
    sk = 1
    while tiles * sk < 256 and K // (sk * 2) >= 128:
        sk *= 2
    return sk


def linear_bwd_x(dy, W, out=None, *, beta=0.0, epilogue=EPI_NONE, aux=None, alpha=1.0, out_dtype=torch.float32,
                 drop=None):
    """out[M,K] = alpha * drop(epi(dy[M,N] @ W[N,K])) + beta*out"""
    M, N = dy.shape
    K = W.shape[1]
    assert W.shape[0] == N and dy.is_contiguous()
    fresh = out is None
    sk = 1
    if fresh and out_dtype == torch.float32 and epilogue == EPI_NONE and aux is None and drop is None and alpha == 1.0:
        sk = _skinny_splitk(M, K, N)
    if out is None:
        assert beta == 0.0
        out = zeros(M, K, device=dy.device) if sk > 1 else torch.empty(M, K, device=dy.device, dtype=out_dtype)
    gemm(dy, W, out, M, K, N, N, K, K, transB=1, beta=beta, epilogue=epilogue, aux=aux, ldaux=K, alpha=alpha,
         drop=drop, splitk=sk)
    return out


# ---- fused position-wise feed-forward (csrc/ffn_f32.hip) ------------------------------------------
FUSED_FFN = True
FUSED_FFN_MIN_ROWS = 4096     # 32 rows per workgroup: fewer rows leave CUs idle


def ffn_fused_ok(x, w1, w2, act):
    """True if eamd_ffn_fwd / _bwd take this problem (operands all fp32 in fp32 mode or all bf16 in bf16 mode, D = 256, F a
    multiple of 128 / 256, enough rows to fill the chip); otherwise the block runs as two eamd_gemm products"""
    bf = x.dtype == torch.bfloat16
    if not FUSED_FFN or x.dtype != w1.dtype or w1.dtype != w2.dtype or (bf and _state["precision"] != 1) or \
            (not bf and (x.dtype != torch.float32 or _state["precision"] != 0)):
        return False
    return (x.shape[1] == 256 and w1.shape[1] == 256 and w1.shape[0] % (256 if bf else 128) == 0 and w1.shape[0] >= 256
            and tuple(w2.shape) == (256, w1.shape[0]) and act in (ACT_RELU, ACT_SWISH)
            and (x.shape[0] >= FUSED_FFN_MIN_ROWS or ffn_hsplit(x.shape[0], w1.shape[0], bf) > 1))


# fp32 operands, few rows (the decoder's 3232 target positions = 101 row blocks on 256 CUs): two workgroups per row block, each over
# half of the hidden units, adding their halves of the second product into a zeroed result (eamd_ffn_t.hsplit).  Measured at
# config 2's decoder: one workgroup per block 147 us whatever the grid, the GEMM pair 104 us, split in two 77 us.
FUSED_FFN_HSPLIT_MIN_ROWS = 1536


def ffn_hsplit(M, F, bf):
    if bf or M >= FUSED_FFN_MIN_ROWS or M < FUSED_FFN_HSPLIT_MIN_ROWS or F % 256 != 0 or F < 512:
        return 1
    return 2


def _ffn_desc(x, w1, b1, w2, b2, R, out, f, h, act, alpha, drop, F=None):
    p = _lib.FfnT()
    p.x, p.w1, p.b1, p.w2, p.b2, p.R = ptr(x), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(R)
    p.out, p.f, p.h = ptr(out), ptr(f), ptr(h)
    p.M, p.D, p.F, p.act = x.shape[0], x.shape[1], (F if F is not None else w1.shape[0]), act
    p.alpha = alpha
    p.dtype = 1 if x.dtype == torch.bfloat16 else 0
    p_in, s_in, p_out, s_out = drop
    p.p_in, p.salt_in, p.p_out, p.salt_out = float(p_in), int(s_in), float(p_out), int(s_out)
    if p_in > 0.0 or p_out > 0.0:
        p.drop_step = ptr(rng_state(x.device))
    return p


def _ffn_call(name, p, keep):
    fn = getattr(_lib.lib(), name)
    if _gemm_record is not None:
        _gemm_record.append((dict(kind=name, flop=4.0 * p.M * p.D * p.F), keep, lambda sp, p=p: check(fn(C.byref(p), sp), name)))
    check(fn(C.byref(p), stream_ptr()), name)


FFN_LN_FUSED = True      # the LayerNorm in front of a fused FFN runs inside its kernel


def _set_ln(p, ln, M):
    """fill the ln_* fields of an FfnT / RowProjT (the LayerNorm in front of a row-block kernel) from
    ln = (x_raw fp32 [M, 256], gamma, beta, eps, mean [M], rstd [M])"""
    xr, g, b, eps, mean, rstd = ln
    for t_ in (xr, g, b, mean, rstd):
        if t_.dtype != torch.float32 or not t_.is_contiguous():
            raise _lib.EamdError("LayerNorm operands are contiguous float32 tensors")
    D = 256         # the width these kernels normalise (csrc/rowblock.h: RB_D)
    if tuple(xr.shape) != (M, D) or g.numel() != D or b.numel() != D or mean.numel() < M or rstd.numel() < M:
        raise _lib.EamdError("LayerNorm operand shapes")
    p.ln_x, p.ln_w, p.ln_b, p.ln_mean, p.ln_rstd, p.ln_eps = ptr(xr), ptr(g), ptr(b), ptr(mean), ptr(rstd), float(eps)


def _set_lnb(p, lnb, device):
    """fill the lnb_* fields of an FfnT / RowProjT (the LayerNorm backward behind a row-block kernel) from
    lnb = (x_block_input, gamma, mean, rstd, dres or None, ws, drop_out or None, (p, salt) or None)"""
    xb, g, mean, rstd, dres, ws, d_out, d_ps = lnb
    p.lnb_x, p.lnb_gamma, p.lnb_mean, p.lnb_rstd, p.lnb_dres, p.lnb_ws = ptr(xb), ptr(g), ptr(mean), ptr(rstd), ptr(dres), ptr(ws)
    if d_out is not None:
        p.lnb_drop_out, p.lnb_drop_p, p.lnb_drop_salt, p.drop_step = ptr(d_out), float(d_ps[0]), int(d_ps[1]), ptr(rng_state(device))


def ffn_fwd(x, w1, b1, w2, b2, *, act, alpha=1.0, R=None, drop=(0.0, 0, 0.0, 0), save=True, packed=None, ln=None):
    """out = R + alpha * drop_out(drop_in(act(x W1^T + b1)) W2^T + b2) in ONE launch; with save also the two tensors
    backward needs: h = drop_in(act(z)) and f = mask / (1 - p) * act'(z).  -> (out fp32, f, h); x / w1 / w2 all fp32 or all
    bf16 (f, h in that dtype).
    ln = (x_raw fp32 [M, D], gamma, beta, eps, mean [M], rstd [M]): the block input is LayerNorm(x_raw), formed by the kernel
    while it stages its rows; `x` is then an uninitialised [M, D] buffer of the operand dtype that RECEIVES the normalised
    rows, and mean / rstd receive the row statistics (what eamd_layernorm_fwd would have left for backward)."""
    M, D = x.shape
    F = w1.shape[0]
    dt = x.dtype
    for t_ in (x, w1, w2):
        if t_.dtype != dt or dt not in (torch.float32, torch.bfloat16) or not t_.is_contiguous():
            raise _lib.EamdError("ffn_fwd: contiguous float32 or bfloat16 operands of one dtype")
    for t_ in tuple(v for v in (b1, b2, R) if v is not None):
        if t_.dtype != torch.float32 or not t_.is_contiguous():
            raise _lib.EamdError("ffn_fwd: biases / residual are contiguous float32 tensors")
    hs = ffn_hsplit(M, F, dt == torch.bfloat16)
    out = zeros(M, D, device=x.device) if hs > 1 else torch.empty(M, D, device=x.device, dtype=torch.float32)
    f = torch.empty(M, F, device=x.device, dtype=dt) if save else None
    h = torch.empty(M, F, device=x.device, dtype=dt) if save else None
    if packed is None:            # the kernels read the packed images (ffn_pack)
        packed = ffn_pack(w1, w2)[:2]
    p = _ffn_desc(x, packed[0], b1, packed[1], b2, R, out, f, h, act, alpha, drop, F=F)
    p.hsplit = hs
    if ln is not None:
        _set_ln(p, ln, M)
    _ffn_call("eamd_ffn_fwd", p, (x, packed, b1, b2, R, out, f, h, ln))
    return out, f, h


def _ffn_pack_buf(w1, device, dt):
    """the [4, F * D] buffer of one FFN's packed images, cached on w1 -> (buffer, whether it was there already)"""
    F, D = w1.shape
    buf = getattr(w1, "_eamd_ffn_pack", None)
    if buf is not None and buf.numel() == 4 * F * D and buf.device == device and buf.dtype == dt:
        return buf, True
    buf = w1._eamd_ffn_pack = torch.empty(4, F * D, device=device, dtype=dt)
    return buf, False


def ffn_pack(w1, w2):
    """the four packed weight images of one FFN (eamd_ffn_pack_f32 / _bf16) -> (fwd_first, fwd_second, bwd_first, bwd_second),
    each F * D elements in the operand dtype of the current mode.  Cached buffers on w1; the PACKING is redone at every call:
    the optimizer kernel rewrites the weights (and the bf16 shadow arena) in place - no tensor version to watch - and under
    hipGraph capture it has to be part of the replayed step."""
    F, D = w1.shape
    bf = fast() or w1.dtype == torch.bfloat16
    s1, s2 = (wshadow(w1), wshadow(w2)) if w1.dtype != torch.bfloat16 else (w1, w2)
    dt = torch.bfloat16 if bf else torch.float32
    buf, cached = _ffn_pack_buf(w1, s1.device, dt)
    if cached and _rp["active"] and getattr(w1, "_eamd_ffn_pack_epoch", -1) == _rp["epoch"]:
        return buf[0], buf[1], buf[2], buf[3]         # packed by this pass's ffn_prepack (one launch for all blocks)
    name = "eamd_ffn_pack_bf16" if bf else "eamd_ffn_pack_f32"
    check(getattr(_lib.lib(), name)(ptr(s1), ptr(s2), ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), ptr(buf[3]), D, F, stream_ptr()), name)
    return buf[0], buf[1], buf[2], buf[3]


def ffn_prepack(pairs):
    """pairs: list of (w1 [F, 256], w2 [256, F]) fp32 parameters: the packed images of ALL these feed-forward blocks in one
    launch (eamd_ffn_pack_f32_multi); ffn_pack() hands them out until rowproj_prepack_end().  fp32 mode only (no-op otherwise)."""
    if fast() or not pairs or not _rp["active"]:
        return
    arr = (_lib.FfnPackT * len(pairs))()
    n = 0
    for w1, w2 in pairs:
        F, D = w1.shape
        if D != 256 or F % 128 != 0 or F < 256 or w1.dtype != torch.float32:
            continue
        buf = _ffn_pack_buf(w1, w1.device, torch.float32)[0]
        q = arr[n]
        q.w1, q.w2, q.fwd_first, q.fwd_second, q.bwd_first, q.bwd_second = ptr(w1), ptr(w2), ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), ptr(buf[3])
        q.D, q.F = D, F
        w1._eamd_ffn_pack_epoch = _rp["epoch"]
        n += 1
    if n:
        check(_lib.lib().eamd_ffn_pack_f32_multi(arr, n, stream_ptr()), "eamd_ffn_pack_f32_multi")


def ffn_bwd_lnb_ok(M, F, dt):
    """eamd_ffn_bwd can run the LayerNorm backward as its epilogue (fp32 operands, one workgroup per row block)"""
    return dt == torch.float32 and ffn_hsplit(M, F, False) == 1


def ffn_bwd(dy, w1, w2, f, *, alpha=1.0, packed=None, lnb=None):
    """dz = alpha * (dy W2) (.) f and dx = dz W1 in ONE launch -> (dz [M, F], dx [M, D] fp32); packed = (bwd_first,
    bwd_second) of ffn_pack(w1, w2) (made here when not given).
    lnb = (x_block_input, gamma, mean, rstd, dres or None, ws, drop_out or None, (p, salt) or None): the LayerNorm backward runs
    on the dx rows inside the launch (as ops.rowproj's lnb): dx = LayerNorm'(dz W1) + dres."""
    M, D = dy.shape
    F = w1.shape[0]
    dt = dy.dtype
    assert f.shape == (M, F) and f.dtype == dt and f.is_contiguous() and dy.is_contiguous()
    dz = torch.empty(M, F, device=dy.device, dtype=dt)
    hs = ffn_hsplit(M, F, dt == torch.bfloat16)
    dx = zeros(M, D, device=dy.device) if hs > 1 else torch.empty(M, D, device=dy.device, dtype=torch.float32)
    if packed is None:
        packed = ffn_pack(w1, w2)[2:]
    assert packed[0].numel() == F * D and packed[1].numel() == F * D and packed[0].dtype == dt
    p = _ffn_desc(dy, packed[0], None, packed[1], None, None, dx, f, dz, ACT_NONE, alpha, (0.0, 0, 0.0, 0), F=F)
    p.hsplit = hs
    if lnb is not None:
        _set_lnb(p, lnb, dy.device)
    _ffn_call("eamd_ffn_bwd", p, (dy, packed, f, dz, dx, lnb))
    return dz, dx


# ---- row-block projections (csrc/rowproj_f32.hip) ---------------------------------------------------
ROWPROJ = True
ROWPROJ_MIN_ROWS = 4096       # 32 rows per workgroup: fewer rows leave CUs idle


def rowproj_ok(M, K, N):
    """shapes eamd_rowproj takes in the current mode (fp32 operands; K, N multiples of 256, K <= 768; enough rows to fill the chip)"""
    return (ROWPROJ and _state["precision"] == 0 and M >= ROWPROJ_MIN_ROWS and K % 256 == 0 and N % 256 == 0 and 256 <= K <= 768
            and N <= 1024)


_rp = {"epoch": 0, "active": False}
_rp_bufs = {}


def rowproj_prepack(groups):
    """groups: list of (holder tensor, [(W, trans), ...]): the images of MANY blocks in one or two launches (an encoder packs all
    its layers' projection weights at the start of its forward); rowproj_images() then hands them out until rowproj_prepack_end()"""
    _rp["epoch"] += 1
    _rp["active"] = True
    flat = [job for _, jobs in groups for job in jobs]
    if not flat:
        return
    imgs = rowproj_pack(flat)
    i = 0
    for holder, jobs in groups:
        holder._eamd_rp = (_rp["epoch"], [id(w) for w, _ in jobs], imgs[i:i + len(jobs)])
        i += len(jobs)
    _rp["active"] = True


def rowproj_prepack_end():
    _rp["active"] = False


def rowproj_images(holder, jobs):
    """packed images of `jobs` = [(W, trans), ...] (the projection weights of one block, cached on `holder`): those of the
    running forward's prepack if there was one, else packed here (one launch)"""
    c = getattr(holder, "_eamd_rp", None)
    if _rp["active"] and c is not None and c[0] == _rp["epoch"] and len(c[2]) == len(jobs):
        return c[2]
    return rowproj_pack(jobs)


def rowproj_pack(jobs):
    """jobs: list of (W 2-D contiguous fp32 tensor (or view with a row stride), trans) -> list of packed images (K * N floats each),
    ALL made by one launch.  trans = False: W is [N, K] (y = x W^T); trans = True: W is [K, N] (dx = dy W).  The image buffers are
    cached on the weight tensor; the packing itself is redone at every call (the optimizer rewrites the weights in place, and
    under hipGraph capture it has to be part of the replayed step)."""
    arr = (_lib.RowProjPackT * len(jobs))()
    imgs = []
    for q, (W, trans) in zip(arr, jobs):
        assert W.dim() == 2 and W.dtype == torch.float32 and W.stride(1) == 1
        K, N = (W.shape[0], W.shape[1]) if trans else (W.shape[1], W.shape[0])
        # image buffers are cached per (weight storage address, shape, orientation): the weights live in persistent arenas
        key = (W.data_ptr(), K, N, bool(trans), W.device.index)
        img = _rp_bufs.get(key)
        if img is None:
            if len(_rp_bufs) > 4096:
                _rp_bufs.clear()
            img = _rp_bufs[key] = torch.empty(K * N, device=W.device, dtype=torch.float32)
        q.w, q.image, q.K, q.N, q.ldw, q.trans = ptr(W), ptr(img), K, N, W.stride(0), bool(trans)
        imgs.append(img)
    check(_lib.lib().eamd_rowproj_pack_f32(arr, len(jobs), stream_ptr()), "eamd_rowproj_pack_f32")
    return imgs


def rowproj(a, img, N, *, bias=None, R=None, alpha=1.0, drop=None, ln=None, affine=None, lnb=None, out=None):
    """out[M, N] = R + alpha * dropout(A' B + bias), 32 rows per workgroup through the whole product (eamd_rowproj).
    a [M, K] fp32 (row stride allowed); img = rowproj_pack image of B [K, N].
    ln = (x_raw [M, 256], gamma, beta, eps, mean [M], rstd [M]): A' = LayerNorm(x_raw), `a` RECEIVES the normalised rows.
    affine = (scale [256], shift [256], act, a_out or None): A' = act(a * scale + shift), also written to a_out.
    lnb = (x_block_input [M, 256], gamma, mean, rstd, dres or None, ws, drop_out or None, (p, salt) or None): N = 256, the
    LayerNorm backward runs on the result rows: out = dx (+ dres), ws = per-workgroup partials of d gamma / d beta."""
    M, K = a.shape
    dev = a.device
    if out is None:
        out = torch.empty(M, N, device=dev, dtype=torch.float32)
    p = _lib.RowProjT()
    p.a, p.lda, p.w, p.bias = ptr(a), a.stride(0), ptr(img), ptr(bias)
    p.R, p.ldr = ptr(R), (R.stride(0) if R is not None else 0)
    p.out, p.ldo = ptr(out), out.stride(0)
    p.M, p.K, p.N, p.alpha = M, K, N, float(alpha)
    if drop is not None and drop[0] > 0.0:
        p.p_out, p.salt_out, p.drop_step = float(drop[0]), int(drop[1]), ptr(rng_state(dev))
    if ln is not None:
        _set_ln(p, ln, M)
    if affine is not None:
        sc, sh, act, a_out = affine
        p.a_scale, p.a_shift, p.a_act, p.a_out = ptr(sc), ptr(sh), int(act), ptr(a_out)
    if lnb is not None:
        _set_lnb(p, lnb, dev)
    fn = _lib.lib().eamd_rowproj
    keep = (a, img, bias, R, out, ln, affine, lnb)
    if _gemm_record is not None:
        _gemm_record.append((dict(kind="rowproj", flop=2.0 * M * K * N), keep, lambda sp, p=p: check(fn(C.byref(p), sp), "eamd_rowproj")))
    check(fn(C.byref(p), stream_ptr()), "eamd_rowproj")
    return out


def rowproj_lnb_ws(M, device):
    return torch.empty(_lib.lib().eamd_rowproj_lnb_workspace(M), device=device, dtype=torch.float32)


# ---- weight-gradient side stream ---------------------------------------------------------------
# dW = dY^T X is needed only by the optimizer (and the gradient all-reduce), never by the rest of
# backward.  When enabled, every weight-gradient GEMM is issued on a second HIP stream so that it
# overlaps the dX chain; under hipGraph capture this becomes a parallel branch of the graph.
_wgrad = {"stream": None, "used": False}


def enable_wgrad_stream(enable=True):
    _wgrad["stream"] = torch.cuda.Stream() if enable else None
    _wgrad["used"] = False


def wgrad_group_end():
    wgrad_group_flush()
    _wgroup["on"] = False


def wgrad_join():
    """launch the queued weight-gradient GEMMs and make the current stream wait for all weight-gradient work issued so far"""
    wgrad_group_flush()
    st = _wgrad["stream"]
    if st is not None and _wgrad["used"]:
        torch.cuda.current_stream().wait_stream(st)
        _wgrad["used"] = False


def linear_bwd_w(dy, x, dW, *, alpha=1.0, b_act=ACT_NONE, db=None, group=True):
    """group=False: never queued for the grouped launch (per-chunk gradients of a streamed loss: queueing would keep
    every chunk's operands alive until the flush)"""
    st = _wgrad["stream"]
    if st is None:
        return _linear_bwd_w(dy, x, dW, alpha=alpha, b_act=b_act, db=db, group=group)
    cur = torch.cuda.current_stream()
    st.wait_stream(cur)                 # operands were produced on the main stream
    with torch.cuda.stream(st):
        _linear_bwd_w(dy, x, dW, alpha=alpha, b_act=b_act, db=db)
    dy.record_stream(st)                # keep the caching allocator from recycling them early
    x.record_stream(st)
    _wgrad["used"] = True


def _linear_bwd_w(dy, x, dW, *, alpha=1.0, b_act=ACT_NONE, db=None, group=True):
    """dW[N,K] += alpha * dy[M,N]^T @ b_act(x)[M,K]   (split-K, f32 atomics)
    db[N] += alpha * column sums of dy (bias gradient, fused into the same launch)"""
    M, N = dy.shape
    K = x.shape[1]
    assert x.shape[0] == M and dW.numel() == N * K and dW.dtype == torch.float32
    grouping = group and _wgroup["on"] and _wgrad["stream"] is None
    if (grouping and M <= STACK_WGRAD_MAX_ROWS and alpha == 1.0 and b_act == ACT_NONE
            and dy.is_contiguous() and x.is_contiguous() and _in_grad_arena(dW)):
        # one decoder step's weight gradient (M = batch rows) reads and writes the whole dW for a reduction of M: the
        # steps of a backward pass are stacked along the reduction instead and leave as ONE product at the flush
        # (config 4: 101 x (22 + 12 us) of 32 MB / 16 MB read-modify-writes -> two GEMMs with K = 3232)
        key = (dW.data_ptr(), db.data_ptr() if db is not None else 0, dy.dtype, x.dtype, N, K)
        _wgroup["stack"].setdefault(key, (dW, db, [], []))
        ent = _wgroup["stack"][key]
        ent[2].append(dy)
        ent[3].append(x)
        return
    sk = auto_splitk(N, K, M)
    tile = 0
    t64 = ((N + 63) // 64) * ((K + 63) // 64)
    if grouping and t64 <= GROUP_WGRAD_MAX_TILES and _in_grad_arena(dW):
        if t64 >= GROUP_WGRAD_TILE128_MIN and N >= 128 and K >= 128 and dy.dtype == torch.float32 and _state["precision"] == 0:
            # big outputs (the FFN weights) go to the 128x128 grouped launch: a quarter of the operand re-reads
            tile = 128
            sk = max(1, min(GROUP_WGRAD_T128_WGS // (((N + 127) // 128) * ((K + 127) // 128)), M // 256))
        else:
            tile = 64
            sk = max(1, sk // GROUP_WGRAD_SK_DIV)
    gemm(dy, x, dW, N, K, M, N, K, K, transA=1, transB=1, alpha=alpha, b_act=b_act, splitk=sk, tile=tile,
         beta=1.0 if sk == 1 else 0.0, colsum=db, group=grouping)


def colsum(x, out, scale=1.0, rows=None, D=None, ld=None):
    rows = x.shape[0] if rows is None else rows
    D = x.shape[1] if D is None else D
    ld = D if ld is None else ld
    assert out.numel() >= D
    check(_lib.lib().eamd_colsum(ptr(x), ld, ptr(out), rows, D, scale,
                                 1 if x.dtype == torch.bfloat16 else 0, stream_ptr()), "eamd_colsum")


# ---- row kernels -------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, out_dtype=torch.float32):
    rows, D = x.shape
    y = torch.empty(rows, D, device=x.device, dtype=out_dtype)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    y32, y16 = (ptr(y), None) if out_dtype == torch.float32 else (None, ptr(y))
    check(_lib.lib().eamd_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), y32, y16, ptr(mean), ptr(rstd), rows, D,
                                        eps, stream_ptr()), "eamd_layernorm_fwd")
    return y, mean, rstd


class _LnReduceJob(C.Structure):
    _fields_ = [("ws", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("nblk", C.c_int32), ("D", C.c_int32)]


# Deferred gamma / beta reduction: inside a backward pass every LayerNorm backward leaves its per-block partial sums
# in its workspace and ONE launch at the end of the pass (autograd's final callback, the hook DistributedDataParallel
# uses) adds them all into the gradients - 80 launches per config-2 training step become one.  Only for gradients
# that live in the flat arena of train.FlatParams (persistent memory); switched off while a
# GradReducer overlaps bucket all-reduces with backward (the gradients must be final when a block reports them).
defer_ln_reduce = True
_ln_pending = []
_ln_task = -1        # autograd graph-task id the pending partials belong to


def flush_ln_reduce():
    """add the pending LayerNorm gamma / beta partials into their gradients (one launch per 64 LayerNorms)"""
    global _ln_pending, _ln_task
    jobs, _ln_pending, _ln_task = _ln_pending, [], -1
    if not jobs:
        return
    tab = (_LnReduceJob * len(jobs))()
    for i, (ws, dg, db, nblk, D) in enumerate(jobs):
        tab[i].ws, tab[i].dgamma, tab[i].dbeta, tab[i].nblk, tab[i].D = ws.data_ptr(), dg.data_ptr(), db.data_ptr(), nblk, D
    with torch.cuda.device(jobs[0][0].device):
        check(_lib.lib().eamd_layernorm_bwd_reduce(tab, len(jobs), stream_ptr()), "eamd_layernorm_bwd_reduce")


def ln_partials_reduce(ws, dgamma, dbeta, nblk, D):
    """per-block partial sums ws [nblk][2][D] of a LayerNorm backward (left by eamd_rowproj's epilogue) -> dgamma / dbeta: queued
    behind the running backward pass like every other LayerNorm's second stage, or reduced right away outside one"""
    if _defer_ln(ws, dgamma, dbeta, nblk, D):
        return
    tab = (_LnReduceJob * 1)()
    tab[0].ws, tab[0].dgamma, tab[0].dbeta, tab[0].nblk, tab[0].D = ws.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), nblk, D
    check(_lib.lib().eamd_layernorm_bwd_reduce(tab, 1, stream_ptr()), "eamd_layernorm_bwd_reduce")


def _defer_ln(ws, dgamma, dbeta, nblk, D):
    """True if the reduction of this pass was queued behind the running backward pass"""
    global _ln_pending, _ln_task
    if not defer_ln_reduce or not (getattr(dgamma, "_eamd_arena", False) and getattr(dbeta, "_eamd_arena", False)):
        return False      # gradients handed back to autograd by value must be complete when backward returns them
    task = torch._C._current_graph_task_id()
    if task < 0:                  # not inside a backward pass (direct call): reduce right away
        return False
    if task != _ln_task:          # first LayerNorm of this pass (partials of a pass that died are dropped)
        _ln_pending = []
        torch.autograd.Variable._execution_engine.queue_callback(flush_ln_reduce)
        _ln_task = task
    _ln_pending.append((ws, dgamma, dbeta, nblk, D))
    return True


def layernorm_bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, drop=None):
    """drop = (p, salt): also return bf16(dropout(dx; p, salt)) written by the same kernel (D = 256 / 512 only) ->
    (dx, dx_dropped); otherwise -> dx"""
    rows, D = x.shape
    assert dy.shape == x.shape and dgamma.numel() == D and dbeta.numel() == D
    dx = torch.empty_like(x)
    L = _lib.lib()
    nws = L.eamd_layernorm_bwd_workspace(rows, D)
    ws = torch.empty(nws, device=x.device, dtype=torch.float32)
    pg, pb = ptr(dgamma), ptr(dbeta)
    if _defer_ln(ws, dgamma, dbeta, nws // (2 * D), D):
        pg = pb = None
    if drop is not None:
        dx16 = torch.empty(rows, D, device=x.device, dtype=act_dtype())        # dropped copy in the GEMM-operand dtype
        fn, name = ((L.eamd_layernorm_bwd_drop, "eamd_layernorm_bwd_drop") if fast()
                    else (L.eamd_layernorm_bwd_drop_f32, "eamd_layernorm_bwd_drop_f32"))
        check(fn(ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dx16),
                 drop[0], ptr(rng_state(x.device)), drop[1], pg,
                 pb, ptr(ws), rows, D, stream_ptr()), name)
        return dx, dx16
    check(L.eamd_layernorm_bwd(ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dx),
                               pg, pb, ptr(ws), rows, D, stream_ptr()), "eamd_layernorm_bwd")
    return dx


F32_FUSED_ATTN = True   # fp32 mode: eamd_attn_fwd_f32 / eamd_attn_bwd_q_f32 (tests flip it to reach the GEMM / softmax path)


def attn_fwd_supported(T1, T2, dk, rel):
    """shapes the fused attention forward (eamd_attn_fwd) covers; alignment is checked by the library"""
    if dk != 64 or (rel and T1 != T2):
        return False
    # rows of 513 .. 4096 keys: the key-split long-row kernels (attn_f32.hip; 16 queries per workgroup up to 2048 keys, 8 beyond)
    return (fast() or F32_FUSED_ATTN) and T2 <= 4096


def _attn_tail(drop, device, rel, T1, T2, shift_len, Pd=()):
    """the argument tail attn_fwd and attn_bwd_q share: (Pd,) drop_p, drop_step, drop_salt, shift_len.  drop = (p, salt) or None;
    relative positions on a padded batch take the rel_shift over the batch's own length (shift_len: int32 device scalar)"""
    dropping = drop is not None and drop[0] > 0.0
    dargs = (drop[0], ptr(rng_state(device)), drop[1]) if dropping else (0.0, None, 0)
    return tuple(ptr(t) if dropping else None for t in Pd) + dargs + (ptr(shift_len) if (rel and T1 == T2) else None,)


def attn_fwd(qu, qv, k, v, pos, mask, B, T1, T2, H, dk, ldp, scale, drop=None, shift_len=None):
    """qu / qv / k / v: (tensor, element offset, row stride) views of [rows, *] matrices, heads side by side, all bf16
    (eamd_attn_fwd) or all fp32 (eamd_attn_fwd_f32); pos: such a view of the [T2, H*dk] projected positions, or None.
    Returns (P [H*B*T1*ldp], Pd, ctx [B*T1, H*dk]) in that dtype, or None if the library declines the operands
    (EAMD_EUNSUPPORTED).  drop = (p, salt): attention dropout - ctx is built from Pd = dropout(P) (same mask as
    ops.dropout(P, p, salt)), which is returned beside the undropped P; without dropout Pd is P."""
    dev = qu[0].device
    dt = qu[0].dtype
    D = H * dk
    mb = mi = 0
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.dim() == 3 and mask.shape[0] in (1, B)
        assert mask.shape[2] == T2 and mask.shape[1] in (1, T1)
        mb = 0 if mask.shape[0] == 1 else mask.shape[1] * mask.shape[2]
        mi = 0 if mask.shape[1] == 1 else T2
    assert dt in (torch.bfloat16, torch.float32)
    for t_, _, _ in (qu, k, v) + ((qv,) if qv is not None else ()):
        assert t_.dtype == dt and t_.is_cuda
    assert pos is None or (pos[0].dtype == dt and pos[2] >= D)
    P = torch.empty(H * B * T1 * ldp, device=dev, dtype=dt)
    cx = torch.empty(B * T1, D, device=dev, dtype=dt)
    dropping = drop is not None and drop[0] > 0.0
    Pd = torch.empty_like(P) if dropping else P
    args = (ptr(qu[0], qu[1]), qu[2], ptr(qv[0], qv[1]) if qv is not None else None, qv[2] if qv is not None else 0,
            ptr(k[0], k[1]), k[2], ptr(v[0], v[1]), v[2], ptr(pos[0], pos[1]) if pos is not None else None,
            pos[2] if pos is not None else 0,
            ptr(mask), mb, mi, ptr(P), ldp, ptr(cx), D, B, H, T1, T2, dk, scale)
    args = args + _attn_tail(drop, dev, pos is not None, T1, T2, shift_len, Pd=(Pd,))
    name = "eamd_attn_fwd" if dt == torch.bfloat16 else "eamd_attn_fwd_f32"
    fn = getattr(_lib.lib(), name)
    rc = fn(*args, stream_ptr())
    if rc == _lib.EAMD_EUNSUPPORTED:
        return None
    check(rc, name)
    if _gemm_record is not None:
        _gemm_record.append((dict(kind=name, flop=0.0), (qu, qv, k, v, pos, mask, P, Pd, cx), lambda sp, args=args: check(fn(*args, sp), name)))
    return P, Pd, cx


def attn_bwd_q(dctx, k, v, P, dS, dbd, dq, B, T1, T2, H, dk, ldp, scale, drop=None, shift_len=None):
    """dctx / k / v / dq: (tensor, element offset, row stride) views; P, dS (and dbd or None): [H*B*T1*ldp], bf16
    (eamd_attn_bwd_q; dq fp32 or bf16) or everything fp32 (eamd_attn_bwd_q_f32).
    dS, dbd and dq are written.  Returns False if the library declines the operands (EAMD_EUNSUPPORTED)."""
    if P.dtype == torch.bfloat16:
        name = "eamd_attn_bwd_q"
        args = (ptr(dctx[0], dctx[1]), dctx[2], ptr(k[0], k[1]), k[2], ptr(v[0], v[1]), v[2], ptr(P), ldp,
                ptr(dS), ptr(dbd), ptr(dq[0], dq[1]), dq[2], dq[0].dtype == torch.bfloat16, B, H, T1, T2, dk,
                scale)
    else:
        name = "eamd_attn_bwd_q_f32"
        for t_ in (dctx[0], k[0], v[0], P, dS, dq[0]) + ((dbd,) if dbd is not None else ()):
            assert t_.dtype == torch.float32
        args = (ptr(dctx[0], dctx[1]), dctx[2], ptr(k[0], k[1]), k[2], ptr(v[0], v[1]), v[2], ptr(P), ldp,
                ptr(dS), ptr(dbd), ptr(dq[0], dq[1]), dq[2], B, H, T1, T2, dk, scale)
    # the forward's attention dropout: dP <- mask * dP / (1 - p)
    args = args + _attn_tail(drop, P.device, dbd is not None, T1, T2, shift_len)
    fn = getattr(_lib.lib(), name)
    rc = fn(*args, stream_ptr())
    if rc == _lib.EAMD_EUNSUPPORTED:
        return False
    check(rc, name)
    if _gemm_record is not None:
        _gemm_record.append((dict(kind=name, flop=0.0), (dctx, k, v, P, dS, dbd, dq), lambda sp, args=args: check(fn(*args, sp), name)))
    return True


FUSED_ATTN_KV = True   # fp32 mode: eamd_attn_bwd_kv_f32 (tests flip it to reach the batched GEMMs)


def attn_bwd_kv(Pd, dS, dbd, dctx, qu, qv, dv, dk_, dpos, B, T1, T2, H, dk, ldp):
    """dv = Pd^T dctx, dk = dS^T qu (and, fp32 only, dpos += dbd^T qv) in one launch.  All tensors fp32
    (eamd_attn_bwd_kv_f32) or all bf16 (eamd_attn_bwd_kv).  dctx / qu / qv / dv / dk_ / dpos: (tensor, element offset,
    row stride) views; dv and dk_ share their row stride.  Returns False if the library declines the operands
    (EAMD_EUNSUPPORTED)."""
    dt = Pd.dtype
    assert dt in (torch.float32, torch.bfloat16)
    for t_ in (Pd, dS, dctx[0], qu[0], dv[0], dk_[0]):
        assert t_.dtype == dt and t_.is_cuda
    assert dv[2] == dk_[2]
    rel = dbd is not None
    if dt == torch.float32:
        args = (ptr(Pd), ptr(dS), ptr(dbd) if rel else None, ldp, ptr(dctx[0], dctx[1]), dctx[2], ptr(qu[0], qu[1]),
                qu[2], ptr(qv[0], qv[1]) if rel else None, qv[2] if rel else 0, ptr(dv[0], dv[1]), ptr(dk_[0], dk_[1]),
                dv[2], ptr(dpos[0], dpos[1]) if rel else None, dpos[2] if rel else 0, B, H, T1, T2, dk)
        name = "eamd_attn_bwd_kv_f32"
    else:
        assert not rel, "the bf16 key-side launch leaves the positional product to the GEMM"
        args = (ptr(Pd), ptr(dS), ldp, ptr(dctx[0], dctx[1]), dctx[2], ptr(qu[0], qu[1]), qu[2],
                ptr(dv[0], dv[1]), ptr(dk_[0], dk_[1]), dv[2], B, H, T1, T2, dk)
        name = "eamd_attn_bwd_kv"
    fn = getattr(_lib.lib(), name)
    rc = fn(*args, stream_ptr())
    if rc == _lib.EAMD_EUNSUPPORTED:
        return False
    check(rc, name)
    if _gemm_record is not None:
        _gemm_record.append((dict(kind=name, flop=0.0), (Pd, dS, dbd, dctx, qu, qv, dv, dk_, dpos),
                             lambda sp, args=args: check(fn(*args, sp), name)))
    return True


def softmax_fwd(ac, bd, mask, P, nblocks, B, T1, T2, ld, scale):
    """P may be fp32 (may alias ac) or bf16 (separate buffer)"""
    mb = mi = 0
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.dim() == 3 and mask.shape[0] in (1, B)
        assert mask.shape[2] == T2 and mask.shape[1] in (1, T1)
        mb = 0 if mask.shape[0] == 1 else mask.shape[1] * mask.shape[2]   # batch-broadcast masks
        mi = 0 if mask.shape[1] == 1 else T2
    assert ac.numel() >= nblocks * T1 * ld and P.numel() >= nblocks * T1 * ld
    p32, p16 = (ptr(P), None) if P.dtype == torch.float32 else (None, ptr(P))
    check(_lib.lib().eamd_softmax_fwd(ptr(ac), ptr(bd), ptr(mask), mb, mi, p32, p16, nblocks,
                                      B, T1, T2, ld, scale, stream_ptr()),
          "eamd_softmax_fwd")


def softmax_bwd(P, dP, dbd, nblocks, T1, T2, ld, scale, dS16=None):
    """fp32: dP is overwritten with dS, dbd (fp32) receives the inverse rel-shift scatter.
    bf16: P bf16, dP fp32 in, dS16 (bf16) out, dbd bf16.  dbd is fully written by the kernel (no pre-zeroing)."""
    assert P.numel() >= nblocks * T1 * ld and dP.numel() >= nblocks * T1 * ld and dP.dtype == torch.float32
    if P.dtype == torch.bfloat16:
        assert dS16 is not None and dS16.dtype == torch.bfloat16 and (dbd is None or dbd.dtype == torch.bfloat16)
        check(_lib.lib().eamd_softmax_bwd(None, ptr(P), ptr(dP), None, ptr(dS16), ptr(dbd), nblocks, T1, T2,
                                          ld, scale, stream_ptr()), "eamd_softmax_bwd")
    else:
        check(_lib.lib().eamd_softmax_bwd(ptr(P), None, ptr(dP), ptr(dbd), None, None, nblocks, T1, T2,
                                          ld, scale, stream_ptr()), "eamd_softmax_bwd")


def lsm_loss(logits, target, smoothing, inv_denom, ignore_id, want_grad=True):
    rows, V = logits.shape
    assert target.numel() == rows and target.dtype == torch.int64
    loss_rows = torch.empty(rows, device=logits.device, dtype=torch.float32)
    correct = torch.empty(rows, device=logits.device, dtype=torch.float32)
    grad = torch.empty_like(logits) if want_grad else None
    check(_lib.lib().eamd_lsm_loss(ptr(logits), ptr(target), ptr(loss_rows), ptr(correct), ptr(grad), rows, V,
                                   ignore_id, smoothing, inv_denom, stream_ptr()),
          "eamd_lsm_loss")
    return loss_rows, correct, grad


def argmax_rows(x):
    rows, V = x.shape
    out = torch.empty(rows, device=x.device, dtype=torch.int32)
    check(_lib.lib().eamd_argmax_rows(ptr(x), V, ptr(out), rows, V, stream_ptr()), "eamd_argmax_rows")
    return out


def reduce_sum(x, scale=1.0):
    out = torch.empty((), device=x.device, dtype=torch.float32)
    check(_lib.lib().eamd_reduce_sum(ptr(x), x.numel(), ptr(out), scale, stream_ptr()),
          "eamd_reduce_sum")
    return out


def linear_rows_ln(x, gamma, beta, eps, W, b, *, act=EPI_NONE, R=None, alpha=1.0, out=None):
    """y = alpha * act(LayerNorm(x) W^T + b) + R in ONE launch (eamd_linear_rows_ln_f32: at most 16 rows, or up to 1024 rows at
    K <= 256 in 16-row blocks on the matrix cores), or None when the library declines (more rows, wider K, unaligned): the caller
    then normalises and multiplies in two launches"""
    M, K = x.shape
    N = W.shape[0]
    # (16-row blocks: every 16 x 16 tile's wave repeats the LayerNorm of its rows - measured at M = 320: 10.6 us against
    # LayerNorm + product = 4.7 + 7.8 us at N = 256 / 768, but 18.8 against 18.4 at N = 2048 and 40 against 22.5 at N = 5000)
    if (M > 16 and (K > 256 or M > LINEAR_ROWS_BLOCK_MAX or N > 1024)) or K > 1024 or x.dtype != torch.float32 or W.dtype != torch.float32 or x.stride(1) != 1 or act not in (EPI_NONE, EPI_RELU, EPI_SWISH):
        return None
    y = out if out is not None else torch.empty(M, N, device=x.device, dtype=torch.float32)
    rc = _lib.lib().eamd_linear_rows_ln_f32(ptr(x), ptr(gamma), ptr(beta), eps, ptr(W), ptr(b), ptr(R), ptr(y), M, N, K,
                                            int(act), alpha, x.stride(0) if M > 1 else K,
                                            R.stride(0) if (R is not None and M > 1) else 0, y.stride(0), stream_ptr())
    if rc == _lib.EAMD_EUNSUPPORTED:
        return None
    check(rc, "eamd_linear_rows_ln_f32")
    return y


def decode_self_attn(qkv, Kc, Vc, slot_at, pos, H, pos_dev=None):
    """the newest position of n hypotheses attends over its prefix; keys / values of this step (columns D.., 2D.. of qkv) are
    appended to the time-major caches Kc / Vc [Lcap, n, D] at row `pos`; slot_at [n, Lcap] int32 (eamd_decode_self_attn_dyn) -> ctx [n, D]"""
    n = qkv.shape[0]
    Lcap, n2, D = Kc.shape
    assert n2 == n and Vc.shape == Kc.shape and slot_at.shape == (n, Lcap) and slot_at.dtype == torch.int32 and qkv.stride(1) == 1
    ctx = torch.empty(n, D, device=qkv.device, dtype=torch.float32)
    check(_lib.lib().eamd_decode_self_attn_dyn(ptr(qkv), qkv.stride(0), ptr(Kc), ptr(Vc), ptr(slot_at), Lcap, int(pos),
                                               ptr(pos_dev), n, H, D, ptr(ctx), stream_ptr()), "eamd_decode_self_attn_dyn")
    return ctx


SRC_ATTN_SPLITS = 4      # key splits of the grouped source attention (1: none)


def decode_src_attn(q, kv, k_off, v_off, ldkv, mask, G, g, T, H, group=False):
    """one query position per hypothesis over the memory of its utterance (eamd_decode_src_attn): q [G * g, D]; kv = the tensor
    that holds keys / values of this layer at element offsets k_off / v_off, row stride ldkv ([G * T] rows); mask [G, 1, T] uint8
    or None -> ctx [G * g, D], or None when the library declines.  group: one workgroup per (utterance, head) for all g
    hypotheses (eamd_decode_src_attn_group; g <= 16, T <= 1024) instead of one per (hypothesis, head)"""
    n, D = q.shape
    ctx = torch.empty(n, D, device=q.device, dtype=torch.float32)
    splits = SRC_ATTN_SPLITS if (group and T >= 128 and G * H * SRC_ATTN_SPLITS <= 4096) else 1
    if group and splits > 1:       # the keys of an utterance over several workgroups + a merge launch (eamd_decode_src_attn_split)
        L = _lib.lib()
        ws = torch.empty(L.eamd_decode_src_attn_split_workspace(G, g, H, splits), device=q.device, dtype=torch.float32)
        rc = L.eamd_decode_src_attn_split(ptr(q), q.stride(0), ptr(kv, k_off), ptr(kv, v_off), ldkv, ptr(mask),
                                          G, g, T, H, D, splits, ptr(ws), ptr(ctx), stream_ptr())
        if rc != _lib.EAMD_EUNSUPPORTED:
            check(rc, "eamd_decode_src_attn_split")
            return ctx
    fn = _lib.lib().eamd_decode_src_attn_group if group else _lib.lib().eamd_decode_src_attn
    rc = fn(ptr(q), q.stride(0), ptr(kv, k_off), ptr(kv, v_off), ldkv, ptr(mask), G, g, T, H, D, ptr(ctx), stream_ptr())
    if rc == _lib.EAMD_EUNSUPPORTED:
        return None
    check(rc, "eamd_decode_src_attn")
    return ctx


def beam_slots(slot_in, hyp, pos, pos_dev=None):
    """the slot table behind a beam step's selection: row i = row hyp[i] of slot_in with column `pos` set to hyp[i]
    (pos_dev: int32 device scalar added to pos)"""
    n, Lcap = slot_in.shape
    out = torch.empty_like(slot_in)
    check(_lib.lib().eamd_beam_slots_dyn(ptr(slot_in), ptr(out), ptr(hyp), n, Lcap, int(pos), ptr(pos_dev), stream_ptr()), "eamd_beam_slots_dyn")
    return out


def copy_jobs(pairs):
    """up to 16 small device-to-device copies (dst <- src, contiguous tensors of equal byte size) in one launch (eamd_copy_jobs)"""
    assert 0 < len(pairs) <= 16
    for d, s_ in pairs:
        assert d.is_contiguous() and s_.is_contiguous() and d.numel() * d.element_size() == s_.numel() * s_.element_size(), (d.shape, s_.shape)
    n = len(pairs)
    src = (C.c_void_p * n)(*[s_.data_ptr() for _, s_ in pairs])
    dst = (C.c_void_p * n)(*[d.data_ptr() for d, _ in pairs])
    nb = (C.c_int64 * n)(*[d.numel() * d.element_size() for d, _ in pairs])
    check(_lib.lib().eamd_copy_jobs(src, dst, nb, n, stream_ptr()), "eamd_copy_jobs")


def weighted_sum(logps, weights):
    """sum_k w_k logp_k over up to four contiguous fp32 [n, V] matrices, in torch's order ((0 + w_0 l_0) + w_1 l_1 ...): one launch"""
    out = torch.empty_like(logps[0])
    arr = (C.c_void_p * 4)(*[lp.data_ptr() for lp in logps] + [None] * (4 - len(logps)))
    wts = (C.c_float * 4)(*[float(w) for w in weights] + [0.0] * (4 - len(weights)))
    check(_lib.lib().eamd_weighted_sum(arr, wts, len(logps), out.numel(), ptr(out), stream_ptr()), "eamd_weighted_sum")
    return out


def weighted_topk_rows(logps, weights, k, extra=-1):
    """weighted_sum + topk_rows(idx32=True) in one launch (eamd_weighted_topk_rows) -> (pre [n, V], idx int64 [n, k], idx32).
    extra >= 0: a column k with that token (-1 where it is already among the k) is appended to idx / idx32"""
    n, V = logps[0].shape
    ko = k + (1 if extra >= 0 else 0)
    for lp in logps:
        if lp.dtype != torch.float32 or not lp.is_contiguous() or lp.shape != (n, V):
            raise _lib.EamdError("weighted_topk_rows: contiguous float32 [n, V] matrices")
    pre = torch.empty_like(logps[0])
    vals = torch.empty(n, ko, device=pre.device, dtype=torch.float32)
    idx = torch.empty(n, ko, device=pre.device, dtype=torch.int64)
    i32 = torch.empty(n, ko, device=pre.device, dtype=torch.int32)
    arr = (C.c_void_p * 4)(*[lp.data_ptr() for lp in logps] + [None] * (4 - len(logps)))
    wts = (C.c_float * 4)(*[float(w) for w in weights] + [0.0] * (4 - len(weights)))
    check(_lib.lib().eamd_weighted_topk_rows(arr, wts, len(logps), n, V, k, int(extra), ptr(pre), ptr(vals), ptr(idx), ptr(i32), stream_ptr()),
          "eamd_weighted_topk_rows")
    return pre, idx, i32


def beam_select(pre, ids, psi, c_s, hyp, w_ctc, nutt, beam):
    """the `beam` best continuations of each utterance among its beam x P pre-beam candidates (eamd_beam_select) ->
    (top_s [nutt, beam], top_i [nutt, beam] = local slot * V + token, c_local [n, P] = psi - c_s)"""
    n, V = pre.shape
    P = ids.shape[1]
    assert n == nutt * beam and ids.dtype == torch.int64 and ids.is_contiguous() and psi.shape == (n, P) and pre.is_contiguous()
    top_s = torch.empty(nutt, beam, device=pre.device, dtype=torch.float32)
    top_i = torch.empty(nutt, beam, device=pre.device, dtype=torch.int64)
    c_local = torch.empty(n, P, device=pre.device, dtype=torch.float32)
    check(_lib.lib().eamd_beam_select(ptr(pre), ptr(ids), ptr(psi), ptr(c_s), ptr(hyp), w_ctc, nutt, beam, P, V, ptr(c_local),
                                      ptr(top_s), ptr(top_i), stream_ptr()), "eamd_beam_select")
    return top_s, top_i, c_local


def topk_rows(x, k, idx32=False):
    """(values [rows, k], indices [rows, k] int64) of the k largest of each row of a contiguous fp32 [rows, n] tensor, sorted
    (value descending, ties by ascending index): one launch, graph-replay safe (torch.topk's multi-block path is neither).
    idx32: a third result, the indices as int32 (the same launch)"""
    rows, n = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous() or k > 64:
        raise _lib.EamdError("topk_rows: contiguous float32 [rows, n], k <= 64")
    vals = torch.empty(rows, k, device=x.device, dtype=torch.float32)
    idx = torch.empty(rows, k, device=x.device, dtype=torch.int64)
    i32 = torch.empty(rows, k, device=x.device, dtype=torch.int32) if idx32 else None
    check(_lib.lib().eamd_topk_rows_i32(ptr(x), n, rows, n, k, ptr(vals), ptr(idx), ptr(i32), stream_ptr()), "eamd_topk_rows_i32")
    return (vals, idx, i32) if idx32 else (vals, idx)


def beam_step(pre, ids, psi, c_s, hyp, w_ctc, nutt, beam, L, step, eos, maxlen, sc_in, logps, yseq_in, dyn=None, slot_in=None):
    """selection and bookkeeping of a BeamSearch step with a pre-beam in one launch (eamd_beam_step_dyn = eamd_beam_select +
    eamd_beam_finish) -> (sc_out [ns, n], yseq_out, hyp_out, hyp_i, tok_i, tok32, cs_out, rec)"""
    n, V = pre.shape
    P = ids.shape[1]
    ns, W = sc_in.shape[0], yseq_in.shape[1]
    nf = len(logps)
    dev = pre.device
    for t_ in (pre, psi, c_s, hyp, sc_in) + tuple(logps):
        if t_.dtype != torch.float32 or not t_.is_contiguous():
            raise _lib.EamdError("beam_step: contiguous float32 score tensors")
    for t_ in (ids, maxlen, yseq_in):
        if t_.dtype != torch.int64 or not t_.is_contiguous():
            raise _lib.EamdError("beam_step: contiguous int64 index tensors")
    assert n == nutt * beam and psi.shape == (n, P) and c_s.numel() == n and hyp.numel() == n and sc_in.shape[1] == n
    assert yseq_in.shape[0] == n and all(lp.shape == (n, V) for lp in logps) and ns == nf + 1 and maxlen.numel() == nutt
    c_local = torch.empty(n, P, device=dev, dtype=torch.float32)
    sc_out = torch.empty(ns, n, device=dev, dtype=torch.float32)
    yseq_out = torch.empty(n, W, device=dev, dtype=torch.int64)
    hyp_out, cs_out = (torch.empty(n, device=dev, dtype=torch.float32) for _ in range(2))
    hyp_i, tok_i = (torch.empty(n, device=dev, dtype=torch.int64) for _ in range(2))
    tok32 = torch.empty(n, device=dev, dtype=torch.int32)
    # dyn = (step_dev, step_out, ring): the step index read from the device, step + 1 written to step_out, the log row into slot
    # step % R of the ring [R, n, 3 + ns + W] (one graph for every step)
    step_dev = step_out = None
    ring = 0
    if dyn is not None:
        step_dev, step_out, rec = dyn
        ring = rec.shape[0]
        assert rec.shape[1:] == (n, 3 + ns + W) and rec.is_contiguous() and step_dev.dtype == torch.int32 and step_out.dtype == torch.int32
    else:
        rec = torch.empty(n, 3 + ns + W, device=dev, dtype=torch.float32)
    slot_out, Lcap = None, 0
    if slot_in is not None:
        assert slot_in.dtype == torch.int32 and slot_in.is_contiguous() and slot_in.shape[0] == n
        slot_out, Lcap = torch.empty_like(slot_in), slot_in.shape[1]
    arr = (C.c_void_p * 4)(*[lp.data_ptr() for lp in logps] + [None] * (4 - nf))
    check(_lib.lib().eamd_beam_step_dyn(ptr(pre), ptr(ids), ptr(psi), ptr(c_s), ptr(hyp), w_ctc, nutt, beam, P, V, W, L, step, eos,
                                        ptr(maxlen), ns, nf, ptr(sc_in), arr, ptr(yseq_in), ptr(c_local), ptr(sc_out), ptr(yseq_out),
                                        ptr(hyp_out), ptr(hyp_i), ptr(tok_i), ptr(tok32), ptr(cs_out), ptr(rec), ptr(step_dev),
                                        ptr(step_out), ring, ptr(slot_in), ptr(slot_out), Lcap, stream_ptr()), "eamd_beam_step_dyn")
    if slot_in is not None:       # (a ninth result: the cached decoder's slot table behind the selection)
        return sc_out, yseq_out, hyp_out, hyp_i, tok_i, tok32, cs_out, rec, slot_out
    return sc_out, yseq_out, hyp_out, hyp_i, tok_i, tok32, cs_out, rec


def beam_finish(top_s, top_i, beam, V, L, step, eos, maxlen, sc_in, logps, c_local, full_mode, ids, yseq_in):
    """the bookkeeping of a beam step after the selection in one launch (eamd_beam_finish) ->
    (sc_out [ns, n], yseq_out, hyp_out, hyp_i, tok_i, pos, rec)"""
    n = top_s.numel()
    ns, W = sc_in.shape[0], yseq_in.shape[1]
    nf = len(logps)
    dev = top_s.device
    for t_ in (top_s, sc_in, c_local) + tuple(logps):
        if t_ is not None and (t_.dtype != torch.float32 or not t_.is_contiguous()):
            raise _lib.EamdError("beam_finish: contiguous float32 score tensors")
    for t_ in (top_i, maxlen, ids, yseq_in):
        if t_ is not None and (t_.dtype != torch.int64 or not t_.is_contiguous()):
            raise _lib.EamdError("beam_finish: contiguous int64 index tensors")
    assert top_i.numel() == n and sc_in.shape[1] == n and yseq_in.shape[0] == n and all(lp.shape == (n, V) for lp in logps)
    assert ns in (nf, nf + 1) and (ns == nf or (c_local is not None and c_local.shape[0] == n))
    sc_out = torch.empty(ns, n, device=dev, dtype=torch.float32)
    yseq_out = torch.empty(n, W, device=dev, dtype=torch.int64)
    hyp_out = torch.empty(n, device=dev, dtype=torch.float32)
    hyp_i, tok_i, pos = (torch.empty(n, device=dev, dtype=torch.int64) for _ in range(3))
    rec = torch.empty(n, 3 + ns + W, device=dev, dtype=torch.float32)
    arr = (C.c_void_p * 4)(*[lp.data_ptr() for lp in logps] + [None] * (4 - nf))
    check(_lib.lib().eamd_beam_finish(ptr(top_s), ptr(top_i), n, beam, V, W, L, step, eos, ptr(maxlen), ns, nf, ptr(sc_in), arr,
                                      ptr(c_local), c_local.shape[1] if c_local is not None else 0, bool(full_mode),
                                      ptr(ids), ids.shape[1] if ids is not None else 0, ptr(yseq_in), ptr(sc_out), ptr(yseq_out),
                                      ptr(hyp_out), ptr(hyp_i), ptr(tok_i), ptr(pos), ptr(rec), stream_ptr()), "eamd_beam_finish")
    return sc_out, yseq_out, hyp_out, hyp_i, tok_i, pos, rec


def log_softmax_rows(x, out=None):
    """log-softmax of the rows of x fp32 [rows, V]; out: a contiguous fp32 [rows, V] buffer other than x to write into"""
    rows, V = x.shape
    if out is None:
        y = torch.empty_like(x)
    else:
        if out.dtype != x.dtype or tuple(out.shape) != (rows, V) or not out.is_contiguous() or out.data_ptr() == x.data_ptr():
            raise _lib.EamdError("log_softmax_rows: out contiguous [rows, V] of x's dtype, not x itself")
        y = out
    check(_lib.lib().eamd_log_softmax_rows(ptr(x), ptr(y), rows, V, stream_ptr()), "eamd_log_softmax_rows")
    return y


def transducer_expand_rows(logits, k, lm=None, lm_row=None, pairs=None):
    """one pass of a transducer search (eamd_transducer_expand_rows): logits fp32 [n, V] (row stride >= V, unit column
    stride), blank = 0; lm fp32 [n_lm, V] with lm_row (n host ints), pairs [(row, token)] * g (host)
    -> (rows, pair_logp) on the host through ONE device-to-host copy: rows[r] = (logp[r][0], [(logp, token)] * k best
    non-blank, [raw LM log-probability of each of those tokens] or None); pair_logp[j] = logp[row_j][token_j]"""
    n, V = logits.shape
    if logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise _lib.EamdError("transducer_expand_rows: float32 [n, V] with unit column stride")
    pairs = list(pairs or ())
    if lm is not None:
        lm_row = [int(i) for i in lm_row]
        if lm.dtype != torch.float32 or not lm.is_contiguous() or lm.shape[1] != V or len(lm_row) != n \
                or not all(0 <= i < lm.shape[0] for i in lm_row):
            raise _lib.EamdError("transducer_expand_rows: lm contiguous float32 [n_lm, V], lm_row n indices into it")
    if not all(0 <= r < n and 0 <= tok < V for r, tok in pairs):
        raise _lib.EamdError("transducer_expand_rows: pairs (row < n, token < V)")
    W = 1 + 2 * k + (k if lm is not None else 0)
    g = len(pairs)
    idx = (lm_row if lm is not None else []) + [int(v) for p in pairs for v in p]
    idx_dev = torch.tensor(idx, dtype=torch.int32).to(logits.device, non_blocking=True) if idx else None
    out = torch.empty(n * W + g, device=logits.device, dtype=torch.float32)
    nl = n if lm is not None else 0
    check(_lib.lib().eamd_transducer_expand_rows(
        ptr(logits), logits.stride(0), n, V, k, ptr(lm), ptr(idx_dev) if lm is not None else None,
        ptr(idx_dev, nl) if g else None, g, ptr(out), ptr(out, n * W) if g else None, stream_ptr()),
        "eamd_transducer_expand_rows")
    host = out.tolist()
    rows = []
    for r in range(n):
        rr = host[r * W:(r + 1) * W]
        rows.append((rr[0], list(zip(rr[1:1 + k], (int(v) for v in rr[1 + k:1 + 2 * k]))),
                     rr[1 + 2 * k:] if lm is not None else None))
    return rows, host[n * W:]


def rnnt_greedy_part(B, V, device):
    """the tile-record buffer eamd_rnnt_greedy_joint fills and eamd_rnnt_greedy_pick reads"""
    return torch.empty(_lib.lib().eamd_rnnt_greedy_part_floats(B, V), device=device, dtype=torch.float32)


def rnnt_greedy_joint(enc_proj, d, w_out, b_out, part, act, t, t_dev=None):
    """frame t (or t_dev[0] + t) of a batched greedy transducer search: the joint network's logits of all B rows as per-tile
    (maximum, first token id, sum of exp) records in `part` - the [B, V] logits are never stored.
    enc_proj [B, T, J], d [B, J], w_out [V, J], b_out [V]: contiguous float32"""
    B, T, J = enc_proj.shape
    V = w_out.shape[0]
    for x in (enc_proj, d, w_out, b_out, part):
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise _lib.EamdError("rnnt_greedy_joint: contiguous float32 operands")
    if tuple(d.shape) != (B, J) or tuple(w_out.shape) != (V, J) or b_out.numel() != V \
            or part.numel() < _lib.lib().eamd_rnnt_greedy_part_floats(B, V) \
            or (t_dev is not None and (t_dev.dtype != torch.int32 or t_dev.numel() < 1)):
        raise _lib.EamdError("rnnt_greedy_joint: operand shapes")
    check(_lib.lib().eamd_rnnt_greedy_joint(ptr(enc_proj), ptr(d), ptr(w_out), ptr(b_out), ptr(part), B, T, J, V, act, t,
                                            ptr(t_dev), stream_ptr()), "eamd_rnnt_greedy_joint")


def rnnt_greedy_pick(part, hlens, yseq, ylen, score, tok, live, T, V, blank, t, t_dev=None):
    """the frame's decision and bookkeeping from the tile records: first maximum per row, live = frame < hlens[b] and token !=
    blank; live rows append the token to yseq [B, ycap] int32 at ylen [B] int32, add its log-probability to score [B] float32
    and put it in tok [B] int64 (others: blank); live [B] uint8 is the cell kernels' mask; t_dev[0] += 1 when given"""
    B, ycap = yseq.shape
    ok = (yseq.dtype == torch.int32 and yseq.is_contiguous() and ylen.dtype == torch.int32 and ylen.numel() == B
          and score.dtype == torch.float32 and score.numel() == B and tok.dtype == torch.int64 and tok.numel() == B
          and tok.is_contiguous() and live.dtype == torch.uint8 and live.numel() == B
          and (hlens is None or (hlens.dtype == torch.int32 and hlens.numel() == B))
          and part.dtype == torch.float32 and part.numel() >= _lib.lib().eamd_rnnt_greedy_part_floats(B, V)
          and (t_dev is None or (t_dev.dtype == torch.int32 and t_dev.numel() >= 1)))
    if not ok:
        raise _lib.EamdError("rnnt_greedy_pick: operand types / shapes")
    check(_lib.lib().eamd_rnnt_greedy_pick(ptr(part), ptr(hlens), ptr(yseq), ptr(ylen), ptr(score), ptr(tok), ptr(live), B, T, V,
                                           ycap, blank, t, ptr(t_dev), stream_ptr()), "eamd_rnnt_greedy_pick")


def transducer_expand_rows_dev(logits, k):
    """eamd_transducer_expand_rows without LM and pairs, its record left on the device: logits fp32 [n, V] (unit column stride) ->
    rec fp32 [n, 1 + 2k] = (logp[r][0], the k best non-blank log-probabilities, their token ids as floats).  Nothing is read back."""
    n, V = logits.shape
    if logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise _lib.EamdError("transducer_expand_rows_dev: float32 [n, V] with unit column stride")
    rec = torch.empty(n, 1 + 2 * k, device=logits.device, dtype=torch.float32)
    check(_lib.lib().eamd_transducer_expand_rows(ptr(logits), logits.stride(0), n, V, k, None, None, None, 0, ptr(rec), None,
                                                 stream_ptr()), "eamd_transducer_expand_rows")
    return rec


def transducer_expand_rows_lm_dev(logits, k, lm, lm_row, in_range=False):
    """eamd_transducer_expand_rows with an LM, its record left on the device: logits fp32 [n, V] (unit column stride), lm fp32
    [n_lm, V] contiguous, lm_row int32 [n] on the device -> rec fp32 [n, 1 + 3k] = (logp[r][0], the k best non-blank
    log-probabilities, their token ids as floats, lm[lm_row[r]][token] of each).  The kernel of transducer_expand_rows; nothing is
    read back, so lm_row cannot be checked on the host: it is clamped to lm's rows on the device first (one small launch), unless
    the caller built it itself and says in_range=True (the search loops' iota)."""
    n, V = logits.shape
    if logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise _lib.EamdError("transducer_expand_rows_lm_dev: float32 [n, V] with unit column stride")
    if lm.dtype != torch.float32 or lm.dim() != 2 or not lm.is_contiguous() or lm.shape[1] != V or lm.shape[0] < 1 \
            or lm.device != logits.device or lm_row.dtype != torch.int32 or lm_row.numel() != n or not lm_row.is_contiguous() \
            or lm_row.device != logits.device:
        raise _lib.EamdError("transducer_expand_rows_lm_dev: lm contiguous float32 [n_lm, V], lm_row int32 [n], on the logits' device")
    if not in_range:
        lm_row = lm_row.clamp(0, lm.shape[0] - 1)
    rec = torch.empty(n, 1 + 3 * k, device=logits.device, dtype=torch.float32)
    check(_lib.lib().eamd_transducer_expand_rows(ptr(logits), logits.stride(0), n, V, k, ptr(lm), ptr(lm_row), None, 0, ptr(rec), None,
                                                 stream_ptr()), "eamd_transducer_expand_rows")
    return rec


def rnnt_alsd_step(rec, hlens, state_in, state_out, fin, par, tok, live, frame, V, T, u_max, i, lm_weight=None):
    """step i of the batched alsd transducer search (eamd_rnnt_alsd_step): rec fp32 [n * W, 1 + 2k] of this step's rows, hlens int32
    [n] or None; state_in / state_out = (score float64 [n, W], ulen int32 [n, W], nhyp int32 [n], yseq int32 [n, W, T + u_max + 1])
    of the two parities; fin = (fin_score float64 [n, fcap], fin_len int32 [n, fcap], fin_yseq int32 [n, fcap, u_max + 2], nfin
    int32 [n]) with fcap = W (u_max + 2), appended in place; par int32 / tok int64 / live uint8 / frame int32 [n * W] are written.
    lm_weight (rnnt_alsd_step_lm): eamd_rnnt_alsd_step_lm on the record of width 1 + 3k"""
    n, W = state_in[0].shape
    k = min(W, V - 1)
    fcap = W * (u_max + 2)
    want = [((n, W), torch.float64), ((n, W), torch.int32), ((n,), torch.int32), ((n, W, T + u_max + 1), torch.int32)]
    ok = rec.dtype == torch.float32 and rec.is_contiguous() and tuple(rec.shape) == (n * W, 1 + (2 if lm_weight is None else 3) * k)
    for st in (state_in, state_out):
        ok = ok and all(tuple(x.shape) == s and x.dtype == d and x.is_contiguous() for x, (s, d) in zip(st, want))
    want_f = [((n, fcap), torch.float64), ((n, fcap), torch.int32), ((n, fcap, u_max + 2), torch.int32), ((n,), torch.int32)]
    ok = ok and all(tuple(x.shape) == s and x.dtype == d and x.is_contiguous() for x, (s, d) in zip(fin, want_f))
    ok = ok and all(x.numel() == n * W and x.dtype == d and x.is_contiguous()
                    for x, d in ((par, torch.int32), (tok, torch.int64), (live, torch.uint8), (frame, torch.int32)))
    ok = ok and (hlens is None or (hlens.dtype == torch.int32 and hlens.numel() == n and hlens.is_contiguous()))
    if not ok:
        raise _lib.EamdError("rnnt_alsd_step: operand types / shapes")
    if lm_weight is None:
        check(_lib.lib().eamd_rnnt_alsd_step(ptr(rec), ptr(hlens), *[ptr(x) for x in state_in], *[ptr(x) for x in state_out],
                                             *[ptr(x) for x in fin], ptr(par), ptr(tok), ptr(live), ptr(frame), n, W, V, T, u_max, i,
                                             stream_ptr()), "eamd_rnnt_alsd_step")
    else:
        check(_lib.lib().eamd_rnnt_alsd_step_lm(ptr(rec), ptr(hlens), *[ptr(x) for x in state_in], *[ptr(x) for x in state_out],
                                                *[ptr(x) for x in fin], ptr(par), ptr(tok), ptr(live), ptr(frame), n, W, V, T, u_max,
                                                i, float(lm_weight), stream_ptr()), "eamd_rnnt_alsd_step_lm")


def rnnt_alsd_step_lm(rec, hlens, state_in, state_out, fin, par, tok, live, frame, V, T, u_max, i, lm_weight):
    """rnnt_alsd_step with RNNLM shallow fusion (eamd_rnnt_alsd_step_lm): rec fp32 [n * W, 1 + 3k] as transducer_expand_rows_lm_dev
    leaves it, lm_weight a finite number; the operands and their checks are rnnt_alsd_step's"""
    rnnt_alsd_step(rec, hlens, state_in, state_out, fin, par, tok, live, frame, V, T, u_max, i, float(lm_weight))


def rnnt_tsd_step(rec, hlens, state, A, par, tok, live, V, T, M, t, v, p, lm_weight=None):
    """pass (t, v) of the batched tsd transducer search (eamd_rnnt_tsd_step): rec fp32 [n * W, 1 + 2k] of the rows of C, hlens int32
    [n] or None; state = (score float64 [M + 1, n, W], ulen int32 [M + 1, n, W], count int32 [M + 1, n], yseq int32
    [M + 1, n, W, 1 + T (M - 1)]) - blocks 0 and M are B's parities, p the one frame t reads, block v the C of pass v; A = (a_score
    float64 [n, W M], a_src int32 [n, W M], nA int32 [n]); state and A are updated in place, par int32 / tok int64 / live uint8
    [n * W] are written.  lm_weight (rnnt_tsd_step_lm): eamd_rnnt_tsd_step_lm on the record of width 1 + 3k"""
    blocks, n, W = state[0].shape
    k = min(W, V - 1)
    want = [((M + 1, n, W), torch.float64), ((M + 1, n, W), torch.int32), ((M + 1, n), torch.int32),
            ((M + 1, n, W, 1 + T * (M - 1)), torch.int32)]
    ok = blocks == M + 1 and rec.dtype == torch.float32 and rec.is_contiguous() \
        and tuple(rec.shape) == (n * W, 1 + (2 if lm_weight is None else 3) * k)
    ok = ok and all(tuple(x.shape) == s and x.dtype == d and x.is_contiguous() for x, (s, d) in zip(state, want))
    want_a = [((n, W * M), torch.float64), ((n, W * M), torch.int32), ((n,), torch.int32)]
    ok = ok and all(tuple(x.shape) == s and x.dtype == d and x.is_contiguous() for x, (s, d) in zip(A, want_a))
    ok = ok and all(x.numel() == n * W and x.dtype == d and x.is_contiguous()
                    for x, d in ((par, torch.int32), (tok, torch.int64), (live, torch.uint8)))
    ok = ok and (hlens is None or (hlens.dtype == torch.int32 and hlens.numel() == n and hlens.is_contiguous()))
    if not ok:
        raise _lib.EamdError("rnnt_tsd_step: operand types / shapes")
    if lm_weight is None:
        check(_lib.lib().eamd_rnnt_tsd_step(ptr(rec), ptr(hlens), *[ptr(x) for x in state], *[ptr(x) for x in A], ptr(par), ptr(tok),
                                            ptr(live), n, W, V, T, M, t, v, p, stream_ptr()), "eamd_rnnt_tsd_step")
    else:
        check(_lib.lib().eamd_rnnt_tsd_step_lm(ptr(rec), ptr(hlens), *[ptr(x) for x in state], *[ptr(x) for x in A], ptr(par),
                                               ptr(tok), ptr(live), n, W, V, T, M, t, v, p, float(lm_weight), stream_ptr()),
              "eamd_rnnt_tsd_step_lm")


def rnnt_tsd_step_lm(rec, hlens, state, A, par, tok, live, V, T, M, t, v, p, lm_weight):
    """rnnt_tsd_step with RNNLM shallow fusion (eamd_rnnt_tsd_step_lm): rec fp32 [n * W, 1 + 3k] as transducer_expand_rows_lm_dev
    leaves it, lm_weight a finite number; the operands and their checks are rnnt_tsd_step's"""
    rnnt_tsd_step(rec, hlens, state, A, par, tok, live, V, T, M, t, v, p, float(lm_weight))


def transducer_expand_rows_pairs_dev(logits, k, pairs, pair_out):
    """eamd_transducer_expand_rows without LM, its record and the pair log-probabilities left on the device: logits fp32 [n, V] (unit
    column stride), pairs int32 [g, 2] on the device (row, token; a row that is no row of logits is skipped), pair_out fp32 [g] ->
    rec fp32 [n, 1 + 2k]; pair_out[j] = logp[row_j][token_j].  Nothing is read back."""
    n, V = logits.shape
    if logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise _lib.EamdError("transducer_expand_rows_pairs_dev: float32 [n, V] with unit column stride")
    g = pair_out.numel()
    if pairs.dtype != torch.int32 or not pairs.is_contiguous() or pairs.numel() != 2 * g or g < 1 \
            or pair_out.dtype != torch.float32 or not pair_out.is_contiguous():
        raise _lib.EamdError("transducer_expand_rows_pairs_dev: pairs int32 [g, 2], pair_out float32 [g], contiguous")
    rec = torch.empty(n, 1 + 2 * k, device=logits.device, dtype=torch.float32)
    check(_lib.lib().eamd_transducer_expand_rows(ptr(logits), logits.stride(0), n, V, k, None, None, ptr(pairs), g, ptr(rec),
                                                 ptr(pair_out), stream_ptr()), "eamd_transducer_expand_rows")
    return rec


def rnnt_nsc_step(rec, pair_lp, hlens, state, S, par, tok, live, hidx, pairs, V, T, N, alpha, t, v, p):
    """call (t, v) of the batched nsc transducer search (eamd_rnnt_nsc_step): rec fp32 [n * W, 1 + 2k] of the rows of hyps' block,
    pair_lp fp32 [max(1, n * W * alpha)] of the frame's first pass, hlens int32 [n] or None; state = (score float64 [N + 2, n, W],
    ulen int32 [N + 2, n, W], count int32 [N + 2, n], yseq int32 [N + 2, n, W, 1 + T N]) - blocks 0 and N + 1 are kept's parities, p
    the one frame t reads, block v the hyps of n-step v; S = (s_score float64 [n, W N], s_src int32 [n, W N], nS int32 [n]); state
    and S are updated in place, par int32 / tok int64 / live uint8 [n * W], hidx int32 [1 + alpha, n * W] and, on a frame's last
    call, pairs int32 [max(1, n * W * alpha), 2] are written"""
    blocks, n, W = state[0].shape
    k = min(W, V - 1)
    g = max(1, n * W * alpha)
    want = [((N + 2, n, W), torch.float64), ((N + 2, n, W), torch.int32), ((N + 2, n), torch.int32),
            ((N + 2, n, W, 1 + T * N), torch.int32)]
    ok = blocks == N + 2 and rec.dtype == torch.float32 and rec.is_contiguous() and tuple(rec.shape) == (n * W, 1 + 2 * k)
    ok = ok and all(tuple(x.shape) == s and x.dtype == d and x.is_contiguous() for x, (s, d) in zip(state, want))
    want_s = [((n, W * N), torch.float64), ((n, W * N), torch.int32), ((n,), torch.int32)]
    ok = ok and all(tuple(x.shape) == s and x.dtype == d and x.is_contiguous() for x, (s, d) in zip(S, want_s))
    ok = ok and all(x.numel() == n * W and x.dtype == d and x.is_contiguous()
                    for x, d in ((par, torch.int32), (tok, torch.int64), (live, torch.uint8)))
    ok = ok and alpha >= 0 and hidx.dtype == torch.int32 and hidx.is_contiguous() and tuple(hidx.shape) == (1 + alpha, n * W)
    ok = ok and pairs.dtype == torch.int32 and pairs.is_contiguous() and tuple(pairs.shape) == (g, 2)
    ok = ok and pair_lp.dtype == torch.float32 and pair_lp.is_contiguous() and pair_lp.numel() == g
    ok = ok and (hlens is None or (hlens.dtype == torch.int32 and hlens.numel() == n and hlens.is_contiguous()))
    if not ok:
        raise _lib.EamdError("rnnt_nsc_step: operand types / shapes")
    check(_lib.lib().eamd_rnnt_nsc_step(ptr(rec), ptr(pair_lp), ptr(hlens), *[ptr(x) for x in state], *[ptr(x) for x in S], ptr(par),
                                        ptr(tok), ptr(live), ptr(hidx), ptr(pairs), n, W, V, T, N, alpha, t, v, p, stream_ptr()),
          "eamd_rnnt_nsc_step")


def gather_rows(jobs):
    """row gathers, sixteen per launch (eamd_gather_rows): jobs = [(dst [r, w], src [m, w], idx int32 [r])], any positive number of
    them, contiguous fp32 matrices on the device: dst[i] = src[idx[i]]"""
    assert len(jobs) > 0
    for d, s_, ix in jobs:
        if not (d.dtype == s_.dtype == torch.float32 and d.is_contiguous() and s_.is_contiguous() and d.dim() == s_.dim() == 2
                and d.shape[1] == s_.shape[1] and ix.dtype == torch.int32 and ix.is_contiguous() and ix.numel() == d.shape[0]
                and s_.shape[0] >= 1):
            raise _lib.EamdError("gather_rows: contiguous float32 [rows, width] matrices of one width, int32 indices")
    for j0 in range(0, len(jobs), 16):
        part = jobs[j0:j0 + 16]
        n = len(part)
        src = (C.c_void_p * n)(*[s_.data_ptr() for _, s_, _ in part])
        dst = (C.c_void_p * n)(*[d.data_ptr() for d, _, _ in part])
        idx = (C.c_void_p * n)(*[ix.data_ptr() for _, _, ix in part])
        nrows = (C.c_int32 * n)(*[d.shape[0] for d, _, _ in part])
        width = (C.c_int32 * n)(*[d.shape[1] for d, _, _ in part])
        srows = (C.c_int32 * n)(*[s_.shape[0] for _, s_, _ in part])
        check(_lib.lib().eamd_gather_rows(src, dst, idx, nrows, width, srows, n, stream_ptr()), "eamd_gather_rows")


def rnnt_default_step(rec, hlens, A, B, cur_score, ctr, log, flags, par, tok, dst, live, frame, alive, W, V, T):
    """one pop of the batched default transducer search (eamd_rnnt_default_step): rec fp32 [n, 1 + 2k] of the pending pops' joint
    rows, hlens int32 [n] or None; A = (a_score float64 [n, P], a_seq, a_row, a_log, a_tok int32 [n, P]), B = (b_score float64 [n, P],
    b_row, b_log int32 [n, P]), cur_score float64 [n], ctr int32 [n, 8], log int32 [n, log_cap, 2], flags int32 [2, n]: updated in
    place; par int32 / tok int64 / dst int32 / live uint8 / frame int32 / alive uint8 [n] are written"""
    n, P = A[0].shape
    k = min(W, V - 1)
    want_a = [torch.float64] + [torch.int32] * 4
    want_b = [torch.float64] + [torch.int32] * 2
    ok = rec.dtype == torch.float32 and rec.is_contiguous() and tuple(rec.shape) == (n, 1 + 2 * k)
    ok = ok and len(A) == 5 and len(B) == 3
    ok = ok and all(tuple(x.shape) == (n, P) and x.dtype == d and x.is_contiguous() for x, d in zip(tuple(A) + tuple(B), want_a + want_b))
    ok = ok and cur_score.dtype == torch.float64 and cur_score.numel() == n and cur_score.is_contiguous()
    ok = ok and ctr.dtype == torch.int32 and tuple(ctr.shape) == (n, 8) and ctr.is_contiguous()
    ok = ok and log.dtype == torch.int32 and log.dim() == 3 and log.shape[0] == n and log.shape[2] == 2 and log.is_contiguous()
    ok = ok and flags.dtype == torch.int32 and tuple(flags.shape) == (2, n) and flags.is_contiguous()
    ok = ok and all(x.numel() == n and x.dtype == d and x.is_contiguous()
                    for x, d in ((par, torch.int32), (tok, torch.int64), (dst, torch.int32), (live, torch.uint8),
                                 (frame, torch.int32), (alive, torch.uint8)))
    ok = ok and (hlens is None or (hlens.dtype == torch.int32 and hlens.numel() == n and hlens.is_contiguous()))
    if not ok:
        raise _lib.EamdError("rnnt_default_step: operand types / shapes")
    check(_lib.lib().eamd_rnnt_default_step(ptr(rec), ptr(hlens), *[ptr(x) for x in A], *[ptr(x) for x in B], ptr(cur_score), ptr(ctr),
                                            ptr(log), ptr(flags), ptr(par), ptr(tok), ptr(dst), ptr(live), ptr(frame), ptr(alive),
                                            n, W, V, T, P, k, log.shape[1], stream_ptr()), "eamd_rnnt_default_step")


def scatter_rows(jobs):
    """masked row scatters, sixteen per launch (eamd_scatter_rows): jobs = [(dst [m, w], src [r, w], idx int32 [r], mask uint8 [r]
    or None)], any positive number of them, contiguous fp32 matrices on the device: dst[idx[i]] = src[i] where mask[i] != 0; an
    index outside dst writes nothing"""
    assert len(jobs) > 0
    for d, s_, ix, m in jobs:
        if not (d.dtype == s_.dtype == torch.float32 and d.is_contiguous() and s_.is_contiguous() and d.dim() == s_.dim() == 2
                and d.shape[1] == s_.shape[1] and ix.dtype == torch.int32 and ix.is_contiguous() and ix.numel() == s_.shape[0]
                and d.shape[0] >= 1 and (m is None or (m.dtype == torch.uint8 and m.is_contiguous() and m.numel() == s_.shape[0]))):
            raise _lib.EamdError("scatter_rows: contiguous float32 [rows, width] matrices of one width, int32 indices, uint8 masks")
    for j0 in range(0, len(jobs), 16):
        part = jobs[j0:j0 + 16]
        n = len(part)
        dst = (C.c_void_p * n)(*[d.data_ptr() for d, _, _, _ in part])
        src = (C.c_void_p * n)(*[s_.data_ptr() for _, s_, _, _ in part])
        idx = (C.c_void_p * n)(*[ix.data_ptr() for _, _, ix, _ in part])
        mask = (C.c_void_p * n)(*[ptr(m) for _, _, _, m in part])
        nrows = (C.c_int32 * n)(*[s_.shape[0] for _, s_, _, _ in part])
        width = (C.c_int32 * n)(*[d.shape[1] for d, _, _, _ in part])
        drows = (C.c_int32 * n)(*[d.shape[0] for d, _, _, _ in part])
        check(_lib.lib().eamd_scatter_rows(dst, src, idx, mask, nrows, width, drows, n, stream_ptr()), "eamd_scatter_rows")


def linear_into(x, W, b, out):
    """out[M, N] = x W^T + b into a caller-owned buffer (the static buffers a replayed decoding step reads and writes): the
    few-row kernel of linear_fwd where it takes the shape, else the GEMM"""
    M, K = x.shape
    N = W.shape[0]
    assert W.shape[1] == K and W.is_contiguous() and x.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (M, N)
    if x.dtype != torch.float32 or W.dtype != torch.float32 or out.dtype != torch.float32:
        raise _lib.EamdError("linear_into: float32 operands")
    if (LINEAR_ROWS and K % 4 == 0 and _state["precision"] == 0
            and (M <= LINEAR_ROWS_MAX or (M <= LINEAR_ROWS_BLOCK_MAX and K <= 512 and N <= 1024 and K % 16 == 0))):
        rc = _lib.lib().eamd_linear_rows_f32(ptr(x), ptr(W), ptr(b), None, ptr(out), M, N, K, ACT_NONE, EPI_NONE, 1.0, K, 0,
                                             stream_ptr())
        if rc == 0:
            return out
        if rc != _lib.EAMD_EUNSUPPORTED:
            check(rc, "eamd_linear_rows_f32")
    gemm(x, W, out, M, N, K, K, K, N, bias=b)
    return out


# ---- element-wise ------------------------------------------------------------------------------
def axpby(x, y, a=1.0, b=1.0, out=None):
    if out is None:
        out = torch.empty_like(x)
    assert y is None or y.numel() == x.numel()
    check(_lib.lib().eamd_axpby(ptr(x), ptr(y), ptr(out), x.numel(), a, b,
                                stream_ptr()), "eamd_axpby")
    return out


def scale_dev(x, scale_t, extra=1.0, out=None):
    if out is None:
        out = torch.empty_like(x)
    check(_lib.lib().eamd_scale_dev(ptr(x), ptr(scale_t), ptr(out), x.numel(), extra,
                                    stream_ptr()), "eamd_scale_dev")
    return out


def glu_fwd(a, Cc):
    rows = a.shape[0]
    y = torch.empty(rows, Cc, device=a.device, dtype=torch.float32)
    check(_lib.lib().eamd_glu_fwd(ptr(a), ptr(y), rows, Cc, stream_ptr()), "eamd_glu_fwd")
    return y


def glu_bwd(dy, a, Cc, out_dtype=torch.float32):
    rows = a.shape[0]
    dx = torch.empty(a.shape, device=a.device, dtype=out_dtype)
    d32, d16 = (ptr(dx), None) if out_dtype == torch.float32 else (None, ptr(dx))
    check(_lib.lib().eamd_glu_bwd(ptr(dy), ptr(a), d32, d16, rows, Cc, stream_ptr()), "eamd_glu_bwd")
    return dx


def add_bias2(q, u, v, rows=None, D=None, ldq=None, q_off=0):
    """qu = q + u, qv = q + v (dense [rows, D] outputs); q may be a column block (q_off, ldq) of a wider matrix"""
    if rows is None:
        rows, D = q.shape
    ldq = D if ldq is None else ldq
    assert u.numel() == D and v.numel() == D and q.numel() >= q_off + (rows - 1) * ldq + D
    qu = torch.empty(rows, D, device=q.device, dtype=q.dtype)
    qv = torch.empty(rows, D, device=q.device, dtype=q.dtype)
    check(_lib.lib().eamd_add_bias2(ptr(q, q_off), ldq, ptr(u), ptr(v), ptr(qu), ptr(qv), rows, D,
                                    1 if q.dtype == torch.bfloat16 else 0, stream_ptr()), "eamd_add_bias2")
    return qu, qv


def add_cast(a, b, out=None, out_off=0, ld_out=None):
    """bf16(a + b) from dense fp32 [rows, cols] inputs (b optional); optionally into a column block of `out`
    (an fp32 `out` takes the sum as it is)"""
    rows, cols = a.shape
    if out is None:
        out = torch.empty(a.shape, device=a.device, dtype=torch.bfloat16)
        ld_out = cols
    if out.dtype == torch.float32:
        assert out.numel() >= out_off + (rows - 1) * ld_out + cols
        check(_lib.lib().eamd_add_block_f32(ptr(a), ptr(b), ptr(out, out_off), rows, cols, ld_out,
                                            stream_ptr()), "eamd_add_block_f32")
        return out
    assert out.dtype == torch.bfloat16 and out.numel() >= out_off + (rows - 1) * ld_out + cols
    check(_lib.lib().eamd_add_cast_bf16(ptr(a), ptr(b), ptr(out, out_off), rows, cols, ld_out,
                                        stream_ptr()), "eamd_add_cast_bf16")
    return out


def add_cast_colsum2(a, b, suma, sumb, out=None, out_off=0, ld_out=None):
    """a + b in the operand dtype (bf16 in fast mode, fp32 otherwise; optionally into a column block of `out`) and
    suma += column sums of a, sumb += column sums of b in one pass; falls back to add_cast + two colsum launches for
    widths the fused kernel does not take"""
    rows, cols = a.shape
    if out is None:
        out = torch.empty(a.shape, device=a.device, dtype=act_dtype())
        ld_out = cols
    assert out.dtype in (torch.bfloat16, torch.float32) and out.numel() >= out_off + (rows - 1) * ld_out + cols
    assert a.is_contiguous() and b.is_contiguous() and suma.numel() == cols and sumb.numel() == cols
    L = _lib.lib()
    fn, name = ((L.eamd_add_cast_colsum2, "eamd_add_cast_colsum2") if out.dtype == torch.bfloat16
                else (L.eamd_add_colsum2_f32, "eamd_add_colsum2_f32"))
    rc = fn(ptr(a), ptr(b), ptr(out, out_off), ld_out, ptr(suma), ptr(sumb), rows, cols, stream_ptr())
    if rc == _lib.EAMD_EUNSUPPORTED:
        colsum(a, suma)
        colsum(b, sumb)
        return add_cast(a, b, out=out, out_off=out_off, ld_out=ld_out)
    check(rc, name)
    return out


def embed_pe(tok, table, pe, U, scale, pos_offset=0, pos_dev=None):
    """out[r] = table[tok[r]] * scale + pe[r % U + pos_offset]   (pe None: plain embedding lookup).  tok contiguous, or one
    column of a wider buffer ([n, 1] with a row stride: the newest tokens of a beam step's prefixes)"""
    rows = tok.numel()
    D = table.shape[1]
    assert tok.dtype == torch.int64
    ldt = 1
    if not tok.is_contiguous():
        assert tok.dim() == 2 and tok.shape[1] == 1 and tok.stride(0) >= 1
        ldt = tok.stride(0)
    assert pe is None or (pe.shape[0] >= U + pos_offset and pe.shape[1] == D)
    out = torch.empty(rows, D, device=table.device, dtype=torch.float32)
    # pos_dev: int32 device scalar added to pos_offset (the step index of a replayed beam step)
    check(_lib.lib().eamd_embed_pe_dyn(ptr(tok), ldt, ptr(table), ptr(pe), ptr(out), rows, U, D,
                                       scale, pos_offset, ptr(pos_dev), stream_ptr()), "eamd_embed_pe_dyn")
    return out


def embed_bwd(tok, dout, dtable, scale, pad_idx=-1):
    rows, D = dout.shape
    check(_lib.lib().eamd_embed_bwd(ptr(tok), ptr(dout), ptr(dtable), rows, D, scale,
                                    pad_idx, stream_ptr()), "eamd_embed_bwd")


def posenc(x, pe, T, scale):
    rows, D = x.shape
    assert pe.shape[0] >= T and pe.shape[1] == D
    out = torch.empty_like(x)
    check(_lib.lib().eamd_posenc(ptr(x), ptr(pe), ptr(out), rows, T, D, scale, stream_ptr()),
          "eamd_posenc")
    return out


def posenc_scaled(x, pe, alpha, T, scale=1.0):
    rows, D = x.shape
    assert pe.shape[0] >= T and pe.shape[1] == D and alpha.numel() == 1
    out = torch.empty_like(x)
    check(_lib.lib().eamd_posenc_scaled(ptr(x), ptr(pe), ptr(alpha), ptr(out), rows, T, D, scale,
                                        stream_ptr()), "eamd_posenc_scaled")
    return out


def posenc_scaled_bwd(dout, pe, dalpha, T):
    rows, D = dout.shape
    check(_lib.lib().eamd_posenc_scaled_bwd(ptr(dout), ptr(pe), ptr(dalpha), rows, T, D, stream_ptr()),
          "eamd_posenc_scaled_bwd")


_rng = {"step": None, "salt": 0}


def rng_state(device):
    """device-resident step counter that seeds every dropout mask of the current training step"""
    st = _rng["step"]
    if st is None or st.device != torch.device(device):
        st = torch.zeros(1, device=device, dtype=torch.int64)
        _rng["step"] = st
    return st


def rng_advance(device):
    check(_lib.lib().eamd_rng_advance(ptr(rng_state(device)), stream_ptr()), "eamd_rng_advance")


def manual_seed(seed, device="cuda"):
    rng_state(device).fill_(int(seed))


def new_salt():
    """unique id for a dropout site (module instance x use); masks of different sites are independent"""
    _rng["salt"] += 1
    return _rng["salt"]


def dropout(x, p, salt, act=ACT_NONE, out_dtype=None):
    """y = act(x) * mask / (1-p); calling it again with the same salt in the same step re-applies the
    same mask (that is the backward pass).  x fp32 or bf16."""
    out_dtype = x.dtype if out_dtype is None else out_dtype
    y = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    check(_lib.lib().eamd_dropout(ptr(x), ptr(y), x.numel(), p, ptr(rng_state(x.device)),
                                  salt, act, 1 if x.dtype == torch.bfloat16 else 0,
                                  1 if out_dtype == torch.bfloat16 else 0, stream_ptr()), "eamd_dropout")
    return y


# ---- convolution module --------------------------------------------------------------------------
def dwconv_fwd(x, w, bias, B, T, Cc, K):
    assert x.numel() == B * T * Cc and w.numel() == Cc * K
    y = torch.empty_like(x)
    check(_lib.lib().eamd_dwconv_fwd(ptr(x), ptr(w), ptr(bias), ptr(y), B, T, Cc, K, stream_ptr()),
          "eamd_dwconv_fwd")
    return y


def dwconv_bwd_x(dy, w, B, T, Cc, K):
    dx = torch.empty_like(dy)
    check(_lib.lib().eamd_dwconv_bwd_x(ptr(dy), ptr(w), ptr(dx), B, T, Cc, K, stream_ptr()), "eamd_dwconv_bwd_x")
    return dx


def dwconv_bwd_w(dy, x, dw, db, B, T, Cc, K):
    assert dw.numel() == Cc * K and (db is None or db.numel() == Cc)
    check(_lib.lib().eamd_dwconv_bwd_w(ptr(dy), ptr(x), ptr(dw), ptr(db), B, T, Cc, K, stream_ptr()),
          "eamd_dwconv_bwd_w")


def dwconv_glu_fwd(a, w, bias, B, T, Cc, K, bn=None):
    """y [B*T, Cc] = dwconv(GLU(a)) for a [B*T, 2*Cc] (value | gate columns): GLU(a) is formed on load, never written.
    bn = (eps, momentum, running_mean, running_var, num_batches_tracked): training-mode BatchNorm statistics of y from
    the same launch (partials in its epilogue + eamd_bn_finalize) -> (y, mean, rstd).
    Returns None when the library declines (kernel size beyond the LDS-tiled kernel)."""
    assert a.numel() == B * T * 2 * Cc and w.numel() == Cc * K and a.dtype == torch.float32
    y = torch.empty(B * T, Cc, device=a.device, dtype=torch.float32)
    nslab = B * ((T + 63) // 64)
    part = torch.empty(3 * Cc * nslab, device=a.device, dtype=torch.float32) if bn is not None else None
    rc = _lib.lib().eamd_dwconv_glu_fwd(ptr(a), ptr(w), ptr(bias), ptr(y), ptr(part), B, T, Cc, K, stream_ptr())
    if rc == _lib.EAMD_EUNSUPPORTED:
        return None
    check(rc, "eamd_dwconv_glu_fwd")
    if bn is None:
        return y
    eps, momentum, running_mean, running_var, nbt = bn
    mean = torch.empty(Cc, device=a.device, dtype=torch.float32)
    rstd = torch.empty(Cc, device=a.device, dtype=torch.float32)
    check(_lib.lib().eamd_bn_finalize(ptr(part), nslab, ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var), ptr(nbt), Cc,
                                      eps, momentum, stream_ptr()), "eamd_bn_finalize")
    return y, mean, rstd


def dwconv_glu_bwd_x(dy, w, a, B, T, Cc, K, out_dtype=torch.float32):
    """da [B*T, 2*Cc] = GLU'(a) . dwconv_bwd_x(dy): the gradient of the GLU output is never written"""
    da = torch.empty(a.shape, device=a.device, dtype=out_dtype)
    check(_lib.lib().eamd_dwconv_glu_bwd_x(ptr(dy), ptr(w), ptr(a), ptr(da), int(out_dtype == torch.bfloat16), B, T, Cc, K,
                                           stream_ptr()), "eamd_dwconv_glu_bwd_x")
    return da


def dwconv_glu_bwd_w(dy, a, dw, db, B, T, Cc, K):
    assert dw.numel() == Cc * K and (db is None or db.numel() == Cc)
    check(_lib.lib().eamd_dwconv_glu_bwd_w(ptr(dy), ptr(a), ptr(dw), ptr(db), B, T, Cc, K, stream_ptr()),
          "eamd_dwconv_glu_bwd_w")


def bn_stats(x, M, Cc, eps, momentum, running_mean, running_var, num_batches_tracked=None, bound=None):
    """bound = (T, int32 device scalar): rows (b, t) with t >= bound[0] are left out (eamd_bn_stats_bounded)"""
    nslab = _lib.lib().eamd_bn_nslab(M, Cc)
    ws = torch.empty(3 * Cc * nslab, device=x.device, dtype=torch.float32)
    mean = torch.empty(Cc, device=x.device, dtype=torch.float32)
    rstd = torch.empty(Cc, device=x.device, dtype=torch.float32)
    assert num_batches_tracked is None or (num_batches_tracked.dtype == torch.int64 and num_batches_tracked.is_cuda)
    if bound is not None:
        check(_lib.lib().eamd_bn_stats_bounded(ptr(x), ptr(ws), ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var),
                                               ptr(num_batches_tracked), M, Cc, eps, momentum,
                                               int(bound[0]), ptr(bound[1]), stream_ptr()), "eamd_bn_stats_bounded")
        return mean, rstd
    check(_lib.lib().eamd_bn_stats(ptr(x), ptr(ws), ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var),
                                   ptr(num_batches_tracked), M, Cc, eps, momentum, stream_ptr()),
          "eamd_bn_stats")
    return mean, rstd


def bn_apply(x, mean, rstd, gamma, beta, M, Cc, act, out_dtype=torch.float32):
    y = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    check(_lib.lib().eamd_bn_apply(ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(y), M, Cc,
                                   act, 1 if out_dtype == torch.bfloat16 else 0, stream_ptr()), "eamd_bn_apply")
    return y


def bn_bwd(dy, x, mean, rstd, gamma, beta, dgamma, dbeta, M, Cc, act, training, bound=None):
    nslab = _lib.lib().eamd_bn_nslab(M, Cc)
    ws = torch.empty((2 * nslab + 2) * Cc, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    if bound is not None:
        check(_lib.lib().eamd_bn_bwd_bounded(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(ws), ptr(dx),
                                             ptr(dgamma), ptr(dbeta), M, Cc, act, int(training), int(bound[0]),
                                             ptr(bound[1]), stream_ptr()), "eamd_bn_bwd_bounded")
        return dx
    check(_lib.lib().eamd_bn_bwd(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(ws), ptr(dx),
                                 ptr(dgamma), ptr(dbeta), M, Cc, act, int(training), stream_ptr()),
          "eamd_bn_bwd")
    return dx


def conv1_fwd(x, w, bias, B, T, F, Cc, out_dtype=torch.float32):
    H, W = (T - 3) // 2 + 1, (F - 3) // 2 + 1
    assert x.numel() == B * T * F and w.numel() == Cc * 9
    y = torch.empty(B, H, W, Cc, device=x.device, dtype=out_dtype)
    check(_lib.lib().eamd_conv1_fwd(ptr(x), ptr(w), ptr(bias), ptr(y), B, T, F, Cc,
                                    1 if out_dtype == torch.bfloat16 else 0, stream_ptr()), "eamd_conv1_fwd")
    return y


def conv1_bwd_w(dy, x, dw, db, B, T, F, Cc):
    L = _lib.lib()
    ws = torch.empty(L.eamd_conv1_bwd_w_workspace(B, T, Cc), device=x.device, dtype=torch.float32)
    check(L.eamd_conv1_bwd_w(ptr(dy), ptr(x), ptr(dw), ptr(db), ptr(ws), B, T, F, Cc,
                             1 if dy.dtype == torch.bfloat16 else 0, stream_ptr()), "eamd_conv1_bwd_w")


def conv2_weight_prep(w, out_dtype=torch.float32):
    Co, Ci = w.shape[0], w.shape[1]
    wf = torch.empty(9, Ci, Co, device=w.device, dtype=out_dtype)
    wd = torch.empty(9, Co, Ci, device=w.device, dtype=out_dtype)
    check(_lib.lib().eamd_conv2_weight_prep(ptr(w), ptr(wf), ptr(wd), Co, Ci,
                                            1 if out_dtype == torch.bfloat16 else 0, stream_ptr()),
          "eamd_conv2_weight_prep")
    return wf, wd


def conv2_weight_grad(dwf, dw, Co, Ci):
    check(_lib.lib().eamd_conv2_weight_grad(ptr(dwf), ptr(dw), Co, Ci, stream_ptr()), "eamd_conv2_weight_grad")


def permute4(src, dst, dims, dst_strides, accumulate=False):
    d0, d1, d2, d3 = dims
    s0, s1, s2, s3 = dst_strides
    assert src.numel() == d0 * d1 * d2 * d3
    assert (d0 - 1) * s0 + (d1 - 1) * s1 + (d2 - 1) * s2 + (d3 - 1) * s3 < dst.numel()
    check(_lib.lib().eamd_permute4(ptr(src), ptr(dst), d0, d1, d2, d3, s0, s1, s2,
                                   s3, int(accumulate), stream_ptr()), "eamd_permute4")


# ---- integer helpers ----------------------------------------------------------------------------
def add_sos_eos(ys_pad, sos, eos, ignore_id):
    B, L = ys_pad.shape
    assert ys_pad.dtype == torch.int64 and ys_pad.is_contiguous()
    ys_in = torch.empty(B, L + 1, device=ys_pad.device, dtype=torch.int64)
    ys_out = torch.empty(B, L + 1, device=ys_pad.device, dtype=torch.int64)
    olen = torch.empty(B, device=ys_pad.device, dtype=torch.int32)
    check(_lib.lib().eamd_add_sos_eos(ptr(ys_pad), ptr(ys_in), ptr(ys_out), ptr(olen), B, L, sos, eos, ignore_id,
                                      stream_ptr()), "eamd_add_sos_eos")
    return ys_in, ys_out, olen


def ctc_collapse(ids, hlens, blank):
    B, T = ids.shape
    assert ids.dtype == torch.int32 and ids.is_contiguous()
    out = torch.empty(B, T, device=ids.device, dtype=torch.int32)
    outlen = torch.empty(B, device=ids.device, dtype=torch.int32)
    check(_lib.lib().eamd_ctc_collapse(ptr(ids), ptr(hlens), ptr(out), ptr(outlen), B, T, blank, stream_ptr()),
          "eamd_ctc_collapse")
    return out, outlen


TEXT_CHARS, TEXT_WORDS = 0, 1      # include/espnet_amd.h: EAMD_TEXT_CHARS / EAMD_TEXT_WORDS


def text_units(ids, tok_off, tok_cp, cap, limit=None, collapse=False, drop_cp=-1, mode=TEXT_CHARS):
    """padded id rows -> symbol rows (eamd_text_units): ids [B,L] int32 (-1 padding), limit [B] int32 or None, the token
    table tok_off [V+1] / tok_cp int32 (CSR of code points), cap >= L * longest token -> out [B,cap] int64, outlen [B] int32"""
    B, L = ids.shape
    assert ids.dtype == torch.int32 and ids.is_contiguous() and tok_off.dtype == torch.int32 and tok_cp.dtype == torch.int32
    assert limit is None or (limit.dtype == torch.int32 and limit.numel() == B)
    V = tok_off.numel() - 1
    dev = ids.device
    scratch = torch.empty(B, cap, device=dev, dtype=torch.int32)
    out = torch.empty(B, cap, device=dev, dtype=torch.int64)
    outlen = torch.empty(B, device=dev, dtype=torch.int32)
    check(_lib.lib().eamd_text_units(ptr(ids), ptr(limit), ptr(tok_off), ptr(tok_cp), ptr(scratch), ptr(out), ptr(outlen),
                                     B, L, V, cap, bool(collapse), int(drop_cp), int(mode), stream_ptr()),
          "eamd_text_units")
    return out, outlen


def edit_distance(a, alen, b, blen):
    """batched Levenshtein distance (eamd_edit_distance): a [B,lda], b [B,ldb] int64 symbols, alen / blen [B] int32
    -> dist [B] int32"""
    B, lda = a.shape
    ldb = b.shape[1]
    assert a.dtype == torch.int64 and b.dtype == torch.int64 and a.is_contiguous() and b.is_contiguous() and b.shape[0] == B
    assert alen.dtype == torch.int32 and blen.dtype == torch.int32 and alen.numel() == B and blen.numel() == B
    ws_bytes = _lib.lib().eamd_edit_distance_workspace_bytes(B, lda, ldb)
    ws = torch.empty(ws_bytes, device=a.device, dtype=torch.uint8)
    dist = torch.empty(B, device=a.device, dtype=torch.int32)
    check(_lib.lib().eamd_edit_distance(ptr(a), lda, ptr(alen), ptr(b), ldb, ptr(blen), ptr(dist), ptr(ws),
                                        ws_bytes, B, stream_ptr()), "eamd_edit_distance")
    return dist


def ngram_score(lm, ctx_prev, tok, first=False):
    """the n-gram LM's rows of n hypotheses in one launch (eamd_ngram_score).  lm: the tables of nets.ngram.ArpaLM, on the device;
    ctx_prev [n, N-1] int32 word ids, most recent first, -1 = empty (a row stride of 0 - one row expanded - is read in place);
    tok [n] int64, any stride (ys[:, -1] needs no copy): the newest token of every row; first: the newest word is <s>
    -> (logp [n, V] fp32 log10-probabilities, ctx_new [n, N-1] int32)"""
    n, Cw = ctx_prev.shape
    V = lm.uni_tok.numel()
    assert Cw == lm.order - 1 and ctx_prev.dtype == torch.int32 and (Cw == 0 or ctx_prev.stride(1) == 1)
    assert tok.dtype == torch.int64 and tok.dim() == 1 and tok.numel() == n
    dev = tok.device
    if lm.uni_tok.device != dev or ctx_prev.device != dev:
        raise _lib.EamdError("ngram_score: tables, contexts and tokens on one device")
    logp = torch.empty(n, V, device=dev, dtype=torch.float32)
    ctx_new = torch.empty(n, Cw, device=dev, dtype=torch.int32)
    check(_lib.lib().eamd_ngram_score(
        ptr(lm.tok2word), ptr(lm.uni_tok), ptr(lm.node_bo), ptr(lm.child_start), ptr(lm.child_word), ptr(lm.child_node),
        ptr(lm.succ_start), ptr(lm.succ_tok), ptr(lm.succ_lp), lm.node_bo.numel(), V, lm.order, lm.bos, lm.unk,
        ptr(ctx_prev) if Cw else None, ctx_prev.stride(0) if Cw else 0, ptr(tok), tok.stride(0) if n > 1 else 1,
        bool(first), ptr(logp), ptr(ctx_new) if Cw else None, n, stream_ptr()), "eamd_ngram_score")
    return logp, ctx_new


def _ngram_query_args(lm):
    """the table arguments eamd_ngram_score_pairs and eamd_ctc_prefix_beam share"""
    return (ptr(lm.tok2word), ptr(lm.uni_tok), ptr(lm.node_bo), ptr(lm.child_start), ptr(lm.child_word), ptr(lm.child_node),
            ptr(lm.succ_start), ptr(lm.qsucc_tok), ptr(lm.qsucc_lp), lm.node_bo.numel())


def ngram_score_pairs(lm, ctx, tok):
    """point queries on the n-gram LM (eamd_ngram_score_pairs): ctx [n, N-1] int32 contexts (most recent word first, -1 = empty),
    tok [n] int64 -> (lp [n] = log10 p(word(tok) | ctx), bit-equal to the element of ngram_score's row, ctx_new [n, N-1])"""
    n, Cw = ctx.shape
    V = lm.uni_tok.numel()
    assert Cw == lm.order - 1 and ctx.dtype == torch.int32 and ctx.is_contiguous()
    assert tok.dtype == torch.int64 and tok.dim() == 1 and tok.numel() == n and tok.is_contiguous()
    dev = tok.device
    if lm.uni_tok.device != dev or ctx.device != dev:
        raise _lib.EamdError("ngram_score_pairs: tables, contexts and tokens on one device")
    lp = torch.empty(n, device=dev, dtype=torch.float32)
    ctx_new = torch.empty(n, Cw, device=dev, dtype=torch.int32)
    check(_lib.lib().eamd_ngram_score_pairs(*_ngram_query_args(lm), V, lm.order, lm.unk, ptr(ctx) if Cw else None, ptr(tok), ptr(lp),
                                            ptr(ctx_new) if Cw else None, n, stream_ptr()), "eamd_ngram_score_pairs")
    return lp, ctx_new


CTC_BEAM_MAX_W, CTC_BEAM_MAX_K, CTC_BEAM_MAX_T = 32, 32, 2048      # csrc/ctc_beam.hip


def ctc_beam_candidates(logp, cand_size):
    """the per-frame candidates of the CTC prefix beam search for all B T rows at once: eamd_topk_rows_i32 on columns 1 .. V-2 of
    logp [B, T, V] (contiguous fp32) -> (values [B T, K] fp32, ids [B T, K] int32 counted from column 1)"""
    B, T, V = logp.shape
    if logp.dtype != torch.float32 or not logp.is_contiguous():
        raise _lib.EamdError("ctc_prefix_beam: contiguous float32 [B, T, V]")
    K = int(cand_size)
    if not 1 <= K <= min(CTC_BEAM_MAX_K, V - 2):
        raise _lib.EamdError("ctc_prefix_beam: 1 <= candidates <= min(%d, V - 2)" % CTC_BEAM_MAX_K)
    rows = B * T
    cval = torch.empty(rows, K, device=logp.device, dtype=torch.float32)
    cidx = torch.empty(rows, K, device=logp.device, dtype=torch.int64)
    cid = torch.empty(rows, K, device=logp.device, dtype=torch.int32)
    check(_lib.lib().eamd_topk_rows_i32(ptr(logp, 1), V, rows, V - 2, K, ptr(cval), ptr(cidx), ptr(cid), stream_ptr()),
          "eamd_topk_rows_i32")
    return cval, cid


def ctc_prefix_beam_search(logp, cval, cid, hlens, beam_size, nbest, penalty=0.0, lm=None, ngram_weight=0.0, ws=None, out=None):
    """eamd_ctc_prefix_beam alone (one launch, one workgroup per utterance) on the candidates of ctc_beam_candidates; ws / out:
    the workspace and result buffer of an earlier call with the same shapes, else allocated here -> (out, ws)"""
    B, T, V = logp.shape
    K = cval.shape[1]
    assert hlens.dtype == torch.int32 and hlens.numel() == B and hlens.is_contiguous() and hlens.device == logp.device
    assert cval.shape == (B * T, K) and cid.shape == (B * T, K) and cid.dtype == torch.int32
    W = int(beam_size)
    if not (1 <= nbest <= W <= CTC_BEAM_MAX_W and T <= CTC_BEAM_MAX_T):
        raise _lib.EamdError("ctc_prefix_beam: 1 <= nbest <= beam <= %d, T <= %d" % (CTC_BEAM_MAX_W, CTC_BEAM_MAX_T))
    dev = logp.device
    ws_bytes = _lib.lib().eamd_ctc_beam_workspace_bytes(B, T, W)
    if ws is None:
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    if out is None:
        out = torch.empty(B, nbest, 2 + T, device=dev, dtype=torch.int32)
    assert ws.numel() >= ws_bytes and out.shape == (B, nbest, 2 + T) and out.dtype == torch.int32 and out.is_contiguous()
    if lm is not None:
        if lm.uni_tok.device != dev or lm.uni_tok.numel() != V:
            raise _lib.EamdError("ctc_prefix_beam: the n-gram tables on the device of logp, over the same %d tokens" % V)
        tables, order, bos, unk = _ngram_query_args(lm), lm.order, lm.bos, lm.unk
    else:
        tables, order, bos, unk = (None,) * 9 + (0,), 0, 0, 0
    check(_lib.lib().eamd_ctc_prefix_beam(ptr(logp), V, ptr(cval), ptr(cid), ptr(hlens), B, T, V, W, K, int(nbest),
                                          penalty, *tables, order, bos, unk, ngram_weight, ptr(ws),
                                          ws.numel(), ptr(out), stream_ptr()), "eamd_ctc_prefix_beam")
    return out, ws


def ctc_prefix_beam(logp, hlens, beam_size, cand_size, nbest, penalty=0.0, lm=None, ngram_weight=0.0):
    """time-synchronous CTC prefix beam search of a padded batch: ctc_beam_candidates, then ctc_prefix_beam_search.  logp [B, T, V]
    contiguous fp32 log-softmax rows, hlens [B] int32 on the device, lm: nets.ngram.ArpaLM on the device or None
    -> int32 [B, nbest, 2 + T] on the device: the bits of the fp32 score, the length (-1: no hypothesis), the tokens"""
    cval, cid = ctc_beam_candidates(logp, cand_size)
    return ctc_prefix_beam_search(logp, cval, cid, hlens, beam_size, nbest, penalty, lm, ngram_weight)[0]


# ---- second-pass n-best rescoring (csrc/rescore.hip) -----------------------------------------------
def _nbest_dims(nbest):
    if not (nbest.is_cuda and nbest.dtype == torch.int32 and nbest.dim() == 3 and nbest.is_contiguous() and nbest.shape[2] > 2):
        raise _lib.EamdError("n-best: contiguous int32 [B, N, 2 + T] on the device")
    B, N, W = nbest.shape
    if not (1 <= N <= CTC_BEAM_MAX_W and W - 2 <= CTC_BEAM_MAX_T):
        raise _lib.EamdError("n-best: 1 <= N <= %d, T <= %d" % (CTC_BEAM_MAX_W, CTC_BEAM_MAX_T))
    return B, N, W - 2


def nbest_pack(nbest, U, V, sos, eos):
    """eamd_nbest_pack: the packed n-best [B, N, 2 + T] of ctc_prefix_beam -> (ys_in [B*N, U] int64, col [B*N*U] int32,
    ulen [B*N] int32), the teacher-forcing operands over U positions (U = the longest length + 1, from the caller)"""
    B, N, T = _nbest_dims(nbest)
    U = int(U)
    if not (1 <= U <= T + 1 and 0 <= sos < V and 0 <= eos < V):
        raise _lib.EamdError("nbest_pack: 1 <= U <= T + 1 and sos, eos in [0, V)")
    dev = nbest.device
    ys_in = torch.empty(B * N, U, device=dev, dtype=torch.int64)
    col = torch.empty(B * N * U, device=dev, dtype=torch.int32)
    ulen = torch.empty(B * N, device=dev, dtype=torch.int32)
    check(_lib.lib().eamd_nbest_pack(ptr(nbest), B, N, T, U, int(V), int(sos), int(eos), ptr(ys_in), ptr(col), ptr(ulen),
                                     stream_ptr()), "eamd_nbest_pack")
    return ys_in, col, ulen


def row_target_stats(hidden, W, bias, col, tile=None):
    """what log p(col[m] | row m) of softmax(hidden W^T + bias) needs, without the [rows, V] logits: eamd_gemm with the
    row-statistics epilogue (epilogue 7) -> (part [rows, tiles_n, 2], zcol [rows], tiles_n).  hidden [rows, D] and W [V, D]
    of one operand dtype, col [rows] int32 (-1: no target, zcol[m] is then not written).  No fall-back: a shape the GEMM
    declines is an error.  tile: the GEMM's column tile, 64 or 128 (default: 128 from 2048 rows on, as the transducer loss)."""
    rows, D = hidden.shape
    V = W.shape[0]
    if not (hidden.is_contiguous() and W.is_contiguous() and W.shape[1] == D and col.dtype == torch.int32 and col.numel() == rows):
        raise _lib.EamdError("row_target_stats: contiguous hidden [rows, D], W [V, D] and int32 col [rows]")
    tile = (128 if rows >= 2048 else 64) if tile is None else int(tile)
    tn = (V + tile - 1) // tile
    dev = hidden.device
    part = torch.empty(rows, tn, 2, device=dev, dtype=torch.float32)
    zcol = torch.zeros(rows, device=dev, dtype=torch.float32)
    zfix = torch.empty(rows, device=dev, dtype=torch.float32)
    gemm(hidden, W, None, rows, V, D, D, D, V, bias=bias, epilogue=EPI_ROW_STATS, tile=tile, stats=(part, col, zcol, zfix, 0))
    return part, zcol, tn


def nbest_rescore(nbest, ulen, U, scorers, w0):
    """eamd_nbest_rescore: scorers = 1 or 2 of (part, zcol, tiles_n, weight) from row_target_stats over the B*N*U rows of
    nbest_pack -> (nbest_out [B, N, 2 + T] re-ranked with word 0 = the bits of f = w0 * s1 + sum_s weight_s * term_s,
    terms [B, N, 1 + S] fp32 = (s1, term_1 ..) and order [B, N] int32 = the first-pass index, all in the new order)"""
    B, N, T = _nbest_dims(nbest)
    S, rows = len(scorers), B * N * int(U)
    if S not in (1, 2) or not 1 <= U <= T + 1:
        raise _lib.EamdError("nbest_rescore: one or two scorers, 1 <= U <= T + 1")
    if not (ulen.dtype == torch.int32 and ulen.numel() == B * N and ulen.is_contiguous() and ulen.device == nbest.device):
        raise _lib.EamdError("nbest_rescore: ulen int32 [B * N] beside the n-best")
    args = []
    for part, zcol, tn, w in scorers:
        if not (part.dtype == torch.float32 and zcol.dtype == torch.float32 and part.is_contiguous() and zcol.is_contiguous()
                and tn >= 1 and part.numel() >= rows * tn * 2 and zcol.numel() >= rows and part.device == nbest.device
                and zcol.device == nbest.device):
            raise _lib.EamdError("nbest_rescore: part [B*N*U, tiles_n, 2] and zcol [B*N*U] float32 beside the n-best")
        args += [ptr(part), ptr(zcol), int(tn), float(w)]
    if S == 1:
        args += [None, None, 0, 0.0]
    dev = nbest.device
    out = torch.empty_like(nbest)
    terms = torch.empty(B, N, 1 + S, device=dev, dtype=torch.float32)
    order = torch.empty(B, N, device=dev, dtype=torch.int32)
    check(_lib.lib().eamd_nbest_rescore(ptr(nbest), ptr(ulen), B, N, T, int(U), S, *args, float(w0), ptr(out), ptr(terms),
                                        ptr(order), stream_ptr()), "eamd_nbest_rescore")
    return out, terms, order


# ---- MVDR beamforming front-end (csrc/beamformer.hip) ----------------------------------------------
BF_PSD, BF_PSD_BWD, BF_MVDR_BWD, BF_APPLY_BWD = 0, 1, 2, 3
BF_TCHUNK = 64               # EAMD_BF_TCHUNK: frames per workgroup of the kernels that split the time axis


def _bf_f32(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.EamdError("beamformer kernels take contiguous float32 tensors, complex as a trailing (re, im) axis")


def _bf_workspace(op, S, B, T, Cn, F, device):
    n = _lib.lib().eamd_bf_workspace_bytes(op, S, B, T, Cn, F)
    if n < 0:
        raise _lib.EamdError(f"eamd_bf_workspace_bytes refused S={S} B={B} T={T} C={Cn} F={F} (2 <= C <= 8)")
    return torch.empty(n // 4, device=device, dtype=torch.float32)


def bf_psd(x, z, out=None):
    """x [B,T,C,F,2], mask logits z [S,B,C,Tm,F] -> (psd [S,B,F,C,C,2], feat [B,C,F], nrm [S,B,F]); out: the same triple to
    write into (eamd_bf_psd)"""
    B, T, Cn, F, two = x.shape
    S, Tm = z.shape[0], z.shape[3]
    assert two == 2 and z.shape == (S, B, Cn, Tm, F) and Tm <= T
    _bf_f32(x, z)
    if out is None:
        out = (torch.empty(S, B, F, Cn, Cn, 2, device=x.device, dtype=torch.float32), torch.empty(B, Cn, F, device=x.device, dtype=torch.float32),
               torch.empty(S, B, F, device=x.device, dtype=torch.float32))
    psd, feat, nrm = out
    assert psd.shape == (S, B, F, Cn, Cn, 2) and feat.shape == (B, Cn, F) and nrm.shape == (S, B, F)
    _bf_f32(psd, feat, nrm)
    ws = _bf_workspace(BF_PSD, S, B, Tm, Cn, F, x.device)
    check(_lib.lib().eamd_bf_psd(ptr(x), ptr(z), ptr(psd), ptr(feat), ptr(nrm), ptr(ws), S, B, T, Tm, Cn, F, stream_ptr()),
          "eamd_bf_psd")
    return psd, feat, nrm


def bf_psd_bwd(x, z, psd, nrm, gpsd, gfeat, out=None):
    """-> dz [S,B,C,Tm,F] (eamd_bf_psd_bwd); gpsd / gfeat: None = zero"""
    B, T, Cn, F, _ = x.shape
    S, Tm = z.shape[0], z.shape[3]
    assert psd.shape == (S, B, F, Cn, Cn, 2) and nrm.shape == (S, B, F)
    assert gpsd is None or gpsd.shape == psd.shape
    assert gfeat is None or gfeat.shape == (B, Cn, F)
    _bf_f32(x, z, psd, nrm, gpsd, gfeat)
    dz = torch.empty_like(z) if out is None else out
    assert dz.shape == z.shape
    _bf_f32(dz)
    ws = _bf_workspace(BF_PSD_BWD, S, B, Tm, Cn, F, x.device)
    check(_lib.lib().eamd_bf_psd_bwd(ptr(x), ptr(z), ptr(psd), ptr(nrm), ptr(gpsd), ptr(gfeat), ptr(dz), ptr(ws), S, B, T, Tm,
                                     Cn, F, stream_ptr()), "eamd_bf_psd_bwd")
    return dz


def bf_mvdr(psd_s, psd_n, u, out=None):
    """psd_s, psd_n [B,F,C,C,2], u [B,C] -> w [B,F,C,2] (eamd_bf_mvdr)"""
    B, F, Cn = psd_s.shape[:3]
    assert psd_s.shape == (B, F, Cn, Cn, 2) and psd_n.shape == psd_s.shape and u.shape == (B, Cn)
    _bf_f32(psd_s, psd_n, u)
    w = torch.empty(B, F, Cn, 2, device=psd_s.device, dtype=torch.float32) if out is None else out
    assert w.shape == (B, F, Cn, 2)
    _bf_f32(w)
    check(_lib.lib().eamd_bf_mvdr(ptr(psd_s), ptr(psd_n), ptr(u), ptr(w), B, F, Cn, stream_ptr()), "eamd_bf_mvdr")
    return w


def bf_mvdr_bwd(psd_s, psd_n, u, gw, out=None):
    """-> (gpsd_s, gpsd_n [B,F,C,C,2], gu [B,C]) (eamd_bf_mvdr_bwd)"""
    B, F, Cn = psd_s.shape[:3]
    assert psd_n.shape == psd_s.shape and u.shape == (B, Cn) and gw.shape == (B, F, Cn, 2)
    _bf_f32(psd_s, psd_n, u, gw)
    gs, gn, gu = (torch.empty_like(psd_s), torch.empty_like(psd_n), torch.empty_like(u)) if out is None else out
    assert gs.shape == psd_s.shape and gn.shape == psd_s.shape and gu.shape == u.shape
    _bf_f32(gs, gn, gu)
    ws = _bf_workspace(BF_MVDR_BWD, 1, B, 1, Cn, F, u.device)
    check(_lib.lib().eamd_bf_mvdr_bwd(ptr(psd_s), ptr(psd_n), ptr(u), ptr(gw), ptr(gs), ptr(gn), ptr(gu), ptr(ws), B, F, Cn,
                                      stream_ptr()), "eamd_bf_mvdr_bwd")
    return gs, gn, gu


def bf_apply(w, x, out=None):
    """w [B,F,C,2], x [B,T,C,F,2] -> y [B,T,F,2] = sum_c conj(w) x (eamd_bf_apply)"""
    B, T, Cn, F, _ = x.shape
    assert w.shape == (B, F, Cn, 2)
    _bf_f32(w, x)
    y = torch.empty(B, T, F, 2, device=x.device, dtype=torch.float32) if out is None else out
    assert y.shape == (B, T, F, 2)
    _bf_f32(y)
    check(_lib.lib().eamd_bf_apply(ptr(w), ptr(x), ptr(y), B, T, Cn, F, stream_ptr()), "eamd_bf_apply")
    return y


def bf_apply_bwd(gy, x, out=None):
    """gy [B,T,F,2], x [B,T,C,F,2] -> gw [B,F,C,2] (eamd_bf_apply_bwd)"""
    B, T, Cn, F, _ = x.shape
    assert gy.shape == (B, T, F, 2)
    _bf_f32(gy, x)
    gw = torch.empty(B, F, Cn, 2, device=x.device, dtype=torch.float32) if out is None else out
    assert gw.shape == (B, F, Cn, 2)
    _bf_f32(gw)
    ws = _bf_workspace(BF_APPLY_BWD, 1, B, T, Cn, F, x.device)
    check(_lib.lib().eamd_bf_apply_bwd(ptr(gy), ptr(x), ptr(gw), ptr(ws), B, T, Cn, F, stream_ptr()), "eamd_bf_apply_bwd")
    return gw


# ---- WPE dereverberation (csrc/wpe.hip) ------------------------------------------------------------
WPE_FTILE = 32               # EAMD_WPE_FTILE: frequency bins per workgroup of the correlation and filter kernels
WPE_MAX_UNKNOWNS = 64        # EAMD_WPE_MAX_UNKNOWNS: C * taps
_WPE_TASKS = 8               # 4 x 4 tiles of [R | P] per correlation workgroup (csrc/wpe.hip: kSlots)


def wpe_check_shape(Cn, taps, delay):
    """the limits of csrc/wpe.hip, refused here by name before anything is launched"""
    if taps < 1 or Cn < 1:
        raise ValueError(f"WPE needs taps >= 1 and at least one channel (taps={taps}, C={Cn})")
    if delay < 0:
        raise ValueError(f"WPE needs delay >= 0 (delay={delay})")
    if Cn * taps > WPE_MAX_UNKNOWNS:
        raise ValueError(f"WPE kernels solve at most C * taps = {WPE_MAX_UNKNOWNS} unknowns per bin (C={Cn}, taps={taps})")


def wpe_nchunk(B, T, Cn, F, taps, backward=False):
    """into how many chunks the correlation pass cuts the time axis: enough workgroups to fill the chip, chunks of at
    least 64 frames, a workspace of at most 1 GiB.  A function of the shape alone, so a launch repeats bit for bit."""
    N = Cn * taps
    nt, pt = -(-N // 4), -(-Cn // 4)
    tasks = nt * pt if backward else nt * (nt + 1) // 2 + nt * pt
    base = -(-F // WPE_FTILE) * -(-tasks // _WPE_TASKS) * B
    n = max(1, min(-(-1024 // base), -(-T // 64)))
    per = B * F * N * (Cn if backward else N + Cn) * 16
    return max(1, min(n, (1 << 30) // per))


def _wpe_lens(lens, B, device):
    if lens is not None:
        assert lens.shape == (B,) and lens.dtype == torch.int32 and lens.device == device and lens.is_contiguous()
    return lens


def wpe_power(y, z=None, out=None):
    """y [B,T,C,F,2], mask logits z [1,B,C,Tm,F] or None -> power [B,T,F] = mean_c |y|^2 sigmoid(z) (eamd_wpe_power)"""
    B, T, Cn, F, two = y.shape
    Tm = T if z is None else z.shape[3]
    assert two == 2 and (z is None or (z.shape == (1, B, Cn, Tm, F) and Tm <= T))
    _bf_f32(y, z)
    power = torch.empty(B, T, F, device=y.device, dtype=torch.float32) if out is None else out
    assert power.shape == (B, T, F)
    _bf_f32(power)
    check(_lib.lib().eamd_wpe_power(ptr(y), ptr(z), ptr(power), B, T, Tm, Cn, F, stream_ptr()), "eamd_wpe_power")
    return power


def wpe_power_bwd(y, z, gpower, out=None):
    """-> dz [1,B,C,Tm,F] (eamd_wpe_power_bwd)"""
    B, T, Cn, F, _ = y.shape
    Tm = z.shape[3]
    assert z.shape == (1, B, Cn, Tm, F) and Tm <= T and gpower.shape == (B, T, F)
    _bf_f32(y, z, gpower)
    dz = torch.empty_like(z) if out is None else out
    assert dz.shape == z.shape
    _bf_f32(dz)
    check(_lib.lib().eamd_wpe_power_bwd(ptr(y), ptr(z), ptr(gpower), ptr(dz), B, T, Tm, Cn, F, stream_ptr()),
          "eamd_wpe_power_bwd")
    return dz


def wpe_taps(y, power, lens, taps, delay, eps=1e-10, inverse_power=True, keep_factor=True, nchunk=None, out=None):
    """y [B,T,C,F,2], power [B,T,F], lens [B] int32 on the device or None -> (G [B,N,C,F,2], fac [B,F,N,N,2] float64 or None):
    the prediction filter, row i = k * C + c of the stacked history, and the factor the backward takes (eamd_wpe_taps)"""
    B, T, Cn, F, two = y.shape
    wpe_check_shape(Cn, taps, delay)
    N = Cn * taps
    assert two == 2 and power.shape == (B, T, F)
    _bf_f32(y, power)
    lens = _wpe_lens(lens, B, y.device)
    nchunk = wpe_nchunk(B, T, Cn, F, taps) if nchunk is None else nchunk
    if out is None:
        out = (torch.empty(B, N, Cn, F, 2, device=y.device, dtype=torch.float32),
               torch.empty(B, F, N, N, 2, device=y.device, dtype=torch.float64) if keep_factor else None)
    G, fac = out
    assert G.shape == (B, N, Cn, F, 2) and (fac is None or (fac.shape == (B, F, N, N, 2) and fac.dtype == torch.float64
                                                             and fac.is_contiguous()))
    _bf_f32(G)
    ws = torch.empty(nchunk * B * F * N * (N + Cn) * 2, device=y.device, dtype=torch.float64)
    check(_lib.lib().eamd_wpe_taps(ptr(y), ptr(power), ptr(lens), ptr(G), ptr(fac), ptr(ws), B, T, Cn, F, taps, delay, eps,
                                   int(bool(inverse_power)), nchunk, stream_ptr()), "eamd_wpe_taps")
    return G, fac


def wpe_filter(y, G, lens, taps, delay, out=None):
    """-> x [B,T,C,F,2] = y - G^H (stacked history), exactly 0 past each length (eamd_wpe_filter)"""
    B, T, Cn, F, _ = y.shape
    wpe_check_shape(Cn, taps, delay)
    assert G.shape == (B, Cn * taps, Cn, F, 2)
    _bf_f32(y, G)
    lens = _wpe_lens(lens, B, y.device)
    x = torch.empty_like(y) if out is None else out
    assert x.shape == y.shape
    _bf_f32(x)
    check(_lib.lib().eamd_wpe_filter(ptr(y), ptr(G), ptr(lens), ptr(x), B, T, Cn, F, taps, delay, stream_ptr()),
          "eamd_wpe_filter")
    return x


def wpe_bwd(y, x, gx, power, lens, fac, taps, delay, eps=1e-10, inverse_power=True, nchunk=None, out=None):
    """gx [B,T,C,F,2], the cotangent of x -> gpower [B,T,F] (eamd_wpe_bwd); x, power, fac as the forward took / wrote them"""
    B, T, Cn, F, _ = y.shape
    wpe_check_shape(Cn, taps, delay)
    N = Cn * taps
    assert x.shape == y.shape and gx.shape == y.shape and power.shape == (B, T, F)
    assert fac.shape == (B, F, N, N, 2) and fac.dtype == torch.float64 and fac.is_contiguous()
    _bf_f32(y, x, gx, power)
    lens = _wpe_lens(lens, B, y.device)
    nchunk = wpe_nchunk(B, T, Cn, F, taps, backward=True) if nchunk is None else nchunk
    gpower = torch.empty_like(power) if out is None else out
    assert gpower.shape == power.shape
    _bf_f32(gpower)
    ws = torch.empty((2 * nchunk + 1) * B * F * N * Cn, device=y.device, dtype=torch.float64)
    check(_lib.lib().eamd_wpe_bwd(ptr(y), ptr(x), ptr(gx), ptr(power), ptr(lens), ptr(fac), ptr(gpower), ptr(ws), B, T, Cn, F,
                                  taps, delay, eps, int(bool(inverse_power)), nchunk, stream_ptr()), "eamd_wpe_bwd")
    return gpower


# ---- WPD / MPDR convolutional beamformers (csrc/wpd.hip) -------------------------------------------
def wpd_check_shape(Cn, btaps, bdelay):
    """the limits of csrc/wpd.hip, refused here by name before anything is launched"""
    if btaps < 0 or Cn < 1:
        raise ValueError(f"WPD needs btaps >= 0 and at least one channel (btaps={btaps}, C={Cn})")
    if bdelay < 1:
        raise ValueError(f"WPD needs bdelay >= 1 (bdelay={bdelay})")
    if Cn * (btaps + 1) > WPE_MAX_UNKNOWNS:
        raise ValueError(f"WPD kernels solve at most (btaps + 1) * C = {WPE_MAX_UNKNOWNS} unknowns per bin (C={Cn}, "
                         f"btaps={btaps})")


def wpd_nchunk(B, T, Cn, F, btaps, backward=False):
    """into how many chunks the covariance pass (backward: the pass that forms gh) cuts the time axis; the rule of
    wpe_nchunk.  A function of the shape alone, so a launch repeats bit for bit."""
    N = Cn * (btaps + 1)
    nt = -(-N // 4)
    groups = -(-N // 8) if backward else -(-(nt * (nt + 1) // 2) // _WPE_TASKS)
    base = -(-F // WPE_FTILE) * groups * B
    n = max(1, min(-(-1024 // base), -(-T // 64)))
    per = B * F * N * (1 if backward else N) * 16
    return max(1, min(n, (1 << 30) // per))


def _wpd_f64(t, shape):
    assert t.shape == shape and t.dtype == torch.float64 and t.is_contiguous(), (tuple(t.shape), t.dtype, shape)


def wpd_cov(y, power, lens, btaps, bdelay, eps=1e-10, inverse_power=True, nchunk=None, out=None):
    """y [B,T,C,F,2], power [B,T,F] or None (unit weights), lens [B] int32 on the device or None -> Rf [B,F,N,N,2] float64,
    N = (btaps + 1) C: the weighted covariance of the stacked frames, exactly Hermitian (eamd_wpd_cov)"""
    B, T, Cn, F, two = y.shape
    wpd_check_shape(Cn, btaps, bdelay)
    N = Cn * (btaps + 1)
    assert two == 2 and (power is None or power.shape == (B, T, F))
    _bf_f32(y, power)
    lens = _wpe_lens(lens, B, y.device)
    nchunk = wpd_nchunk(B, T, Cn, F, btaps) if nchunk is None else nchunk
    Rf = torch.empty(B, F, N, N, 2, device=y.device, dtype=torch.float64) if out is None else out
    _wpd_f64(Rf, (B, F, N, N, 2))
    ws = torch.empty(nchunk * B * F * N * N * 2, device=y.device, dtype=torch.float64)
    check(_lib.lib().eamd_wpd_cov(ptr(y), ptr(power), ptr(lens), ptr(Rf), ptr(ws), B, T, Cn, F, btaps, bdelay, eps,
                                  int(bool(inverse_power)), nchunk, stream_ptr()), "eamd_wpd_cov")
    return Rf


def wpd_cov_bwd(y, gRf, power, lens, btaps, bdelay, eps=1e-10, inverse_power=True, out=None):
    """gRf [B,F,N,N,2] float64, the cotangent of Rf -> gpower [B,T,F] (eamd_wpd_cov_bwd)"""
    B, T, Cn, F, _ = y.shape
    wpd_check_shape(Cn, btaps, bdelay)
    N = Cn * (btaps + 1)
    assert power.shape == (B, T, F)
    _wpd_f64(gRf, (B, F, N, N, 2))
    _bf_f32(y, power)
    lens = _wpe_lens(lens, B, y.device)
    gpower = torch.empty_like(power) if out is None else out
    assert gpower.shape == power.shape
    _bf_f32(gpower)
    ws = torch.empty(B * F * N * N * 2, device=y.device, dtype=torch.float64)
    check(_lib.lib().eamd_wpd_cov_bwd(ptr(y), ptr(gRf), ptr(power), ptr(lens), ptr(gpower), ptr(ws), B, T, Cn, F, btaps, bdelay,
                                      eps, int(bool(inverse_power)), stream_ptr()), "eamd_wpd_cov_bwd")
    return gpower


def wpd_vector(Rf, phi, u, keep=True, out=None):
    """Rf [B,F,N,N,2] float64, phi [B,F,C,C,2], u [B,C] -> (h [B,F,N,2], fac [B,F,N,N,2], xkeep [B,F,N,C,2]); fac and xkeep,
    float64, are what wpd_vector_bwd takes (None unless keep) (eamd_wpd_vector)"""
    B, F, N = Rf.shape[:3]
    Cn = u.shape[1]
    assert N % Cn == 0 and phi.shape == (B, F, Cn, Cn, 2) and u.shape == (B, Cn)
    btaps = N // Cn - 1
    wpd_check_shape(Cn, btaps, 1)
    _wpd_f64(Rf, (B, F, N, N, 2))
    _bf_f32(phi, u)
    if out is None:
        out = (torch.empty(B, F, N, 2, device=Rf.device, dtype=torch.float32),
               torch.empty(B, F, N, N, 2, device=Rf.device, dtype=torch.float64) if keep else None,
               torch.empty(B, F, N, Cn, 2, device=Rf.device, dtype=torch.float64) if keep else None)
    h, fac, xk = out
    assert h.shape == (B, F, N, 2)
    _bf_f32(h)
    if fac is not None:
        _wpd_f64(fac, (B, F, N, N, 2))
    if xk is not None:
        _wpd_f64(xk, (B, F, N, Cn, 2))
    check(_lib.lib().eamd_wpd_vector(ptr(Rf), ptr(phi), ptr(u), ptr(h), ptr(fac), ptr(xk), B, F, Cn, btaps, stream_ptr()),
          "eamd_wpd_vector")
    return h, fac, xk


def wpd_vector_bwd(fac, xk, phi, u, gh, out=None):
    """gh [B,F,N,2] -> (gphi [B,F,C,C,2], gu [B,C], gRf [B,F,N,N,2] float64) (eamd_wpd_vector_bwd)"""
    B, F, N = fac.shape[:3]
    Cn = u.shape[1]
    btaps = N // Cn - 1
    _wpd_f64(fac, (B, F, N, N, 2))
    _wpd_f64(xk, (B, F, N, Cn, 2))
    assert phi.shape == (B, F, Cn, Cn, 2) and u.shape == (B, Cn) and gh.shape == (B, F, N, 2)
    _bf_f32(phi, u, gh)
    if out is None:
        out = (torch.empty_like(phi), torch.empty_like(u), torch.empty_like(fac))
    gphi, gu, gRf = out
    assert gphi.shape == phi.shape and gu.shape == u.shape
    _bf_f32(gphi, gu)
    _wpd_f64(gRf, (B, F, N, N, 2))
    ws = torch.empty(B * F * Cn, device=fac.device, dtype=torch.float64)
    check(_lib.lib().eamd_wpd_vector_bwd(ptr(fac), ptr(xk), ptr(phi), ptr(u), ptr(gh), ptr(gphi), ptr(gu), ptr(gRf), ptr(ws), B,
                                         F, Cn, btaps, stream_ptr()), "eamd_wpd_vector_bwd")
    return gphi, gu, gRf


def wpd_apply(h, y, lens, btaps, bdelay, out=None):
    """h [B,F,N,2], y [B,T,C,F,2] -> e [B,T,F,2] = h^H (stacked frames), exactly 0 past each length (eamd_wpd_apply)"""
    B, T, Cn, F, _ = y.shape
    wpd_check_shape(Cn, btaps, bdelay)
    N = Cn * (btaps + 1)
    assert h.shape == (B, F, N, 2)
    _bf_f32(h, y)
    lens = _wpe_lens(lens, B, y.device)
    e = torch.empty(B, T, F, 2, device=y.device, dtype=torch.float32) if out is None else out
    assert e.shape == (B, T, F, 2)
    _bf_f32(e)
    ws = torch.empty(B * N * F * 2, device=y.device, dtype=torch.float32)
    check(_lib.lib().eamd_wpd_apply(ptr(h), ptr(y), ptr(lens), ptr(e), ptr(ws), B, T, Cn, F, btaps, bdelay, stream_ptr()),
          "eamd_wpd_apply")
    return e


def wpd_apply_bwd(ge, y, lens, btaps, bdelay, nchunk=None, out=None):
    """ge [B,T,F,2], the cotangent of e -> gh [B,F,N,2] (eamd_wpd_apply_bwd)"""
    B, T, Cn, F, _ = y.shape
    wpd_check_shape(Cn, btaps, bdelay)
    N = Cn * (btaps + 1)
    assert ge.shape == (B, T, F, 2)
    _bf_f32(ge, y)
    lens = _wpe_lens(lens, B, y.device)
    nchunk = wpd_nchunk(B, T, Cn, F, btaps, backward=True) if nchunk is None else nchunk
    gh = torch.empty(B, F, N, 2, device=y.device, dtype=torch.float32) if out is None else out
    assert gh.shape == (B, F, N, 2)
    _bf_f32(gh)
    ws = torch.empty(nchunk * B * F * N * 2, device=y.device, dtype=torch.float64)
    check(_lib.lib().eamd_wpd_apply_bwd(ptr(ge), ptr(y), ptr(lens), ptr(gh), ptr(ws), B, T, Cn, F, btaps, bdelay, nchunk,
                                        stream_ptr()), "eamd_wpd_apply_bwd")
    return gh


# ---- CTC -----------------------------------------------------------------------------------------
def ctc_loss(acts_btv, ys_pad, ilens, blank=0, ignore_id=-1, grad_scale=1.0, want_grad=True, time_major=False,
             keep_workspace=False):
    """acts [B,T,V] raw activations (time_major: [T,B,V], warp-ctc's layout - read in place through the entry point's
    (stride_t, stride_b), the gradient comes back in the same layout); ys_pad [B,L] int64; ilens [B] int32 -> nll [B], grad.
    keep_workspace: -> nll, grad, workspace (what ctc_grad needs to run the gradient pass later)"""
    if time_major:
        T, B, V = acts_btv.shape
        st, sb = B * V, V
    else:
        B, T, V = acts_btv.shape
        st, sb = V, T * V
    L = ys_pad.shape[1]
    assert acts_btv.is_contiguous() and ys_pad.is_contiguous() and ys_pad.dtype == torch.int64
    assert ilens.dtype == torch.int32 and ilens.numel() == B and ys_pad.shape[0] == B
    ws_bytes = _lib.lib().eamd_ctc_workspace_bytes(B, T, L)
    ws = torch.empty(ws_bytes, device=acts_btv.device, dtype=torch.uint8)
    nll = torch.empty(B, device=acts_btv.device, dtype=torch.float32)
    grad = torch.empty_like(acts_btv) if want_grad else None
    check(_lib.lib().eamd_ctc_loss(ptr(acts_btv), st, sb, ptr(ys_pad), ptr(ilens), ptr(nll),
                                   ptr(grad), st, sb, ptr(ws), B, T, V, L, blank, ignore_id,
                                   grad_scale, stream_ptr()), "eamd_ctc_loss")
    if keep_workspace:
        return nll, grad, ws
    return nll, grad


def ctc_grad(acts_btv, ilens, nll, ws, L, blank=0, grad_scale=1.0, gscale=None, time_major=False):
    """the gradient pass of ctc_loss alone, on the workspace `ws` and `nll` that ctc_loss(..., want_grad=False,
    keep_workspace=True) returned for the same acts / ilens and labels of padded length L.  gscale: optional float32 device
    scalar, multiplied in last: the result equals scale_dev(ctc_loss(...)[1], gscale), from one pass"""
    if time_major:
        T, B, V = acts_btv.shape
        st, sb = B * V, V
    else:
        B, T, V = acts_btv.shape
        st, sb = V, T * V
    L_ = _lib.lib()
    assert acts_btv.is_contiguous() and acts_btv.dtype == torch.float32 and ilens.dtype == torch.int32 and ilens.numel() == B
    assert nll.dtype == torch.float32 and nll.numel() == B and ws.numel() >= L_.eamd_ctc_workspace_bytes(B, T, L)
    assert gscale is None or (gscale.dtype == torch.float32 and gscale.numel() == 1)
    grad = torch.empty_like(acts_btv)
    check(L_.eamd_ctc_grad(ptr(acts_btv), st, sb, ptr(ilens), ptr(nll), ptr(grad), st, sb, ptr(ws), B, T, V, L, blank,
                           grad_scale, ptr(gscale), stream_ptr()), "eamd_ctc_grad")
    return grad


def ctc_pit_loss(acts, ys_pad, ilens, blank=0, ignore_id=-1, grad_scale=1.0, want_grad=True):
    """permutation-invariant CTC of S = 2 or 3 speakers (eamd_ctc_pit_loss): acts [S,B,T,V] raw activations, ys_pad [B,S,L] int64
    padded with ignore_id, ilens [B] int32 -> nll_pair [B,S,S] (-log p of hypothesis i against reference j), perm [B,S] int64
    (the reference assigned to hypothesis i), pit [B] (the chosen permutation's score, (sum_i nll_pair[b,i,perm]/B)/S), grad
    [S,B,T,V] = grad_scale * d(sum_b sum_i nll_pair[b,i,perm[b,i]])/d acts (None unless want_grad).  No host synchronisation."""
    S, B, T, V = acts.shape
    L = ys_pad.shape[2]
    assert acts.is_contiguous() and acts.dtype == torch.float32
    assert ys_pad.is_contiguous() and ys_pad.dtype == torch.int64 and tuple(ys_pad.shape[:2]) == (B, S)
    assert ilens.dtype == torch.int32 and ilens.numel() == B
    dev = acts.device
    ws = torch.empty(_lib.lib().eamd_ctc_pit_workspace_bytes(S, B, T, L), device=dev, dtype=torch.uint8)
    nll = torch.empty(B, S, S, device=dev, dtype=torch.float32)
    perm = torch.empty(B, S, device=dev, dtype=torch.int64)
    pit = torch.empty(B, device=dev, dtype=torch.float32)
    grad = torch.empty_like(acts) if want_grad else None
    check(_lib.lib().eamd_ctc_pit_loss(ptr(acts), ptr(ys_pad), ptr(ilens), ptr(nll), ptr(perm), ptr(pit), ptr(grad), ptr(ws), S, B,
                                       T, V, L, blank, ignore_id, grad_scale, stream_ptr()), "eamd_ctc_pit_loss")
    return nll, perm, pit, grad


def ctc_forced_align(acts, ilens, ys_pad, blank=0, ignore_id=-1, normalized=False, time_major=False):
    """best CTC path of each utterance (eamd_ctc_forced_align): acts [B,T,V] raw activations, or log-probabilities when
    normalized (time_major: [T,B,V]); ilens [B] int32; ys_pad [B,L] int64 padded with ignore_id
    -> score [B] f32, states [B,T] int32, tokens [B,T] int64, seg_start / seg_end [B,L] int32 (device tensors; -1 past
    ilens / the labels and for utterances without a path, whose score is -inf - also those with a label outside [0, V),
    which the kernel never reads).  L <= 2047."""
    if time_major:
        T, B, V = acts.shape
        st, sb = B * V, V
    else:
        B, T, V = acts.shape
        st, sb = V, T * V
    L = ys_pad.shape[1]
    assert acts.is_contiguous() and ys_pad.is_contiguous() and ys_pad.dtype == torch.int64 and acts.dtype == torch.float32
    assert ilens.dtype == torch.int32 and ilens.numel() == B and ys_pad.shape[0] == B
    dev = acts.device
    if L == 0:          # no label column at all: one column of padding (the entry point takes no NULL operands)
        seg = torch.empty(B, 0, device=dev, dtype=torch.int32)
        out = ctc_forced_align(acts, ilens, torch.full((B, 1), ignore_id, device=dev, dtype=torch.int64), blank, ignore_id,
                               normalized, time_major)
        return out[:3] + (seg, seg.clone())
    ws = torch.empty(_lib.lib().eamd_ctc_align_workspace_bytes(B, T, L), device=dev, dtype=torch.uint8)
    score = torch.empty(B, device=dev, dtype=torch.float32)
    states = torch.empty(B, T, device=dev, dtype=torch.int32)
    tokens = torch.empty(B, T, device=dev, dtype=torch.int64)
    seg_start = torch.empty(B, L, device=dev, dtype=torch.int32)
    seg_end = torch.empty(B, L, device=dev, dtype=torch.int32)
    check(_lib.lib().eamd_ctc_forced_align(ptr(acts), st, sb, ptr(ys_pad), ptr(ilens), ptr(score),
                                           ptr(states), ptr(tokens), ptr(seg_start), ptr(seg_end), ptr(ws), B, T, V, L, blank,
                                           ignore_id, bool(normalized), stream_ptr()), "eamd_ctc_forced_align")
    return score, states, tokens, seg_start, seg_end


CTC_SEGMENT_MAX_S = 16      # longest token in characters (csrc/ctc_segment.hip kMaxS)


def _seg_align(n, a=256):
    return (n + a - 1) // a * a


def ctc_segment_window(window, Tmax):
    return max(1, min(int(window), int(Tmax)))


def ctc_segment_ring_in_lds(S, window, Tmax):
    """whether the fill kernel keeps its S + 1 columns of values in LDS at this window (else: in the workspace)"""
    rc = _lib.lib().eamd_ctc_segment_ring_in_lds(S, ctc_segment_window(window, Tmax))
    if rc < 0:
        check(rc, "eamd_ctc_segment_ring_in_lds")
    return bool(rc)


def ctc_segment_workspace_layout(nsel, B, Tmax, Lmax, S, window, ring_global=False):
    """byte offsets of (psum, ring, bp) in the workspace of one window attempt, and its size.  ring is None when it lives in LDS"""
    Wm = ctc_segment_window(window, Tmax)
    o_psum, n = 0, _seg_align(B * (Tmax + 1) * 8)
    o_ring = None
    if ring_global or not ctc_segment_ring_in_lds(S, window, Tmax):
        o_ring, n = n, n + _seg_align(nsel * (S + 1) * (Wm + Wm // 32 + 1) * 4)
    o_bp, n = n, n + _seg_align(nsel * Wm * Lmax)
    return o_psum, o_ring, o_bp, n


def ctc_segment_bytes(nsel, B, Tmax, Lmax, S, Umax, window, ring_global=False):
    """device bytes one window attempt needs beside its results: backpointers, ring, prefix sums, and the emission rows"""
    return ctc_segment_workspace_layout(nsel, B, Tmax, Lmax, S, window, ring_global)[3] + B * Umax * Tmax * 4


def ctc_segment_emissions(lpz, lens, tok, blank=0, gratis_blank=False):
    """eamd_ctc_segment_emissions: lpz [B,Tmax,V] fp32 log-probabilities, lens [B] int32, tok [B,Umax] int32 (row 0: blank; -1:
    unused) -> em [B,Umax,Tmax]: the rows the trellis reads, contiguous in t (frames behind lens[b] are left unwritten)"""
    B, Tmax, V = lpz.shape
    assert lpz.dtype == torch.float32 and lpz.is_contiguous() and lens.dtype == torch.int32 and lens.numel() == B
    assert tok.dtype == torch.int32 and tok.is_contiguous() and tok.shape[0] == B
    if not 0 <= blank < V:
        raise ValueError("blank id %d outside the %d outputs" % (blank, V))
    em = torch.empty(B, tok.shape[1], Tmax, device=lpz.device, dtype=torch.float32)
    check(_lib.lib().eamd_ctc_segment_emissions(ptr(lpz), ptr(lens), ptr(tok), ptr(em), B, Tmax, V, tok.shape[1], blank,
                                                bool(gratis_blank), stream_ptr()), "eamd_ctc_segment_emissions")
    return em


def ctc_segment_result_bytes(B, Tmax, Lmax, NU):
    return B * (NU * 3 * 8 + 4 * 4 + 2 * Lmax * 4 + 2 * Tmax * 4)


def ctc_segment_result(B, Tmax, Lmax, NU, device, out=None):
    """the results of eamd_ctc_segment_run as views of ONE byte buffer, so that the host fetches them in one copy: seg [B,NU,3]
    f64 and info [B,4] int32 first (res["head"] bytes: all a caller of the segments needs), then offsets / timings [B,Lmax] int32,
    char_probs [B,Tmax] f32, states [B,Tmax] int32.  out: a byte tensor of res["bytes"] bytes at an 8-byte aligned address"""
    shapes = (("seg", torch.float64, (B, NU, 3)), ("info", torch.int32, (B, 4)), ("offsets", torch.int32, (B, Lmax)),
              ("timings", torch.int32, (B, Lmax)), ("char_probs", torch.float32, (B, Tmax)), ("states", torch.int32, (B, Tmax)))
    total = ctc_segment_result_bytes(B, Tmax, Lmax, NU)
    if out is None:
        out = torch.zeros(total, device=device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.numel() == total and out.is_contiguous() and out.data_ptr() % 8 == 0
    res, o = {"buf": out, "bytes": total}, 0
    for name, d, s in shapes:
        n = math.prod(s) * torch.empty(0, dtype=d).element_size()
        res[name] = out[o:o + n].view(d).view(s)
        o += n
        if name == "info":
            res["head"] = o
    return res


def ctc_segment_fetch(res, full=False):
    """ONE device-to-host copy of a result buffer (its head: seg and info, or all of it) -> dict of numpy arrays"""
    host = (res["buf"] if full else res["buf"][:res["head"]]).cpu()
    out, o = {}, 0
    for name in ("seg", "info") + (("offsets", "timings", "char_probs", "states") if full else ()):
        v = res[name]
        n = v.numel() * v.element_size()
        out[name] = host[o:o + n].view(v.dtype).view(v.shape).numpy()
        o += n
    return out


def ctc_segment_run(em, gtu, tok, lens, llens, sel, utt, nutt, res, window, n_mean, index_duration, ring_global=False,
                    workspace=None):
    """eamd_ctc_segment_run: one window attempt (fill, walk back, segments) for the recordings sel (int32 indices) into the views
    of res (ctc_segment_result); the other recordings keep what res holds.  em [B,Umax,Tmax]; gtu [B,Lmax,S] int32 rows of em
    (-1: no token); tok [B,Umax]; lens / llens [B] frames / characters; utt [B,NU+1], nutt [B] utterance begin indices.
    workspace: a byte tensor of ctc_segment_workspace_layout(...)[3] bytes (256-byte aligned), else allocated here"""
    B, Umax, Tmax = em.shape
    Lmax, S = gtu.shape[1], gtu.shape[2]
    NU = utt.shape[1] - 1
    nsel = sel.numel()
    for t in (gtu, tok, lens, llens, sel, utt, nutt):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == em.device
    assert em.dtype == torch.float32 and em.is_contiguous() and gtu.shape[0] == B and tok.shape == (B, Umax)
    assert lens.numel() == B and llens.numel() == B and nutt.numel() == B and utt.shape[0] == B and 1 <= nsel <= B
    assert res["seg"].shape == (B, NU, 3) and res["offsets"].shape == (B, Lmax) and res["states"].shape == (B, Tmax)
    if S > CTC_SEGMENT_MAX_S:
        raise ValueError("tokens of %d characters: the segmentation kernel takes at most %d" % (S, CTC_SEGMENT_MAX_S))
    o_psum, o_ring, o_bp, nbytes = ctc_segment_workspace_layout(nsel, B, Tmax, Lmax, S, window, ring_global)
    if workspace is None:
        workspace = torch.empty(nbytes, device=em.device, dtype=torch.uint8)
    assert workspace.dtype == torch.uint8 and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0
    base = workspace.data_ptr()
    check(_lib.lib().eamd_ctc_segment_run(ptr(em), ptr(gtu), ptr(tok), ptr(lens), ptr(llens), ptr(sel), ptr(utt), ptr(nutt),
                                          base + o_bp, None if o_ring is None else base + o_ring, base + o_psum,
                                          ptr(res["info"]), ptr(res["offsets"]), ptr(res["timings"]), ptr(res["char_probs"]),
                                          ptr(res["states"]), ptr(res["seg"]), nsel, B, Tmax, Lmax, S, Umax, NU, int(window),
                                          int(n_mean), float(index_duration), bool(ring_global), stream_ptr()),
          "eamd_ctc_segment_run")
    return res


def maskctc_seed(logits, hlens, thr, K, mask_token, eos, blank=0, Lcap=None):
    """Mask-CTC seed (eamd_maskctc_seed): logits [B,T',V] fp32 CTC output-layer activations, hlens [B] int32 (device) valid
    frames -> dict of device tensors: y_in [B,Lcap] int64 (confident token or mask_token, padded with eos), tok_p [B,Lcap] (max p
    over each token's run), len / nmask / niter / kper [B] int32, frame_id / frame_p [B,T'] (per-frame argmax of p and its p,
    valid for t < hlens).  Lcap defaults to T'."""
    B, T, V = logits.shape
    Lcap = T if Lcap is None else int(Lcap)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and hlens.dtype == torch.int32 and hlens.numel() == B
    dev = logits.device
    i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)  # noqa: E731
    out = dict(y_in=torch.empty(B, Lcap, device=dev, dtype=torch.int64), tok_p=torch.empty(B, Lcap, device=dev, dtype=torch.float32),
               len=i32(B), nmask=i32(B), niter=i32(B), kper=i32(B), frame_id=i32(B, T),
               frame_p=torch.empty(B, T, device=dev, dtype=torch.float32))
    check(_lib.lib().eamd_maskctc_seed(ptr(logits), ptr(hlens), ptr(out["frame_id"]), ptr(out["frame_p"]), ptr(out["y_in"]),
                                       ptr(out["tok_p"]), ptr(out["len"]), ptr(out["nmask"]), ptr(out["niter"]), ptr(out["kper"]),
                                       B, T, V, Lcap, blank, mask_token, eos, float(thr), int(K), stream_ptr()),
          "eamd_maskctc_seed")
    return out


def maskctc_update(pass_, logits, y_in, lens, niter, kper, mask_token, score=None, arg=None):
    """one Mask-CTC mask-predict pass (eamd_maskctc_update): logits [B,L,V] fp32 decoder output on y_in[:, :L]; y_in [B,ldy]
    int64 (row-contiguous, ldy >= L) is updated in place; lens / niter / kper [B] int32.  score / arg: optional [B,L] workspaces
    (reused across passes).  -> (score, arg); they hold the max logit and its argmax at the masked rows of active utterances."""
    B, L, V = logits.shape
    assert logits.dtype == torch.float32 and logits.is_contiguous() and y_in.dtype == torch.int64 and y_in.stride(1) == 1
    assert y_in.shape[0] == B and y_in.shape[1] >= L
    dev = logits.device
    if score is None:
        score = torch.empty(B, L, device=dev, dtype=torch.float32)
        arg = torch.empty(B, L, device=dev, dtype=torch.int32)
    check(_lib.lib().eamd_maskctc_update(int(pass_), ptr(logits), ptr(y_in), ptr(lens), ptr(niter), ptr(kper), ptr(score), ptr(arg),
                                         B, L, y_in.stride(0), V, mask_token, stream_ptr()), "eamd_maskctc_update")
    return score, arg


def ctc_prefix_score(logp, r_prev, cand, last, olen, blank, eos):
    """logp [T,V] fp32; r_prev [nhyp,T,2]; cand [nhyp,ncand] int32; last, olen [nhyp] int32
    -> psi [nhyp,ncand], r_new [nhyp,ncand,T,2]"""
    T, V = logp.shape
    nhyp, ncand = cand.shape
    assert r_prev.shape == (nhyp, T, 2) and cand.dtype == torch.int32 and logp.is_contiguous()
    # (candidates come from top-k / arange over the V scores: in range by construction; checking would cost a host sync per beam step)
    psi = torch.empty(nhyp, ncand, device=logp.device, dtype=torch.float32)
    r_new = torch.empty(nhyp, ncand, T, 2, device=logp.device, dtype=torch.float32)
    check(_lib.lib().eamd_ctc_prefix_score(ptr(logp), ptr(r_prev.contiguous()), ptr(cand.contiguous()), ptr(last),
                                           ptr(olen), ptr(psi), ptr(r_new), nhyp, ncand, T, V, blank, eos,
                                           stream_ptr()), "eamd_ctc_prefix_score")
    return psi, r_new


def ctc_prefix_score_batch(logp, lens, per_utt, r_prev, cand, last, olen, blank, eos):
    """the hypotheses of several utterances at once: logp [U,Tmax,V], lens [U] int32 (device), r_prev [U*per_utt,Tmax,2],
    cand [U*per_utt,ncand] int32 -> psi [U*per_utt,ncand], r_new [U*per_utt,ncand,Tmax,2] (rows beyond an utterance's length: 0)"""
    U, Tmax, V = logp.shape
    nhyp, ncand = cand.shape
    assert nhyp == U * per_utt and r_prev.shape == (nhyp, Tmax, 2) and cand.dtype == torch.int32 and logp.is_contiguous()
    assert lens.dtype == torch.int32 and lens.numel() == U
    psi = torch.empty(nhyp, ncand, device=logp.device, dtype=torch.float32)
    r_new = torch.zeros(nhyp, ncand, Tmax, 2, device=logp.device, dtype=torch.float32)
    check(_lib.lib().eamd_ctc_prefix_score_batch(ptr(logp), ptr(lens), U, per_utt, ptr(r_prev.contiguous()), ptr(cand.contiguous()),
                                                 ptr(last), ptr(olen), ptr(psi), ptr(r_new), ncand, Tmax, V, blank, eos,
                                                 stream_ptr()), "eamd_ctc_prefix_score_batch")
    return psi, r_new


def ctc_prefix_psi(logp, lens, per_utt, r_prev, cand, last, olen, blank, eos, olen_dev=None):
    """log psi of the candidates as a parallel reduction over the frames (eamd_ctc_prefix_psi_dyn): logp [U, Tmax, V], r_prev
    [U * per_utt, Tmax, 2], cand [n, P] int32, last [n] int32, olen int -> psi [n, P]; None when the library declines (Tmax > 2048)"""
    U, Tmax, V = logp.shape
    nhyp, ncand = cand.shape
    assert nhyp == U * per_utt and r_prev.shape == (nhyp, Tmax, 2) and cand.dtype == torch.int32 and logp.is_contiguous()
    psi = torch.empty(nhyp, ncand, device=logp.device, dtype=torch.float32)
    # olen_dev: int32 device scalar added to olen (the step index of a replayed beam step)
    rc = _lib.lib().eamd_ctc_prefix_psi_dyn(ptr(logp), ptr(lens), U, per_utt, ptr(r_prev.contiguous()), ptr(cand.contiguous()), ptr(last),
                                            int(olen), ptr(olen_dev), ptr(psi), ncand, Tmax, V, blank, eos, stream_ptr())
    if rc == _lib.EAMD_EUNSUPPORTED:
        return None
    check(rc, "eamd_ctc_prefix_psi_dyn")
    return psi


def ctc_prefix_state(logp, lens, per_utt, r_prev, parent, tok, last, olen, alive, blank, out=None, olen_dev=None):
    """forward variables of the continuations that survived a selection (eamd_ctc_prefix_state_dyn): slot s continues hypothesis
    parent[s] (whose state is r_prev[parent[s]], last token last[parent[s]], prefix length olen + 1) with token tok[s];
    alive [n] = the slots' running scores (-inf: ended / empty) -> r [n, Tmax, 2]"""
    U, Tmax, V = logp.shape
    n = parent.numel()
    r = out if out is not None else torch.empty(n, Tmax, 2, device=logp.device, dtype=torch.float32)
    check(_lib.lib().eamd_ctc_prefix_state_dyn(ptr(logp), ptr(lens), U, per_utt, ptr(r_prev), ptr(parent), ptr(tok), ptr(last), int(olen),
                                               ptr(olen_dev), ptr(alive), ptr(r), Tmax, V, blank, stream_ptr()), "eamd_ctc_prefix_state_dyn")
    return r


# ---- optimizer -------------------------------------------------------------------------------------
def grad_norm(g, ws, out):
    check(_lib.lib().eamd_grad_norm(ptr(g), g.numel(), ptr(ws), ptr(out), stream_ptr()),
          "eamd_grad_norm")


def sched_step(state, gnorm, mode, base_lr, factor, dmodel, warmup, beta1, beta2, max_norm):
    check(_lib.lib().eamd_sched_step(ptr(state), ptr(gnorm), mode, base_lr, factor,
                                     dmodel, warmup, beta1, beta2,
                                     max_norm, stream_ptr()), "eamd_sched_step")


def adam_step(p, g, m, v, state, beta1, beta2, eps, weight_decay, p16=None):
    n = p.numel()
    assert g.numel() == n and m.numel() == n and v.numel() == n and (p16 is None or p16.numel() == n)
    check(_lib.lib().eamd_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p16), n, ptr(state), beta1,
                                    beta2, eps, weight_decay, stream_ptr()),
          "eamd_adam_step")


def adadelta_step(p, g, sq, acc, state, rho, weight_decay, p16=None):
    check(_lib.lib().eamd_adadelta_step(ptr(p), ptr(g), ptr(sq), ptr(acc), ptr(p16), p.numel(), ptr(state),
                                        rho, weight_decay, stream_ptr()), "eamd_adadelta_step")


def add_gradient_noise(g, sigma, salt=0x6e6f697365):
    """g += sigma * N(0, 1) over a flat fp32 gradient buffer (draws keyed by the device step counter)"""
    check(_lib.lib().eamd_add_gradient_noise(ptr(g), g.numel(), sigma, ptr(rng_state(g.device)),
                                             salt, stream_ptr()), "eamd_add_gradient_noise")


def make_gather(Cc, taps, Ho, Wo, Hin, Win, sh, sw):
    g = GatherT()
    g.enabled = 1
    g.C, g.ntap, g.Ho, g.Wo, g.Hin, g.Win, g.sh, g.sw = Cc, len(taps), Ho, Wo, Hin, Win, sh, sw
    for i, (dh, dw) in enumerate(taps):
        g.dh[i] = dh
        g.dw[i] = dw
    return g


def make_rowmap(Ho, Wo, Hc, Wc, sh, oh, sw, ow):
    m = RowMapT()
    m.enabled = 1
    m.Ho, m.Wo, m.Hc, m.Wc, m.sh, m.oh, m.sw, m.ow = Ho, Wo, Hc, Wc, sh, oh, sw, ow
    return m


# ---- recurrent layers / RNN-Transducer (rows a20, a21) -------------------------------------------
ACT_TANH, ACT_HARDTANH, ACT_SELU = 3, 4, 5      # eamd_act ids beyond relu / swish (nets_utils.py:485-498)


def act_fwd_any(x, act):
    y = torch.empty_like(x)
    check(_lib.lib().eamd_act_fwd(ptr(x), ptr(y), x.numel(), act, stream_ptr()), "eamd_act_fwd")
    return y


def act_bwd_any(dy, x, act):
    dx = torch.empty_like(x)
    check(_lib.lib().eamd_act_bwd(ptr(dy), ptr(x), ptr(dx), x.numel(), act, stream_ptr()), "eamd_act_bwd")
    return dx


def lstm_cell_fwd(gates, c_prev, h_prev, live, h, c, y, acts):
    B, H4 = gates.shape
    H = H4 // 4
    assert c_prev.numel() == B * H and h.numel() == B * H and c.numel() == B * H and acts.numel() == B * H4
    assert live is None or (live.dtype == torch.uint8 and live.numel() == B and h_prev is not None)
    check(_lib.lib().eamd_lstm_cell_fwd(ptr(gates), ptr(c_prev), ptr(h_prev), ptr(live), ptr(h), ptr(c), ptr(y),
                                        ptr(acts), B, H, stream_ptr()), "eamd_lstm_cell_fwd")


def lstm_cell_bwd(dy, dh, dc, acts, c_prev, c, live, dgates, dc_prev, dh_pass):
    B, H4 = acts.shape
    H = H4 // 4
    assert dgates.numel() == B * H4 and dc_prev.numel() == B * H
    check(_lib.lib().eamd_lstm_cell_bwd(ptr(dy), ptr(dh), ptr(dc), ptr(acts), ptr(c_prev), ptr(c), ptr(live),
                                        ptr(dgates), ptr(dc_prev), ptr(dh_pass), B, H, stream_ptr()),
          "eamd_lstm_cell_bwd")


def lstm_step_ok(B, H):
    """shapes the one-launch LSTM step kernels take"""
    return LSTM_FUSED_STEP and H % 64 == 0 and B <= 64


LSTM_FUSED_STEP = True      # tests flip this to compare against the GEMM + cell-kernel steps


# bench.py: list collecting the recurrent launches of one step as (tag, operand references, replay(stream_ptr), bytes)
_rnn_record = None


def lstm_step_fwd(gx_t, w_hh, b_hh, h_prev, c_prev, live_t, h, c, y, acts):
    B, H4 = gx_t.shape
    H = H4 // 4
    args = (ptr(gx_t), ptr(w_hh), ptr(b_hh), ptr(h_prev), ptr(c_prev), ptr(live_t), ptr(h), ptr(c), ptr(y), ptr(acts), B, H)
    fn = _lib.lib().eamd_lstm_step_fwd
    if _rnn_record is not None:
        _rnn_record.append(("lstm_step_fwd", (gx_t, w_hh, b_hh, h_prev, c_prev, live_t, h, c, y, acts),
                            lambda sp, args=args: check(fn(*args, sp), "eamd_lstm_step_fwd"), 4 * (H4 * H + 3 * B * H4)))
    check(fn(*args, stream_ptr()), "eamd_lstm_step_fwd")


def lstm_step_bwd(dy_t, dgates_next, w_t, dh_pass_in, dc, acts, c_prev, c, live_t, dgates, dc_prev, dh_pass):
    B, H4 = acts.shape
    H = H4 // 4
    args = (ptr(dy_t), ptr(dgates_next), ptr(w_t), ptr(dh_pass_in), ptr(dc), ptr(acts), ptr(c_prev), ptr(c), ptr(live_t),
            ptr(dgates), ptr(dc_prev), ptr(dh_pass), B, H)
    fn = _lib.lib().eamd_lstm_step_bwd
    if _rnn_record is not None:
        _rnn_record.append(("lstm_step_bwd", (dy_t, dgates_next, w_t, dh_pass_in, dc, acts, c_prev, c, live_t, dgates, dc_prev, dh_pass),
                            lambda sp, args=args: check(fn(*args, sp), "eamd_lstm_step_bwd"), 4 * (H4 * H + 4 * B * H4)))
    check(fn(*args, stream_ptr()), "eamd_lstm_step_bwd")


LSTM_PERSISTENT = True      # whole-sequence persistent LSTM launches (csrc/lstm_seq.hip); tests flip it
_lstm_seq_last_ws = None    # sync words of the most recent persistent launch (lstm_seq_status)


_comm_overlap = False      # a gradient all-reduce may run beside backward (train.GradReducer / GraphedDataParallelStep, world > 1)
_lstm_seq_sticky = {}       # device index -> int32 word: first give-up code of any persistent launch since it was last cleared


def set_comm_overlap(active):
    """the data-parallel drivers announce collectives that overlap backward: their kernels hold CUs, and a persistent LSTM launch
    needs one workgroup on EVERY CU at once (it would sit in its flag waits until the collective drains) - lstm_seq_ok then
    declines and the per-step kernels run"""
    global _comm_overlap
    _comm_overlap = bool(active)


def lstm_seq_ok(njobs, B, H):
    """shapes eamd_lstm_seq_fwd / _bwd take for `njobs` recurrences side by side (one workgroup per CU for the whole
    launch; the entry points themselves answer EAMD_EUNSUPPORTED for anything else)"""
    if not (LSTM_PERSISTENT and LSTM_FUSED_STEP and H % 64 == 0 and B <= 64 and H <= 1024) or _comm_overlap:
        return False
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return njobs * (H // 8) <= cus and njobs * (H // 16) * ((B + 15) // 16) <= cus


def _lstm_seq_ws(dev):
    global _lstm_seq_last_ws
    n = _lib.lib().eamd_lstm_seq_sync_bytes()
    _lstm_seq_last_ws = torch.empty(n, dtype=torch.uint8, device=dev)
    return _lstm_seq_last_ws


def lstm_seq_fwd(jobs, T, B, H):
    """jobs: list of (gx [T,B,4H], w_hh, b_hh, live [T,B] | None, h_out, c_out, y, acts, reverse) - ONE persistent launch"""
    arr = (_lib.LstmSeqFwdT * len(jobs))()
    for q, (gx, w, b, live, h, c, y, acts, rev) in zip(arr, jobs):
        q.gx, q.w_hh, q.b_hh, q.live = ptr(gx), ptr(w), ptr(b), ptr(live)
        q.h_out, q.c_out, q.y, q.acts, q.reverse = ptr(h), ptr(c), ptr(y), ptr(acts), bool(rev)
    ws = _lstm_seq_ws(jobs[0][0].device)
    fn = _lib.lib().eamd_lstm_seq_fwd
    args = (arr, len(jobs), T, B, H, ptr(ws))
    if _rnn_record is not None:
        _rnn_record.append(("lstm_seq_fwd", (jobs, ws, arr), lambda sp, args=args: check(fn(*args, sp), "eamd_lstm_seq_fwd"),
                            4 * len(jobs) * (4 * H * H + T * B * 9 * H), 2.0 * len(jobs) * (T - 1) * B * 4 * H * H))
    check(fn(*args, stream_ptr()), "eamd_lstm_seq_fwd")
    _lstm_seq_merge(ws)


def lstm_seq_bwd(jobs, T, B, H):
    """jobs: list of (dy [T,B,H], w_t [H,4H], acts, c_out, live | None, dgates (out), reverse = the FORWARD direction)"""
    arr = (_lib.LstmSeqBwdT * len(jobs))()
    for q, (dy, w_t, acts, c, live, dg, rev) in zip(arr, jobs):
        q.dy, q.w_t, q.acts, q.c_out, q.live, q.dgates, q.reverse = ptr(dy), ptr(w_t), ptr(acts), ptr(c), ptr(live), ptr(dg), bool(rev)
    ws = _lstm_seq_ws(jobs[0][2].device)
    fn = _lib.lib().eamd_lstm_seq_bwd
    args = (arr, len(jobs), T, B, H, ptr(ws))
    if _rnn_record is not None:
        _rnn_record.append(("lstm_seq_bwd", (jobs, ws, arr), lambda sp, args=args: check(fn(*args, sp), "eamd_lstm_seq_bwd"),
                            4 * len(jobs) * (4 * H * H + T * B * 11 * H), 2.0 * len(jobs) * (T - 1) * B * 4 * H * H))
    check(fn(*args, stream_ptr()), "eamd_lstm_seq_bwd")
    _lstm_seq_merge(ws)


def _lstm_seq_merge(ws):
    """fold the launch's status word into the device's sticky word (one tiny launch, no synchronisation)"""
    dev = ws.device
    st = _lstm_seq_sticky.get(dev.index)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            return                   # first persistent launch inside a capture: no persistent word yet (eager warm-ups come first)
        st = _lstm_seq_sticky[dev.index] = torch.zeros(1, dtype=torch.int32, device=dev)
    check(_lib.lib().eamd_lstm_seq_status_merge(ptr(ws), ptr(st), stream_ptr()), "eamd_lstm_seq_status_merge")


def lstm_seq_sticky_status(clear=True):
    """first give-up code of ANY persistent LSTM launch on the current device since the last clear (synchronises: call it
    where the host waits anyway - train.EpochRunner does once per epoch); 0 = all hand-off waits completed"""
    st = _lstm_seq_sticky.get(torch.cuda.current_device()) if torch.cuda.is_available() else None
    if st is None:
        return 0
    v = int(st.item())
    if v and clear:
        st.zero_()
    return v


def lstm_seq_status():
    """status word of the most recent persistent LSTM launch (synchronises): 0 = every hand-off wait completed"""
    if _lstm_seq_last_ws is None:
        return 0
    return _lib.lib().eamd_lstm_seq_status(ptr(_lstm_seq_last_ws), stream_ptr())


def maxpool2x2_fwd(x):
    B, H, W, Cc = x.shape
    y = torch.empty(B, (H + 1) // 2, (W + 1) // 2, Cc, device=x.device, dtype=torch.float32)
    idx = torch.empty(y.shape, device=x.device, dtype=torch.uint8)
    check(_lib.lib().eamd_maxpool2x2_fwd(ptr(x), ptr(y), ptr(idx), B, H, W, Cc, stream_ptr()), "eamd_maxpool2x2_fwd")
    return y, idx


def maxpool2x2_bwd(dy, idx, shape):
    B, H, W, Cc = shape
    dx = torch.empty(B, H, W, Cc, device=dy.device, dtype=torch.float32)
    check(_lib.lib().eamd_maxpool2x2_bwd(ptr(dy), ptr(idx), ptr(dx), B, H, W, Cc, stream_ptr()), "eamd_maxpool2x2_bwd")
    return dx


def conv3x3_c1_fwd(x, w, bias, B, T, F, Cc, out_dtype=torch.float32):
    assert x.numel() == B * T * F and w.numel() == Cc * 9
    y = torch.empty(B, T, F, Cc, device=x.device, dtype=out_dtype)
    check(_lib.lib().eamd_conv3x3_c1_fwd(ptr(x), ptr(w), ptr(bias), ptr(y), B, T, F, Cc,
                                         1 if out_dtype == torch.bfloat16 else 0, stream_ptr()), "eamd_conv3x3_c1_fwd")
    return y


def conv3x3_c1_bwd_w(dy, x, dw, db, B, T, F, Cc):
    L = _lib.lib()
    ws = torch.empty(L.eamd_conv3x3_c1_bwd_w_workspace(B, T, Cc), device=x.device, dtype=torch.float32)
    check(L.eamd_conv3x3_c1_bwd_w(ptr(dy), ptr(x), ptr(dw), ptr(db), ptr(ws), B, T, F, Cc,
                                  1 if dy.dtype == torch.bfloat16 else 0, stream_ptr()), "eamd_conv3x3_c1_bwd_w")


def conv3x3_c1_bwd_x(dy, w, B, T, F, Cc, out=None):
    """dy [B,T,F,C] fp32 / bf16, w [C,1,3,3] -> dx [B,T,F] fp32"""
    assert dy.numel() == B * T * F * Cc and w.numel() == Cc * 9 and dy.is_contiguous() and w.is_contiguous()
    assert dy.dtype in (torch.float32, torch.bfloat16) and w.dtype == torch.float32
    dx = torch.empty(B, T, F, device=dy.device, dtype=torch.float32) if out is None else out
    assert dx.shape == (B, T, F) and dx.dtype == torch.float32 and dx.is_contiguous()
    check(_lib.lib().eamd_conv3x3_c1_bwd_x(ptr(dy), ptr(w), ptr(dx), B, T, F, Cc, 1 if dy.dtype == torch.bfloat16 else 0,
                                           stream_ptr()), "eamd_conv3x3_c1_bwd_x")
    return dx


def joint_fwd(enc, dec, act, out_dtype=torch.float32):
    B, T, J = enc.shape
    U = dec.shape[1]
    assert dec.shape[0] == B and dec.shape[2] == J and enc.is_contiguous() and dec.is_contiguous()
    out = torch.empty(B, T, U, J, device=enc.device, dtype=out_dtype)
    o32, o16 = (ptr(out), None) if out_dtype == torch.float32 else (None, ptr(out))
    check(_lib.lib().eamd_joint_fwd(ptr(enc), ptr(dec), o32, o16, B, T, U, J, act, stream_ptr()), "eamd_joint_fwd")
    return out


def joint_bwd(dh, enc, dec, act):
    B, T, J = enc.shape
    U = dec.shape[1]
    assert dh.numel() == B * T * U * J and dh.dtype == torch.float32
    d_enc = torch.empty_like(enc)
    d_dec = torch.empty_like(dec)
    check(_lib.lib().eamd_joint_bwd(ptr(dh), ptr(enc), ptr(dec), ptr(d_enc), ptr(d_dec), B, T, U, J, act,
                                    stream_ptr()), "eamd_joint_bwd")
    return d_enc, d_dec


def rnnt_grad(logits, labels, tlens, ulens, blank, ws, gscale, scale, grad=None):
    """d loss / d logits from the lattice workspace `ws` of a previous rnnt_loss(..., return_ws=True) call;
    gscale: 0-dim / 1-element device tensor multiplied in (the upstream gradient of the scalar loss)"""
    B, T, U, V = logits.shape
    grad = torch.empty_like(logits) if grad is None else grad
    lab = labels if labels.numel() > 0 else torch.zeros(1, device=logits.device, dtype=torch.int32)
    check(_lib.lib().eamd_rnnt_grad(ptr(logits), ptr(lab), ptr(tlens), ptr(ulens), ptr(ws), ptr(grad), B, T, U, V, blank,
                                    ptr(gscale), scale, stream_ptr()), "eamd_rnnt_grad")
    return grad


def rnnt_loss(logits, labels, tlens, ulens, blank, grad=None, gscale=None, scale=1.0, return_ws=False):
    """logits [B,T,U,V] fp32; labels [B,U-1] int32; tlens/ulens [B] int32 -> per-utterance loss [B]"""
    B, T, U, V = logits.shape
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == B * max(U - 1, 0)
    assert tlens.dtype == torch.int32 and ulens.dtype == torch.int32 and tlens.numel() == B and ulens.numel() == B
    assert grad is None or (grad.numel() == logits.numel() and grad.dtype == torch.float32)
    ws = torch.empty(_lib.lib().eamd_rnnt_workspace(B, T, U), device=logits.device, dtype=torch.float32)
    loss = torch.empty(B, device=logits.device, dtype=torch.float32)
    lab = labels if labels.numel() > 0 else torch.zeros(1, device=logits.device, dtype=torch.int32)
    check(_lib.lib().eamd_rnnt_loss(ptr(logits), ptr(lab), ptr(tlens), ptr(ulens), ptr(ws), ptr(loss), ptr(grad),
                                    B, T, U, V, blank, ptr(gscale), scale, stream_ptr()), "eamd_rnnt_loss")
    return (loss, ws) if return_ws else loss


def rnnt_workspace(B, T, U, device):
    return torch.empty(_lib.lib().eamd_rnnt_workspace(B, T, U), device=device, dtype=torch.float32)


def rnnt_node_stats(z_rows, labels, ws, node0, B, T, U, blank):
    """lse / log p(blank) / log p(label) of the lattice rows node0.. (z_rows [nrows, V] fp32) into the workspace"""
    nrows, V = z_rows.shape
    assert z_rows.dtype == torch.float32 and z_rows.is_contiguous() and labels.dtype == torch.int32
    check(_lib.lib().eamd_rnnt_node_stats(ptr(z_rows), ptr(labels), ptr(ws), node0, nrows, B, T, U, V,
                                          blank, stream_ptr()), "eamd_rnnt_node_stats")


RNNT_FUSED_STATS = True     # tests flip this to reach the stored-logits form (linear_fwd + eamd_rnnt_node_stats)


def rnnt_node_stats_fused(H2, W, b_out, col, ws, node0, B, T, U, blank):
    """the node statistics of the lattice rows node0.. straight from the joint activations H2 [nrows, J] (operand dtype) and
    the output projection W [V, J] / b_out: the logits GEMM runs with the row-statistics epilogue (no logits written) and
    eamd_rnnt_node_stats_part combines its partials.  col [nrows] int32: each node's next label or -1.
    Returns False if the library declines (the caller then stores the logits)."""
    if not RNNT_FUSED_STATS:
        return False
    nrows, J = H2.shape
    V = W.shape[0]
    tile = 128 if nrows >= 2048 else 64
    tn = (V + tile - 1) // tile
    dev = H2.device
    part = torch.empty(nrows * tn * 2, device=dev, dtype=torch.float32)
    zcol = torch.empty(nrows, device=dev, dtype=torch.float32)
    zfix = torch.empty(nrows, device=dev, dtype=torch.float32)
    try:
        gemm(H2, W, None, nrows, V, J, J, J, V, bias=b_out, epilogue=EPI_ROW_STATS, tile=tile,
             stats=(part, col, zcol, zfix, blank))
    except _lib.EamdError as e:
        if ("code %d" % _lib.EAMD_EUNSUPPORTED) in str(e):
            return False
        raise
    check(_lib.lib().eamd_rnnt_node_stats_part(ptr(part), ptr(zcol), ptr(zfix), ptr(ws), node0, nrows, tn,
                                               B, T, U, stream_ptr()), "eamd_rnnt_node_stats_part")
    return True


def rnnt_node_grad_fused(H2, W, b_out, labels, tlens, ulens, ws, node0, B, T, U, blank, gscale, scale, out_dtype):
    """d loss / d logits of the lattice rows node0.. -> [nrows, V] in out_dtype, written by the recomputing logits GEMM itself
    (epilogue 8 with eamd_rnnt_row_coef's per-node coefficients): no fp32 logits chunk, no separate gradient pass.
    Returns None if the library declines."""
    if not RNNT_FUSED_STATS:
        return None
    nrows, J = H2.shape
    V = W.shape[0]
    dev = H2.device
    rowc = torch.empty(nrows * 3, device=dev, dtype=torch.float32)
    col = torch.empty(nrows, device=dev, dtype=torch.int32)
    check(_lib.lib().eamd_rnnt_row_coef(ptr(labels), ptr(tlens), ptr(ulens), ptr(ws), ptr(rowc), ptr(col), node0,
                                        nrows, B, T, U, stream_ptr()), "eamd_rnnt_row_coef")
    dZ = torch.empty(nrows, V, device=dev, dtype=out_dtype)
    try:
        gemm(H2, W, dZ, nrows, V, J, J, J, V, bias=b_out, epilogue=EPI_ROW_GRAD, tile=128 if nrows >= 2048 else 64,
             stats=(rowc, col, blank, gscale, scale))
    except _lib.EamdError as e:
        if ("code %d" % _lib.EAMD_EUNSUPPORTED) in str(e):
            return None
        raise
    return dZ


def rnnt_alpha_beta(ws, tlens, ulens, B, T, U):
    loss = torch.empty(B, device=ws.device, dtype=torch.float32)
    check(_lib.lib().eamd_rnnt_alpha_beta(ptr(ws), ptr(tlens), ptr(ulens), ptr(loss), B, T, U, stream_ptr()),
          "eamd_rnnt_alpha_beta")
    return loss


def rnnt_node_grad(z_rows, labels, tlens, ulens, ws, node0, B, T, U, blank, gscale, scale, out_dtype=torch.float32):
    """d loss / d logits of the lattice rows node0.. -> [nrows, V] in out_dtype (fp32: written over z_rows)"""
    nrows, V = z_rows.shape
    if out_dtype == torch.float32:
        g32, g16, out = ptr(z_rows), None, z_rows
    else:
        out = torch.empty(nrows, V, device=z_rows.device, dtype=torch.bfloat16)
        g32, g16 = None, ptr(out)
    check(_lib.lib().eamd_rnnt_node_grad(ptr(z_rows), g32, g16, ptr(labels), ptr(tlens), ptr(ulens), ptr(ws), node0,
                                         nrows, B, T, U, V, blank, ptr(gscale), scale, stream_ptr()),
          "eamd_rnnt_node_grad")
    return out


def attloc_fwd(att_prev, conv_w, w_att, pre_enc, dec_proj, gvec, gb, lens, enc_h, scaling):
    B, T, A = pre_enc.shape
    Cc, K = (conv_w.shape[0], conv_w.shape[-1]) if conv_w is not None else (0, 0)   # no conv: additive attention
    R = conv_w.shape[2] if (conv_w is not None and conv_w.dim() == 4) else 1          # rows of attention history
    E = enc_h.shape[2]
    dev = enc_h.device
    assert dec_proj.shape == (B, A) and gvec.numel() == A and lens.dtype == torch.int32 and lens.numel() == B
    assert conv_w is None or (att_prev.numel() == B * R * T and w_att.shape == (A, Cc) and conv_w.numel() == Cc * R * K)
    e = torch.empty(B, T, device=dev, dtype=torch.float32)
    th = torch.empty(B, T, A, device=dev, dtype=torch.float32)
    conv = torch.empty(B, T, Cc, device=dev, dtype=torch.float32) if Cc else None
    w = torch.empty(B, T, device=dev, dtype=torch.float32)
    ctx = torch.empty(B, E, device=dev, dtype=torch.float32)
    check(_lib.lib().eamd_attloc_fwd(ptr(att_prev), ptr(conv_w), ptr(w_att), ptr(pre_enc), ptr(dec_proj), ptr(gvec),
                                     ptr(gb), ptr(lens), ptr(enc_h), scaling, ptr(e), ptr(th), ptr(conv),
                                     ptr(w), ptr(ctx), B, T, A, Cc, K, R, E, stream_ptr()), "eamd_attloc_fwd")
    return ctx, w, th, conv


def attloc_bwd_energy(dctx, dw_ext, w, enc_h, th, gvec, scaling, dgvec, dgb):
    B, T, A = th.shape
    E = enc_h.shape[2]
    dev = enc_h.device
    de = torch.empty(B, T, device=dev, dtype=torch.float32)
    d_enc_h = torch.empty(B, T, E, device=dev, dtype=torch.float32)
    df = torch.empty(B, T, A, device=dev, dtype=torch.float32)
    d_dec = zeros(B, A, device=dev)
    check(_lib.lib().eamd_attloc_bwd_energy(ptr(dctx), ptr(dw_ext), ptr(w), ptr(enc_h), ptr(th), ptr(gvec),
                                            scaling, ptr(de), ptr(d_enc_h), ptr(df), ptr(dgvec), ptr(dgb),
                                            ptr(d_dec), B, T, A, E, stream_ptr()), "eamd_attloc_bwd_energy")
    return d_enc_h, df, d_dec


ATTLOC_FUSED_BWD = True     # tests flip this to reach the GEMM form of the two products over mlp_att's weight


def attloc_bwd_energy_conv(dctx, dw_ext, w, enc_h, th, gvec, scaling, conv, w_att, dgvec, dgb, dw_att, acc=None):
    """attloc_bwd_energy plus dconv = df @ W_att and dw_att += df^T conv from the same pass over th
    (eamd_attloc_bwd_energy_conv).  Returns (d_enc_h, df, d_dec, dconv), or None if the library declines the shape.
    acc: a dict shared by the decoder steps of one utterance batch - d_enc_h and df (gradients of step-invariant tensors)
    are then kept as ONE running sum in it (created by the first call, added to by the later ones) and returned as such."""
    B, T, A = th.shape
    E, Cc = enc_h.shape[2], conv.shape[2]
    if not ATTLOC_FUSED_BWD or Cc > 16 or A % 4 or A > 1024:
        return None
    dev = enc_h.device
    lib = _lib.lib()
    nws = lib.eamd_attloc_bwd_workspace(B, T, A, Cc) // 4
    ws = torch.empty(nws, device=dev, dtype=torch.float32)
    de = torch.empty(B, T, device=dev, dtype=torch.float32)
    accumulate = acc is not None and "df" in acc
    if accumulate:
        d_enc_h, df = acc["deh"], acc["df"]
    else:
        d_enc_h = torch.empty(B, T, E, device=dev, dtype=torch.float32)
        df = torch.empty(B, T, A, device=dev, dtype=torch.float32)
    dconv = torch.empty(B, T, Cc, device=dev, dtype=torch.float32)
    d_dec = zeros(B, A, device=dev)
    rc = lib.eamd_attloc_bwd_energy_conv(ptr(dctx), ptr(dw_ext), ptr(w), ptr(enc_h), ptr(th), ptr(gvec), scaling,
                                         ptr(conv), ptr(w_att), ptr(de), ptr(d_enc_h), ptr(df), ptr(dconv), ptr(dgvec),
                                         ptr(dgb), ptr(d_dec), ptr(dw_att), ptr(ws), int(accumulate), B, T, A, Cc, E,
                                         stream_ptr())
    if rc == _lib.EAMD_EUNSUPPORTED:
        return None
    check(rc, "eamd_attloc_bwd_energy_conv")
    if acc is not None and not accumulate:
        acc["deh"], acc["df"] = d_enc_h, df
    return d_enc_h, df, d_dec, dconv


def attloc_bwd_conv(dconv, conv_w, att_prev, dconv_w):
    B, T, Cc = dconv.shape
    K = conv_w.shape[-1]
    R = conv_w.shape[2] if conv_w.dim() == 4 else 1
    d_prev = torch.empty(att_prev.shape, device=dconv.device, dtype=torch.float32)
    check(_lib.lib().eamd_attloc_bwd_conv(ptr(dconv), ptr(conv_w), ptr(att_prev), ptr(d_prev), ptr(dconv_w), B, T, Cc,
                                          K, R, stream_ptr()), "eamd_attloc_bwd_conv")
    return d_prev


def attloc_convmax_fwd(att_prev, conv_w):
    """att_prev [B,T], conv_w [C,1,1,K] -> pooled [B,C] = max_t relu(conv), idx [B,C] int32 (AttLocRec front end)"""
    B, T = att_prev.shape
    Cc, K = conv_w.shape[0], conv_w.shape[-1]
    pooled = torch.empty(B, Cc, device=att_prev.device, dtype=torch.float32)
    idx = torch.empty(B, Cc, device=att_prev.device, dtype=torch.int32)
    check(_lib.lib().eamd_attloc_convmax_fwd(ptr(att_prev), ptr(conv_w), ptr(pooled), ptr(idx), B, T, Cc, K, stream_ptr()),
          "eamd_attloc_convmax_fwd")
    return pooled, idx


def attloc_convmax_bwd(dpool, pooled, idx, att_prev, conv_w, dconv_w):
    B, T = att_prev.shape
    Cc, K = conv_w.shape[0], conv_w.shape[-1]
    d_prev = zeros(B, T, device=att_prev.device)
    check(_lib.lib().eamd_attloc_convmax_bwd(ptr(dpool), ptr(pooled), ptr(idx), ptr(att_prev), ptr(conv_w), ptr(d_prev),
                                             ptr(dconv_w), B, T, Cc, K, stream_ptr()), "eamd_attloc_convmax_bwd")
    return d_prev


def mask_rows(x, keep):
    """x [rows, D] fp32, keep [rows] uint8 -> rows with keep == 0 zeroed"""
    rows, D = x.shape
    assert keep.dtype == torch.uint8 and keep.numel() == rows and x.dtype == torch.float32
    y = torch.empty_like(x)
    check(_lib.lib().eamd_mask_rows(ptr(x), ptr(keep), ptr(y), rows, D, stream_ptr()), "eamd_mask_rows")
    return y


def att_dot_fwd(k, q, v, lens, scaling):
    """dot-product attention step: k [B,T,A], q [B,A] (both tanh-activated), v [B,T,E] -> ctx [B,E], w [B,T]"""
    B, T, A = k.shape
    E = v.shape[2]
    dev = k.device
    e = torch.empty(B, T, device=dev, dtype=torch.float32)
    w = torch.empty(B, T, device=dev, dtype=torch.float32)
    ctx = torch.empty(B, E, device=dev, dtype=torch.float32)
    L = _lib.lib()
    check(L.eamd_att_dot_energy_fwd(ptr(k), ptr(q), ptr(lens), ptr(e), B, T, A, stream_ptr()), "eamd_att_dot_energy_fwd")
    check(L.eamd_att_ctx_fwd(ptr(e), ptr(v), scaling, ptr(w), ptr(ctx), B, T, E, stream_ptr()),
          "eamd_att_ctx_fwd")
    return ctx, w


def att_dot_bwd(dctx, dw_ext, w, k, q, v, scaling):
    B, T, A = k.shape
    E = v.shape[2]
    dev = k.device
    de = torch.empty(B, T, device=dev, dtype=torch.float32)
    d_v = torch.empty(B, T, E, device=dev, dtype=torch.float32)
    dk = torch.empty(B, T, A, device=dev, dtype=torch.float32)
    dq = zeros(B, A, device=dev)
    dsum = zeros(1, device=dev)
    L = _lib.lib()
    check(L.eamd_att_ctx_bwd(ptr(dctx), ptr(dw_ext), ptr(w), ptr(v), scaling, ptr(de), ptr(d_v), ptr(dsum),
                             B, T, E, stream_ptr()), "eamd_att_ctx_bwd")
    check(L.eamd_att_dot_energy_bwd(ptr(de), ptr(k), ptr(q), ptr(dk), ptr(dq), B, T, A, stream_ptr()),
          "eamd_att_dot_energy_bwd")
    return d_v, dk, dq


# ---- host constants on the device ----------------------------------------------------------------
# Length vectors, padding masks and padded label matrices are integer work the reference does on the host
# (nets_utils.py:64-176, rnn/decoders.py:167-190).  They are small and depend only on the batch's lengths / labels,
# so the device copies are cached by content: the eager warm-up step of a batch uploads them once and a later
# hipGraph capture / replay of the same batch finds them resident (no host-to-device copy inside a capture).
_h2d_cache = {}


def h2d_cached(tag, array, device):
    """device tensor holding `array` (numpy), cached by (tag, dtype, shape, bytes)"""
    import numpy as np
    a = np.ascontiguousarray(array)
    key = (tag, str(device), a.dtype.str, a.shape, a.tobytes())
    t = _h2d_cache.get(key)
    if t is None:
        if len(_h2d_cache) > 4096:
            _h2d_cache.clear()
        t = torch.from_numpy(a.copy()).to(device)
        _h2d_cache[key] = t
    return t


_side_streams = {}
TWO_STREAM_BIRNN = True     # the two directions of a bidirectional recurrent layer on two streams (tests flip it)


def side_stream(device, i=0):
    """a cached second stream per device (independent branches of a step: the reverse direction of a BLSTM layer)"""
    key = (str(device), i)
    st = _side_streams.get(key)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _side_streams[key] = st
    return st


def h2d_async(t_cpu, device):
    """small host tensor -> device without making the host wait for the stream: a copy from PAGEABLE memory blocks the
    host until everything queued before it has run (a whole training step behind a graph replay); from a pinned
    staging copy it is just enqueued (the caching host allocator keeps the staging block until the copy has run)"""
    if not t_cpu.is_cuda and torch.device(device).type == "cuda":
        return t_cpu.contiguous().pin_memory().to(device, non_blocking=True)
    return t_cpu.to(device)


def gru_cell_fwd(gx, gh, h_prev, live, h, y, acts):
    B, H3 = gx.shape
    H = H3 // 3
    assert gh.numel() == B * H3 and h_prev.numel() == B * H and h.numel() == B * H and acts.numel() == B * 4 * H
    check(_lib.lib().eamd_gru_cell_fwd(ptr(gx), ptr(gh), ptr(h_prev), ptr(live), ptr(h), ptr(y), ptr(acts), B, H,
                                       stream_ptr()), "eamd_gru_cell_fwd")


def gru_cell_bwd(dy, dh, acts, h_prev, live, dgx, dgh, dh_direct):
    B, H4 = acts.shape
    H = H4 // 4
    assert dgx.numel() == B * 3 * H and dgh.numel() == B * 3 * H and dh_direct.numel() == B * H
    check(_lib.lib().eamd_gru_cell_bwd(ptr(dy), ptr(dh), ptr(acts), ptr(h_prev), ptr(live), ptr(dgx), ptr(dgh),
                                       ptr(dh_direct), B, H, stream_ptr()), "eamd_gru_cell_bwd")


# ---- feature-side layers --------------------------------------------------------------------------
def specaug(x, lens=None, center=None, warped=None, fpos=None, flen=None, tpos=None, tlen=None):
    """x [B,T,F] fp32 -> augmented copy; all parameter arrays are int32 device tensors (see include/espnet_amd.h)"""
    B, T, F = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    y = torch.empty_like(x)
    nf = fpos.shape[1] if fpos is not None else 0
    nt = tpos.shape[1] if tpos is not None else 0
    check(_lib.lib().eamd_specaug(ptr(x), ptr(y), ptr(lens), ptr(center), ptr(warped), ptr(fpos), ptr(flen), nf, ptr(tpos),
                                  ptr(tlen), nt, B, T, F, stream_ptr()), "eamd_specaug")
    return y


def global_mvn(x, lens, mean, std):
    B, T, F = x.shape
    y = torch.empty_like(x)
    check(_lib.lib().eamd_global_mvn(ptr(x), ptr(y), ptr(lens), ptr(mean), ptr(std), B, T, F, stream_ptr()), "eamd_global_mvn")
    return y


def utterance_mvn(x, lens, norm_means, norm_vars, eps):
    B, T, F = x.shape
    y = torch.empty_like(x)
    ws = torch.empty(2 * B * F, device=x.device, dtype=torch.float32)
    check(_lib.lib().eamd_utterance_mvn(ptr(x), ptr(y), ptr(lens), ptr(ws), int(norm_means), int(norm_vars), eps,
                                        B, T, F, stream_ptr()), "eamd_utterance_mvn")
    return y


def reflect_pad(x, pad, ldy, tail):
    """x [B, L] fp32 -> flat buffer of B rows of stride ldy (+ `tail` zero floats): reflect padding by `pad` on both
    sides of every row (torch.stft center=True), zeros up to ldy"""
    B, L = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and ldy >= L + 2 * pad
    y = torch.zeros(B * ldy + tail, device=x.device, dtype=torch.float32)
    check(_lib.lib().eamd_reflect_pad(ptr(x), L, ptr(y), ldy, B, L, pad, stream_ptr()),
          "eamd_reflect_pad")
    return y


def logmel(spec, ld, rows_per_utt, melmat, lo, hi, flens, B, T, F, log_scale=1.0, power_input=False):
    """-> [B, T, M] log-mel features (see include/espnet_amd.h: eamd_logmel)"""
    M = melmat.shape[1]
    assert melmat.shape[0] == F and melmat.is_contiguous() and lo.dtype == torch.int32 and hi.dtype == torch.int32
    need = ((B - 1) * rows_per_utt + T - 1) * ld + (F if power_input else 2 * F)
    if spec.numel() < need:
        raise _lib.EamdError(f"logmel: spectrum buffer too small ({spec.numel()} < {need})")
    out = torch.empty(B, T, M, device=spec.device, dtype=torch.float32)
    check(_lib.lib().eamd_logmel(ptr(spec), ld, rows_per_utt, ptr(melmat), ptr(lo), ptr(hi),
                                 ptr(flens) if flens is not None else None, ptr(out), B, T, F, M, log_scale,
                                 int(power_input), stream_ptr()), "eamd_logmel")
    return out


# ---- espnet1 feature transform (csrc/feature_transform.hip; see include/espnet_amd.h) ---------------------------------
def _ft_f32(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.EamdError("feature-transform kernels take contiguous float32 tensors")


def _ft_out(out, shape, device):
    if out is None:
        return torch.empty(shape, device=device, dtype=torch.float32)
    assert tuple(out.shape) == tuple(shape)
    _ft_f32(out)
    return out


def ft_logmel_fwd(spec, melmat, lo, hi, lens, out=None):
    """spec [B,T,F,2], melmat [F,M], lo/hi [M] int32, lens [B] int32 -> log(|spec|^2 melmat + 1e-20) [B,T,M], padded frames 0"""
    B, T, F, two = spec.shape
    M = melmat.shape[1]
    assert two == 2 and melmat.shape[0] == F and lo.numel() == M and hi.numel() == M and lens.numel() == B
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32 and lens.dtype == torch.int32
    _ft_f32(spec, melmat)
    out = _ft_out(out, (B, T, M), spec.device)
    check(_lib.lib().eamd_ft_logmel_fwd(ptr(spec), ptr(melmat), ptr(lo), ptr(hi), ptr(lens), ptr(out), B, T, F, M,
                                        stream_ptr()), "eamd_ft_logmel_fwd")
    return out


def ft_logmel_bwd(spec, g, melmat, lo, hi, mlo, mhi, lens, out=None):
    """gradient of ft_logmel_fwd with respect to spec: [B,T,F,2]; mlo/mhi [F] int32 = the filters that cover each bin"""
    B, T, F, two = spec.shape
    M = melmat.shape[1]
    assert two == 2 and g.shape == (B, T, M) and melmat.shape[0] == F and mlo.numel() == F and mhi.numel() == F
    assert all(t.dtype == torch.int32 for t in (lo, hi, mlo, mhi, lens)) and lo.numel() == M and hi.numel() == M
    _ft_f32(spec, g, melmat)
    gspec = _ft_out(out, spec.shape, spec.device)
    check(_lib.lib().eamd_ft_logmel_bwd(ptr(spec), ptr(g), ptr(melmat), ptr(lo), ptr(hi), ptr(mlo), ptr(mhi), ptr(lens),
                                        ptr(gspec), B, T, F, M, stream_ptr()), "eamd_ft_logmel_bwd")
    return gspec


def ft_mvn_fwd(x, lens, bias=None, scale=None, apply_utt=True, norm_means=True, norm_vars=False, eps=1e-20, out=None):
    """x [B,T,M] -> GlobalMVN (bias, scale given) then utterance_mvn (apply_utt) of the espnet1 feature transform"""
    B, T, M = x.shape
    _ft_f32(x, bias, scale)
    assert lens is None or (lens.dtype == torch.int32 and lens.numel() == B)
    y = _ft_out(out, x.shape, x.device)
    ws = torch.empty(2 * B * M, device=x.device, dtype=torch.float32) if apply_utt else None
    check(_lib.lib().eamd_ft_mvn_fwd(ptr(x), ptr(y), ptr(lens), ptr(bias), ptr(scale), ptr(ws), bool(apply_utt),
                                     bool(norm_means), bool(norm_vars), eps, B, T, M, stream_ptr()),
          "eamd_ft_mvn_fwd")
    return y


def ft_mvn_bwd(gy, lens, scale=None, apply_utt=True, out=None):
    """gradient of ft_mvn_fwd(norm_vars=False) with respect to x"""
    B, T, M = gy.shape
    _ft_f32(gy, scale)
    assert lens is None or (lens.dtype == torch.int32 and lens.numel() == B)
    gx = _ft_out(out, gy.shape, gy.device)
    ws = torch.empty(B * M, device=gy.device, dtype=torch.float32) if apply_utt else None
    check(_lib.lib().eamd_ft_mvn_bwd(ptr(gy), ptr(gx), ptr(lens), ptr(scale), ptr(ws), bool(apply_utt), B, T, M,
                                     stream_ptr()), "eamd_ft_mvn_bwd")
    return gx


def unfold1d(x, B, T, Cc, k):
    """x [B*T, C] (fp32 / bf16) -> col [B*T, k*C]: rows t-(k-1)/2 .. t+(k-1)/2 of the same sequence side by side"""
    assert x.numel() == B * T * Cc and x.is_contiguous() and x.dtype in (torch.float32, torch.bfloat16)
    col = torch.empty(B * T, k * Cc, device=x.device, dtype=x.dtype)
    check(_lib.lib().eamd_unfold1d(ptr(x), ptr(col), B, T, Cc, k, 1 if x.dtype == torch.bfloat16 else 0, stream_ptr()),
          "eamd_unfold1d")
    return col


def fold1d(dcol, B, T, Cc, k):
    """adjoint of unfold1d on fp32: dcol [B*T, k*C] -> dx [B*T, C]"""
    assert dcol.numel() == B * T * k * Cc and dcol.dtype == torch.float32 and dcol.is_contiguous()
    dx = torch.empty(B * T, Cc, device=dcol.device, dtype=torch.float32)
    check(_lib.lib().eamd_fold1d(ptr(dcol), ptr(dx), B, T, Cc, k, stream_ptr()), "eamd_fold1d")
    return dx


# ---- speech enhancement training (csrc/enh.hip; see include/espnet_amd.h) ----------------------------------------------
ENH_ACTS = {"sigmoid": 0, "relu": 1, "tanh": 2, "none": 3}
ENH_MASK, ENH_MAG, ENH_SPEC, ENH_REAL = 0, 1, 2, 3
ENH_LABELS = {"IBM": 0, "IRM": 1, "IAM": 2, "PSM": 3, "NPSM": 4, "PSM^2": 5}
ENH_SNR_ZEROMEAN, ENH_SNR_L2NORM = 0, 1
ENH_CHUNK = 4096             # elements of one utterance per workgroup of the reduction kernels
ENH_MAX_SPK = 3
ISTFT_MAX_OVERLAP = 16


def _enh_f32(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.EamdError("enhancement kernels take contiguous float32 tensors, complex as a trailing (re, im) axis")


def _enh_out(out, shape, device, dtype=torch.float32):
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    assert tuple(out.shape) == tuple(shape) and out.dtype == dtype and out.is_contiguous(), (tuple(out.shape), tuple(shape))
    return out


_istft_env_seen = {}


def istft_check(window, T, n_fft, hop, center, length):
    """the limits of the overlap-add kernel, and torch.istft's check of the window envelope over the written range, on the
    host (the envelope depends on the window and the shape alone) -> the number of samples written before the zeros"""
    if hop < 1 or n_fft > ISTFT_MAX_OVERLAP * hop:
        raise _lib.EamdError(f"istft: n_fft / hop_length = {n_fft}/{hop} > {ISTFT_MAX_OVERLAP} overlapping frames "
                             f"(code {_lib.EAMD_EUNSUPPORTED})")
    import numpy as np
    w = np.asarray(window, dtype=np.float64)
    assert w.shape == (n_fft,)
    full = hop * (T - 1) + n_fft
    start = n_fft // 2 if center else 0
    end = min(start + length, full)
    if end <= start:
        raise ValueError(f"istft: no sample to write (T={T}, n_fft={n_fft}, hop={hop}, length={length})")
    key = (w.tobytes(), T, hop, start, end)
    if key not in _istft_env_seen:
        env = np.zeros(full)
        for t in range(T):
            env[t * hop:t * hop + n_fft] += w * w
        if len(_istft_env_seen) > 64:
            _istft_env_seen.clear()
        _istft_env_seen[key] = float(np.abs(env[start:end]).min())
    if not _istft_env_seen[key] > 1e-11:                      # torch.istft: "window overlap add min: 1"
        raise RuntimeError("istft(n_fft=%d, hop_length=%d): window overlap add min: %g" % (n_fft, hop, _istft_env_seen[key]))
    return end - start


def istft_ola(frames, window, hop, center, length, out=None):
    """frames [B,T,n_fft], synthesis window [n_fft] -> wav [B,length] (eamd_istft_ola); the caller has run istft_check"""
    B, T, N = frames.shape
    _enh_f32(frames, window)
    assert window.shape == (N,)
    wav = _enh_out(out, (B, length), frames.device)
    check(_lib.lib().eamd_istft_ola(ptr(frames), ptr(window), ptr(wav), B, T, N, hop, int(bool(center)), length, stream_ptr()),
          "eamd_istft_ola")
    return wav


def istft_rows(T, n_fft, hop):
    """rows of `hop` samples per utterance of the backward's buffer"""
    return T - 1 + -(-n_fft // hop)


def istft_ola_bwd(dwav, window, T, hop, center, out=None):
    """dwav [B,length] -> g, flat [B * istft_rows * hop + n_fft] (eamd_istft_ola_bwd)"""
    B, length = dwav.shape
    N = window.numel()
    _enh_f32(dwav, window)
    rpu = istft_rows(T, N, hop)
    g = _enh_out(out, (B * rpu * hop + N,), dwav.device)
    check(_lib.lib().eamd_istft_ola_bwd(ptr(dwav), ptr(window), ptr(g), B, T, N, hop, int(bool(center)), length, rpu,
                                        stream_ptr()), "eamd_istft_ola_bwd")
    return g


class IstftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, inv_basis, bwd_basis, window, hop, center, length):
        B, T, F, _ = spec.shape
        N, F2 = inv_basis.shape
        frames = torch.empty(B * T, N, device=spec.device, dtype=torch.float32)
        gemm(spec, inv_basis, frames, B * T, N, F2, F2, F2, N, precision=0)
        ctx.save_for_backward(bwd_basis, window)
        ctx.dims = (B, T, F, hop, center)
        return istft_ola(frames.view(B, T, N), window, hop, center, length)

    @staticmethod
    def backward(ctx, dwav):
        bwd_basis, window = ctx.saved_tensors
        B, T, F, hop, center = ctx.dims
        N = window.numel()
        rpu = istft_rows(T, N, hop)
        g = istft_ola_bwd(dwav.contiguous(), window, T, hop, center)
        out = torch.empty(B * rpu, 2 * F, device=dwav.device, dtype=torch.float32)
        # g is read in place as overlapping rows (leading dimension hop), as Stft.spectrum reads the padded waveform
        gemm(g, bwd_basis, out, B * rpu, 2 * F, N, hop, N, 2 * F, precision=0)
        return out.view(B, rpu, F, 2)[:, :T].contiguous(), None, None, None, None, None, None


def istft(spec, inv_basis, bwd_basis, window, hop, center=True, length=None, window_host=None):
    """spec [B,T,F,2] -> wav [B,length], differentiable in spec.  inv_basis [n_fft, 2F]: the inverse DFT of one frame,
    frames = spec @ inv_basis^T (espnet2.frontend.Stft.inverse_basis); bwd_basis [2F, n_fft]: its transpose with the
    synthesis window folded in (both in the [N, K] layout of eamd_gemm's right operand);
    window [n_fft]: the synthesis window, on the device (window_host: the same on the host, which saves the envelope check a
    copy back).  length None: every sample the frames cover (less the centre
    padding).  One GEMM and one overlap-add kernel; backward one kernel and one GEMM."""
    B, T, F, two = spec.shape
    N, F2 = inv_basis.shape
    assert two == 2 and F2 == 2 * F and bwd_basis.shape == (F2, N) and window.shape == (N,)
    _enh_f32(spec, inv_basis, bwd_basis, window)
    if length is None:
        length = hop * (T - 1) + N - (2 * (N // 2) if center else 0)
    istft_check(window.cpu().numpy() if window_host is None else window_host, T, N, hop, center, int(length))
    return IstftFn.apply(spec, inv_basis, bwd_basis, window, hop, bool(center), int(length))


def enh_mask_apply(logits, X, act, want_mask=True, want_spec=True, out=None):
    """logits [S, ...], X [..., 2] or None -> (mask [S, ...] = act(logits) or None, P [S, ..., 2] or None) (eamd_enh_mask_apply)"""
    S = logits.shape[0]
    Bn = logits[0].numel()
    _enh_f32(logits, X)
    want_spec = want_spec and X is not None
    assert X is None or tuple(X.shape) == tuple(logits.shape[1:]) + (2,)
    mask, P = out if out is not None else (None, None)
    mask = _enh_out(mask, logits.shape, logits.device) if want_mask else None
    P = _enh_out(P, tuple(logits.shape) + (2,), logits.device) if want_spec else None
    check(_lib.lib().eamd_enh_mask_apply(ptr(logits), ptr(X), ptr(mask), ptr(P), S, Bn, act, stream_ptr()), "eamd_enh_mask_apply")
    return mask, P


def enh_mask_apply_bwd(logits, X, gmask, gP, act, out=None):
    """-> dlogits [S, ...] (eamd_enh_mask_apply_bwd); gmask or gP may be None"""
    S = logits.shape[0]
    Bn = logits[0].numel()
    _enh_f32(logits, X, gmask, gP)
    dl = _enh_out(out, logits.shape, logits.device)
    check(_lib.lib().eamd_enh_mask_apply_bwd(ptr(logits), ptr(X), ptr(gmask), ptr(gP), ptr(dl), S, Bn, act, stream_ptr()),
          "eamd_enh_mask_apply_bwd")
    return dl


class EnhMaskFn(torch.autograd.Function):
    """(logits [S, ...], X [..., 2] or None) -> (act(logits), X act(logits) |X| / (|X| + 10e-12) or None); X is data"""

    @staticmethod
    def forward(ctx, logits, X, act, want_spec):
        ctx.set_materialize_grads(False)
        logits = logits.contiguous()
        mask, P = enh_mask_apply(logits, X, act, True, want_spec)
        ctx.save_for_backward(logits, X)
        ctx.act = act
        return mask, P

    @staticmethod
    def backward(ctx, gmask, gP):
        logits, X = ctx.saved_tensors
        if gmask is None and gP is None:
            return None, None, None, None
        gmask = None if gmask is None else gmask.contiguous()
        gP = None if gP is None else gP.contiguous()
        return enh_mask_apply_bwd(logits, X, gmask, gP, ctx.act), None, None, None


def enh_nchunk(n):
    return -(-n // ENH_CHUNK)


def enh_check_spk(S):
    if not 1 <= S <= ENH_MAX_SPK:
        raise _lib.EamdError(f"the permutation kernels take 1 to {ENH_MAX_SPK} speakers, not {S} (code {_lib.EAMD_EUNSUPPORTED})")


def enh_pair_tf(est, ref, mix, mode, label=0, act=3, out=None):
    """pair [B,S,S] float64: pair[b,s,t] = mean squared error of (reference s, estimate t) over the inner extent (eamd_enh_pair_tf).
    mode ENH_MASK: est [S,B,...] real (act is applied), ref [S,B,...,2] and mix [B,...,2] spectra, the reference is the
    ideal-mask label `label`; ENH_MAG / ENH_SPEC: est, ref [S,B,...,2]; ENH_REAL: est, ref [S,B,...]"""
    S, B = est.shape[:2]
    enh_check_spk(S)
    cplx = mode in (ENH_MAG, ENH_SPEC)
    n = est[0, 0].numel() // (2 if cplx else 1)
    _enh_f32(est, ref, mix)
    assert ref.numel() == S * B * n * (1 if mode == ENH_REAL else 2), (tuple(est.shape), tuple(ref.shape))
    assert mode != ENH_MASK or (mix is not None and mix.numel() == B * n * 2)
    nchunk = enh_nchunk(n)
    pair = _enh_out(out, (B, S, S), est.device, torch.float64)
    ws = torch.empty(B * nchunk * S * S, device=est.device, dtype=torch.float64)
    check(_lib.lib().eamd_enh_pair_tf(ptr(est), ptr(ref), ptr(mix), ptr(pair), ptr(ws), S, B, n, nchunk, mode, label, act,
                                      stream_ptr()), "eamd_enh_pair_tf")
    return pair


def enh_pair_tf_bwd(est, ref, mix, perm_index, cot, mode, label=0, act=3, out=None):
    """the gradient of the estimate under the permutations perm_index [B] int64, cot [B] the cotangent of the loss per
    utterance (eamd_enh_pair_tf_bwd)"""
    S, B = est.shape[:2]
    enh_check_spk(S)
    n = est[0, 0].numel() // (2 if mode in (ENH_MAG, ENH_SPEC) else 1)
    _enh_f32(est, ref, mix, cot)
    assert perm_index.dtype == torch.int64 and perm_index.numel() == B and cot.numel() == B and perm_index.is_contiguous()
    dest = _enh_out(out, est.shape, est.device)
    check(_lib.lib().eamd_enh_pair_tf_bwd(ptr(est), ptr(ref), ptr(mix), ptr(perm_index), ptr(cot), ptr(dest), S, B, n, mode,
                                          label, act, stream_ptr()), "eamd_enh_pair_tf_bwd")
    return dest


def enh_pair_sisnr(est, ref, mode=ENH_SNR_ZEROMEAN, out=None):
    """est, ref [S,B,L] -> (pair [B,S,S] float64, sums [B, 4S + S^2] float64, kept for the backward) (eamd_enh_pair_sisnr)"""
    S, B, L = est.shape
    enh_check_spk(S)
    assert ref.shape == est.shape
    _enh_f32(est, ref)
    NV = 4 * S + S * S
    nchunk = enh_nchunk(L)
    pair, sums = out if out is not None else (None, None)
    pair = _enh_out(pair, (B, S, S), est.device, torch.float64)
    sums = _enh_out(sums, (B, NV), est.device, torch.float64)
    ws = torch.empty(B * nchunk * NV, device=est.device, dtype=torch.float64)
    check(_lib.lib().eamd_enh_pair_sisnr(ptr(est), ptr(ref), ptr(pair), ptr(sums), ptr(ws), S, B, L, nchunk, mode, stream_ptr()),
          "eamd_enh_pair_sisnr")
    return pair, sums


def enh_pair_sisnr_bwd(est, ref, sums, perm_index, cot, mode=ENH_SNR_ZEROMEAN, out=None):
    """-> d est [S,B,L] = a est_t + b ref_s + c per (b, t) (eamd_enh_pair_sisnr_bwd)"""
    S, B, L = est.shape
    enh_check_spk(S)
    _enh_f32(est, ref, cot)
    assert sums.dtype == torch.float64 and sums.shape == (B, 4 * S + S * S) and sums.is_contiguous()
    assert perm_index.dtype == torch.int64 and perm_index.numel() == B and cot.numel() == B and perm_index.is_contiguous()
    dest = _enh_out(out, est.shape, est.device)
    check(_lib.lib().eamd_enh_pair_sisnr_bwd(ptr(est), ptr(ref), ptr(sums), ptr(perm_index), ptr(cot), ptr(dest), S, B, L, mode,
                                             stream_ptr()), "eamd_enh_pair_sisnr_bwd")
    return dest


def enh_pit_pick(pair, forced=None, out=None):
    """pair [B,S,S] float64 -> (loss [B] float32, perm_index [B] int64): the best permutation in itertools order, or `forced` [B] int64
    (eamd_enh_pit_pick).  Nothing visits the host."""
    B, S, S2 = pair.shape
    assert S == S2
    enh_check_spk(S)
    assert pair.dtype == torch.float64 and pair.is_contiguous()
    assert forced is None or (forced.dtype == torch.int64 and forced.numel() == B and forced.is_contiguous() and forced.is_cuda)
    loss, perm = out if out is not None else (None, None)
    loss = _enh_out(loss, (B,), pair.device)
    perm = _enh_out(perm, (B,), pair.device, torch.int64)
    check(_lib.lib().eamd_enh_pit_pick(ptr(pair), ptr(forced), ptr(loss), ptr(perm), B, S, stream_ptr()), "eamd_enh_pit_pick")
    return loss, perm


class EnhTFLossFn(torch.autograd.Function):
    """(est, ref, mix) -> (loss [B] under the best or the forced permutation, perm_index [B]); gradient to est only"""

    @staticmethod
    def forward(ctx, est, ref, mix, mode, label, act, forced):
        est = est.contiguous()
        loss, perm = enh_pit_pick(enh_pair_tf(est, ref, mix, mode, label, act), forced)
        ctx.save_for_backward(est, ref, mix, perm)
        ctx.conf = (mode, label, act)
        ctx.mark_non_differentiable(perm)
        return loss, perm

    @staticmethod
    def backward(ctx, gloss, _gperm):
        est, ref, mix, perm = ctx.saved_tensors
        mode, label, act = ctx.conf
        return enh_pair_tf_bwd(est, ref, mix, perm, gloss.contiguous(), mode, label, act), None, None, None, None, None, None


class EnhSisnrLossFn(torch.autograd.Function):
    """(est [S,B,L], ref [S,B,L]) -> (loss [B], perm_index [B]); gradient to est only"""

    @staticmethod
    def forward(ctx, est, ref, mode, forced):
        est = est.contiguous()
        pair, sums = enh_pair_sisnr(est, ref, mode)
        loss, perm = enh_pit_pick(pair, forced)
        ctx.save_for_backward(est, ref, sums, perm)
        ctx.mode = mode
        ctx.mark_non_differentiable(perm)
        return loss, perm

    @staticmethod
    def backward(ctx, gloss, _gperm):
        est, ref, sums, perm = ctx.saved_tensors
        return enh_pair_sisnr_bwd(est, ref, sums, perm, gloss.contiguous(), ctx.mode), None, None, None
