"""CPU-side checks of the entry points behind the fused front-end / CTC backward passes: eamd_conv2_bwd_x_conv1_bwd_w,
eamd_ctc_grad and eamd_gemm's column sums of a gathered product's B operand refuse NULL and unsupported arguments on the
host, before anything is launched (no GPU is touched here)."""
import ctypes

import pytest

EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    from espnet_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def mem():
    """host memory whose 16-byte aligned address stands in for device operands: every call below is refused before a launch"""
    buf = ctypes.create_string_buffer(1 << 12)
    return (ctypes.addressof(buf) + 15) & ~15, buf


def dx_class(addr, **over):
    """a descriptor eamd_conv2_bwd_x_conv1_bwd_w accepts (one 1-tap class of a [1, 7, 7] -> [1, 3, 3, 128] conv1 output):
    x W^T with gathered rows, epilogue 3, fp32 aux, the 128 tile"""
    from espnet_amd import _lib
    p = _lib.GemmT()
    p.A = p.B = p.aux = addr
    p.M, p.N, p.K = 4, 128, 128
    p.transB = 1
    p.lda = p.ldb = p.ldc = p.ldaux = p.ldr = 128
    p.batch1 = p.batch2 = 1
    p.alpha, p.beta = 1.0, 0.0
    p.epilogue, p.splitk, p.tile = 3, 1, 128
    g = p.gather
    g.enabled, g.C, g.ntap, g.Ho, g.Wo, g.Hin, g.Win, g.sh, g.sw = 1, 128, 1, 2, 2, 2, 2, 1, 1
    c = p.cmap
    c.enabled, c.Ho, c.Wo, c.Hc, c.Wc, c.sh, c.oh, c.sw, c.ow = 1, 2, 2, 3, 3, 2, 0, 2, 0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def test_fused_conv1_gradient_entry_rejects_bad_arguments(L, mem):
    from espnet_amd import _lib
    addr, _ = mem
    fn = L.eamd_conv2_bwd_x_conv1_bwd_w
    ok = (_lib.GemmT * 1)(dx_class(addr))
    assert fn(None, 1, addr, 7, 7, addr, addr, addr, None) == EINVAL
    assert fn(ok, 0, addr, 7, 7, addr, addr, addr, None) == EINVAL
    assert fn(ok, 5, addr, 7, 7, addr, addr, addr, None) == EINVAL
    for hole in range(4):                                        # x, part, dw, db
        args = [addr] * 4
        args[hole] = None
        assert fn(ok, 1, args[0], 7, 7, args[1], args[2], args[3], None) == EINVAL
    assert fn(ok, 1, addr, 2, 7, addr, addr, addr, None) == EINVAL
    assert fn((_lib.GemmT * 1)(), 1, addr, 7, 7, addr, addr, addr, None) == EINVAL        # a descriptor without operands
    assert fn((_lib.GemmT * 1)(dx_class(addr, aux=None)), 1, addr, 7, 7, addr, addr, addr, None) == EINVAL     # epilogue 3 needs aux
    unsupported = [dict(epilogue=0), dict(epilogue=4), dict(tile=64), dict(precision=1), dict(alpha=2.0), dict(beta=1.0),
                   dict(bias=addr), dict(R=addr), dict(N=64), dict(ldaux=130), dict(aux=addr + 4), dict(M=5)]
    for over in unsupported:
        assert fn((_lib.GemmT * 1)(dx_class(addr, **over)), 1, addr, 7, 7, addr, addr, addr, None) == EUNSUPPORTED, over
    # a row map that is not conv1's output for this (T, F), a class that leaves it, a tap offset beyond 4 bits, no gather
    assert fn(ok, 1, addr, 9, 7, addr, addr, addr, None) == EUNSUPPORTED
    p = dx_class(addr)
    p.cmap.oh = 1
    assert fn((_lib.GemmT * 1)(p), 1, addr, 7, 7, addr, addr, addr, None) == EUNSUPPORTED
    p = dx_class(addr)
    p.gather.dh[0] = -9
    assert fn((_lib.GemmT * 1)(p), 1, addr, 7, 7, addr, addr, addr, None) == EUNSUPPORTED
    p = dx_class(addr)
    p.gather.enabled = 0
    assert fn((_lib.GemmT * 1)(p), 1, addr, 7, 7, addr, addr, addr, None) == EUNSUPPORTED
    p = dx_class(addr)
    p.cmap.enabled = 0
    assert fn((_lib.GemmT * 1)(p), 1, addr, 7, 7, addr, addr, addr, None) == EUNSUPPORTED
    # two classes over different numbers of images
    assert fn((_lib.GemmT * 2)(dx_class(addr), dx_class(addr, M=8)), 2, addr, 7, 7, addr, addr, addr, None) == EUNSUPPORTED


def test_ctc_grad_entry_rejects_bad_arguments(L, mem):
    addr, _ = mem
    fn = L.eamd_ctc_grad

    def call(acts=addr, ilens=addr, nll=addr, grad=addr, ws=addr, B=2, T=5, V=7, Lmax=3, gscale=None):
        return fn(acts, V, T * V, ilens, nll, grad, V, T * V, ws, B, T, V, Lmax, 0, 1.0, gscale, None)
    for hole in ("acts", "ilens", "nll", "grad", "ws"):
        assert call(**{hole: None}) == EINVAL, hole
    assert call(B=0) == EINVAL and call(T=0) == EINVAL and call(V=0) == EINVAL and call(Lmax=-1) == EINVAL
    assert call(V=16385) == EUNSUPPORTED               # the occupancy row must fit in 64 KB of LDS, as in eamd_ctc_loss
    assert call(Lmax=512) == EUNSUPPORTED              # 2 L + 1 lattice states in one workgroup


def test_gemm_column_sums_of_b_need_the_gathered_fp32_weight_gradient(L, mem):
    from espnet_amd import _lib
    addr, _ = mem
    p = _lib.GemmT()
    p.A = p.B = p.C = p.colsum = addr
    p.M, p.N, p.K = 64, 64, 64
    p.transA, p.transB = 0, 1
    p.lda = p.ldb = p.ldc = p.ldaux = p.ldr = 64
    p.batch1 = p.batch2 = 1
    p.alpha, p.splitk, p.tile = 1.0, 1, 64
    g = p.gather
    g.enabled, g.C, g.ntap, g.Ho, g.Wo, g.Hin, g.Win, g.sh, g.sw = 1, 64, 1, 8, 8, 8, 8, 1, 1
    assert L.eamd_gemm(ctypes.byref(p), None) == EUNSUPPORTED           # gathered rows of a non-transposed A
    p.transA, p.transB = 1, 0
    assert L.eamd_gemm(ctypes.byref(p), None) == EUNSUPPORTED           # B must be [K, N]
    p.transB, p.in_dtype, p.precision = 1, 1, 1
    assert L.eamd_gemm(ctypes.byref(p), None) == EUNSUPPORTED           # bf16 operands keep eamd_colsum
    p.in_dtype, p.precision, p.batch2 = 0, 0, 2
    assert L.eamd_gemm(ctypes.byref(p), None) == EUNSUPPORTED


def test_conv_front_end_routes_on_the_host():
    """the fused route is taken by the first 3x3 stage in fp32 mode with whole 128-channel tiles only"""
    import torch
    import espnet_amd
    from espnet_amd import functional as Fn
    y = torch.zeros(4, 128)
    try:
        espnet_amd.set_precision("fp32")
        assert Fn.FUSE_CONV1_WGRAD and Fn._conv1w_fusable(y, 128) and Fn._conv1w_fusable(y, 256)
        assert not Fn._conv1w_fusable(y, 64) and not Fn._conv1w_fusable(y, 192)
        Fn.FUSE_CONV1_WGRAD = False
        assert not Fn._conv1w_fusable(y, 128)
        Fn.FUSE_CONV1_WGRAD = True
        espnet_amd.set_precision("bf16")
        assert not Fn._conv1w_fusable(y.bfloat16(), 128)
    finally:
        Fn.FUSE_CONV1_WGRAD = True
        espnet_amd.set_precision("fp32")
