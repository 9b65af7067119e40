"""CPU-side checks of the C-ABI boundary: the library builds, loads, and exports exactly the entry
points include/espnet_amd.h declares (no kernels are launched here)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "include", "espnet_amd.h")
LIB = os.path.join(ROOT, "espnet_amd", "csrc", "libespnet_amd_hip.so")


def declared_symbols():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(eamd_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.dirname(LIB), "-j4"])
    return ctypes.CDLL(LIB)


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert "eamd_gemm" in syms and "eamd_ctc_loss" in syms and len(syms) >= 35


def test_library_exports_every_declared_symbol(lib):
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing


def test_python_binding_lists_every_symbol():
    from espnet_amd import _lib
    assert sorted(_lib.SYMBOLS) == declared_symbols()


def test_abi_version(lib):
    assert lib.eamd_abi_version() == 1


def test_bad_arguments_are_rejected_without_a_gpu(lib):
    # NULL operands must be refused on the host (negative code), never launched
    assert lib.eamd_gemm(None, None) < 0
    lib.eamd_ctc_workspace_bytes.restype = ctypes.c_int64
    assert lib.eamd_ctc_workspace_bytes(2, 10, 3) > 0
    assert lib.eamd_layernorm_fwd(None, None, None, None, None, None, None, 4, 8, ctypes.c_float(1e-12), None) < 0


_ATTN_FWD = ("qu ldq qv ldqv k ldk v ldv pos ldpos mask mb mi P ldp ctx ldc B H T1 T2 dk scale Pd drop_p drop_step drop_salt "
             "shift_len stream").split()
_ATTN_BWD = "dctx ldd k ldk v ldv P ldp dS dbd dq ldo dq_is_bf16 B H T1 T2 dk scale drop_p drop_step drop_salt shift_len stream".split()
_ATTN_ENTRY = {"eamd_attn_fwd": _ATTN_FWD, "eamd_attn_fwd_f32": _ATTN_FWD, "eamd_attn_bwd_q": _ATTN_BWD,
               "eamd_attn_bwd_q_f32": [n for n in _ATTN_BWD if n != "dq_is_bf16"]}
_EINVAL, _EUNSUP = -1, -2
# (what is wrong, the arguments changed from a well-formed relative-position call, the code, forward only?).  Every row is refused
# on the host, before anything is launched: the pointers are made-up addresses, so no row may be a valid call.
_ATTN_ROWS = [
    ("null operand", dict(k=None), _EINVAL, False),
    ("dk != 64", dict(dk=32), _EUNSUP, False),
    ("pos without qv", dict(qv=None), _EINVAL, True),
    ("T1 != T2 with positions", dict(T1=90), _EUNSUP, False),
    ("leading dimension off its unit (a multiple of 2)", dict(ldk=258), _EUNSUP, False),
    ("misaligned pointer", dict(v=0x30008), _EUNSUP, False),
    ("ldp < T2", dict(ldp=96), _EUNSUP, False),
    ("T2 > 4096", dict(T1=4104, T2=4104, ldp=4104), _EUNSUP, False),
    ("drop_p out of range", dict(drop_p=1.0), _EINVAL, False),
    ("drop_p > 0 without Pd", dict(drop_p=0.1, drop_step=0x90000), _EINVAL, True),
    ("drop_p > 0 without the step counter", dict(drop_p=0.1), _EINVAL, False),
]


def test_attention_entry_points_reject_bad_arguments_without_a_gpu():
    """the argument checks of the four query-side attention entry points (one forward and one backward check in
    csrc/attn_common.h, parameterised by the 16-byte unit: 4 fp32 / 8 bf16 elements) keep the code of every combination"""
    from espnet_amd import _lib
    L = _lib.lib()
    good = dict(qu=0x10000, qv=0x20000, k=0x30000, v=0x40000, pos=0x50000, mask=None, mb=0, mi=0, P=0x60000, ctx=0x70000,
                dctx=0x10000, dS=0x20000, dbd=0x50000, dq=0x70000, dq_is_bf16=0, ldq=256, ldqv=256, ldk=256, ldv=256, ldpos=256,
                ldc=256, ldd=256, ldo=256, ldp=104, B=2, H=4, T1=100, T2=100, dk=64, scale=0.125, Pd=None, drop_p=0.0,
                drop_step=None, drop_salt=0, shift_len=None, stream=None)
    for name, params in _ATTN_ENTRY.items():
        forward = "fwd" in name
        for what, change, code, forward_only in _ATTN_ROWS:
            if forward_only and not forward:
                continue
            assert set(change) <= set(params), (name, what)
            args = dict(good, **change)
            if forward and what.endswith("step counter"):
                args["Pd"] = 0xa0000                       # the forward names Pd first
            assert getattr(L, name)(*[args[p] for p in params]) == code, (name, what)
        if not name.endswith("_f32"):                      # the unit is 8 elements for bf16 operands: 260 is a multiple of 4 only
            assert getattr(L, name)(*[dict(good, ldv=260)[p] for p in params]) == _EUNSUP, name


def header_prototypes():
    """(return type, name, parameter list) of every prototype, by a regex of this file's own over the comment-free header"""
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return [(r, n, [] if a.strip() in ("", "void") else a.split(","))
            for r, n, a in re.findall(r"\b(int64_t|int)\s+(eamd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)]


def test_binding_takes_every_prototype_from_the_header():
    from espnet_amd import _lib
    L = _lib.lib()
    protos = header_prototypes()
    assert sorted(n for _, n, _ in protos) == declared_symbols()
    by_value = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
                "double": ctypes.c_double}
    wide = set()
    for ret, name, params in protos:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        for decl, bound in zip(params, fn.argtypes):
            want = ctypes.c_void_p if "*" in decl else by_value[decl.replace("const", "").split()[0]]
            assert bound is want, (name, decl)
        assert fn.restype is (ctypes.c_int64 if ret == "int64_t" else ctypes.c_int), name
        if ret == "int64_t":
            wide.add(name)
    assert {"eamd_rowproj_lnb_workspace", "eamd_decode_src_attn_split_workspace"} <= wide and len(wide) == 14


def test_binding_passes_64_bit_values_whole_and_checks_arguments():
    from espnet_amd import _lib
    L = _lib.lib()
    # int64_t arguments, passed as plain ints: cut to 32 bits, (1 << 32) + 1 rows would be one slab again
    assert L.eamd_bn_nslab(1, 64) == 1
    assert L.eamd_bn_nslab((1 << 32) + 1, 64) > 1
    # int64_t results: about 3.2e9 bytes by the formula in csrc/ctc.hip
    assert L.eamd_ctc_workspace_bytes(64, 4096, 512) > 2 ** 31
    # a plain Python float for a float parameter; NULL operands are still refused on the host
    assert L.eamd_layernorm_fwd(None, None, None, None, None, None, None, 4, 8, 1e-12, None) < 0
    with pytest.raises(TypeError):                       # ten arguments for eleven parameters
        L.eamd_layernorm_fwd(None, None, None, None, None, None, 4, 8, 1e-12, None)
    with pytest.raises((TypeError, ctypes.ArgumentError)):   # a float where the header says int
        L.eamd_layernorm_fwd(None, None, None, None, None, None, None, 4.0, 8, 1e-12, None)
    with pytest.raises((TypeError, ctypes.ArgumentError)):   # a c_int64 where the header says int
        L.eamd_layernorm_fwd(None, None, None, None, None, None, None, ctypes.c_int64(4), 8, 1e-12, None)
    # what the call sites hand to pointer parameters: None, an address, a c_void_p, byref(struct), a ctypes array
    g = _lib.GemmT()
    for p in (None, 0, ctypes.c_void_p(0), ctypes.byref(g), (_lib.GemmT * 2)()):
        assert L.eamd_gemm_multi(p, 0, None) < 0


def test_prototype_parser():
    from espnet_amd import _lib
    got = _lib.parse_prototypes("/* int eamd_not_this(int a); */\n"
                                "typedef struct { int32_t n; } eamd_x_t;\n"
                                "int eamd_a(const float* x, const float* const* rows, int64_t n, uint64_t salt, float p,\n"
                                "           double thr, int32_t k, const eamd_x_t* d, void* stream);\n"
                                "int64_t eamd_b(int rows);\nint eamd_c(void);\n")
    vp = ctypes.c_void_p
    assert got == {"eamd_a": (ctypes.c_int, [vp, vp, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double,
                                             ctypes.c_int, vp, vp]),
                   "eamd_b": (ctypes.c_int64, [ctypes.c_int]), "eamd_c": (ctypes.c_int, [])}
    with pytest.raises(_lib.EamdError, match="eamd_d"):
        _lib.parse_prototypes("int eamd_d(const float* x, size_t n, void* stream);")
    with pytest.raises(_lib.EamdError, match="eamd_e"):
        _lib.parse_prototypes("size_t eamd_e(int n);")


def test_only_the_binding_sets_prototypes_and_only_ops_calls_the_library():
    pkg = os.path.join(ROOT, "espnet_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith(".py"):
                continue
            src = open(os.path.join(dirpath, f)).read()
            if f == "_lib.py":
                assert len(re.findall(r"\.restype\s*=", src)) == 1
            elif f != "graphs.py":                                     # graphs.py binds the HIP runtime, not this library
                assert "restype" not in src, f
            if f not in ("ops.py", "_lib.py"):
                assert not re.search(r"\.eamd_\w+\(", src), f
    assert not re.search(r"\bc_(int64|uint64|float|double)\(", open(os.path.join(pkg, "ops.py")).read())


def test_struct_layout_matches_header():
    from espnet_amd._lib import GatherT, GemmT, RowMapT
    assert ctypes.sizeof(GatherT) == 4 * 27
    assert ctypes.sizeof(RowMapT) == 4 * 9
    assert ctypes.sizeof(GemmT) == 472          # sizeof(eamd_gemm_t) as a C compiler lays out include/espnet_amd.h


def test_round3_struct_layouts_and_null_arguments():
    """eamd_ffn_t / eamd_lstm_seq_*_t as ctypes sees them = as the header lays them out; the new entry points reject NULL
    arguments before touching a device"""
    from espnet_amd import _lib
    # 9 pointers, 4 int32, 2 float, u64, float (+pad), u64, pointer, 2 int32; LayerNorm in front: 5 pointers, float, int32;
    # round 4, LayerNorm backward behind eamd_ffn_bwd: 7 pointers, u64, float, int32
    assert ctypes.sizeof(_lib.FfnT) == 136 + 48 + 72
    assert ctypes.sizeof(_lib.RowProjT) == 240 and ctypes.sizeof(_lib.RowProjPackT) == 32       # include/espnet_amd.h: eamd_rowproj_t, eamd_rowproj_pack_t
    assert ctypes.sizeof(_lib.LstmSeqFwdT) == 8 * 8 + 8    # 8 pointers, 2 int32
    assert ctypes.sizeof(_lib.LstmSeqBwdT) == 6 * 8 + 8    # 6 pointers, 2 int32
    lib = _lib.lib()
    assert lib.eamd_lstm_seq_sync_bytes() == 4096
    assert lib.eamd_lstm_seq_fwd(None, 1, 4, 2, 64, None, None) < 0
    assert lib.eamd_lstm_seq_bwd(None, 2, 4, 2, 64, None, None) < 0
    assert lib.eamd_ffn_fwd(None, None) < 0 and lib.eamd_ffn_bwd(None, None) < 0
    assert lib.eamd_ctc_prefix_score_batch(None, None, 1, 1, None, None, None, None, None, None, 1, 1, 1, 0, 1, None) < 0
    # eamd_gemm_multi validates every descriptor before it launches anything: NULL table, n < 1, and a descriptor without operands
    assert lib.eamd_gemm_multi(None, 2, None) < 0
    arr = (_lib.GemmT * 2)()
    assert lib.eamd_gemm_multi(arr, 0, None) < 0 and lib.eamd_gemm_multi(arr, 2, None) < 0


def test_zero_arena_host_logic():
    """ops.zeros: torch.zeros until a step has been measured; then distinct 256-byte aligned slices of one fresh buffer per
    begin (slices of an earlier step keep their own storage), torch.zeros again beyond the buffer and after zero_arena_off"""
    import torch
    from espnet_amd import ops
    a = ops._zarena
    ops.zero_arena_off()
    a.cap = 0
    ops.zeros(1 << 16, device="cpu")                        # demand outside a training step (an eval forward, a search): not counted
    assert a.need == 0
    ops.zero_arena_begin("cpu")
    assert not a.active
    x, y = ops.zeros(3, 5, device="cpu"), ops.zeros((7,), device="cpu")
    assert x.shape == (3, 5) and y.shape == (7,) and a.need == 512
    ops.zero_arena_begin("cpu")
    assert a.active and a.cap >= 512
    p, q = ops.zeros(3, 5, device="cpu"), ops.zeros((7,), device="cpu")
    assert p.data_ptr() == a.buf.data_ptr() and q.data_ptr() - p.data_ptr() == 256
    p += 1.0
    big = ops.zeros(1 << 20, device="cpu")                  # beyond the buffer: an ordinary allocation
    assert big.data_ptr() < a.buf.data_ptr() or big.data_ptr() >= a.buf.data_ptr() + a.cap
    ops.zero_arena_begin("cpu")
    r = ops.zeros(3, 5, device="cpu")
    assert float(r.sum()) == 0.0 and float(p.sum()) == 15.0 and r.data_ptr() != p.data_ptr()   # the old slice lives on
    ops.zero_arena_off()
    z = ops.zeros(4, device="cpu")
    assert a.buf is None and float(z.sum()) == 0.0 and a.need == 0
    # the arena follows the last step's demand down as well as up
    ops.zero_arena_begin("cpu")
    ops.zeros(1 << 18, device="cpu")
    ops.zero_arena_begin("cpu")
    assert a.cap >= (1 << 20)
    ops.zeros(16, device="cpu")
    ops.zero_arena_begin("cpu")
    assert a.cap == 4096
    ops.zero_arena_off()
    a.cap = 0


def test_product_path_has_no_cpu_fallback():
    import torch
    from espnet_amd import ops, _lib
    x = torch.zeros(4, 8)
    with pytest.raises(_lib.EamdError):
        ops.layernorm_fwd(x, torch.ones(8), torch.zeros(8), 1e-12)


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "espnet_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "oracle" not in open(os.path.join(dirpath, f)).read().replace("# oracle", ""), f
