"""ctypes binding of the espnet_amd C ABI (include/espnet_amd.h).

The product path has no CPU fallback: if the HIP library is missing or a call is made with
tensors that are not on a GPU, this module raises.  torch is used only for device memory and
streams (tensor.data_ptr(), torch.cuda.current_stream()).
"""
import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libespnet_amd_hip.so")


class EamdError(RuntimeError):
    pass


class GatherT(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("C", C.c_int32), ("ntap", C.c_int32), ("Ho", C.c_int32),
                ("Wo", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32), ("sh", C.c_int32),
                ("sw", C.c_int32), ("dh", C.c_int32 * 9), ("dw", C.c_int32 * 9)]


class RowMapT(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("Hc", C.c_int32),
                ("Wc", C.c_int32), ("sh", C.c_int32), ("oh", C.c_int32), ("sw", C.c_int32),
                ("ow", C.c_int32)]


class RowStatsT(C.Structure):
    _fields_ = [("part", C.c_void_p), ("col", C.c_void_p), ("zcol", C.c_void_p), ("zfix", C.c_void_p),
                ("fix", C.c_int32), ("reserved", C.c_int32),
                ("rowc", C.c_void_p), ("gscale", C.c_void_p), ("scale", C.c_float), ("reserved2", C.c_int32)]


class GemmT(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p),
                ("aux", C.c_void_p), ("R", C.c_void_p), ("colsum", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("transA", C.c_int32), ("transB", C.c_int32),
                ("lda", C.c_int64), ("ldb", C.c_int64), ("ldc", C.c_int64), ("ldaux", C.c_int64),
                ("ldr", C.c_int64),
                ("batch1", C.c_int32), ("batch2", C.c_int32),
                ("sA1", C.c_int64), ("sA2", C.c_int64), ("sB1", C.c_int64), ("sB2", C.c_int64),
                ("sC1", C.c_int64), ("sC2", C.c_int64),
                ("alpha", C.c_float), ("beta", C.c_float),
                ("a_act", C.c_int32), ("b_act", C.c_int32), ("epilogue", C.c_int32),
                ("splitk", C.c_int32), ("precision", C.c_int32), ("tile", C.c_int32),
                ("gather", GatherT), ("cmap", RowMapT),
                ("Cb", C.c_void_p), ("in_dtype", C.c_int32), ("aux_dtype", C.c_int32),
                ("drop_p", C.c_float), ("drop_salt", C.c_uint64), ("drop_step", C.c_void_p), ("Hb", C.c_void_p),
                ("h_act", C.c_int32), ("h_dtype", C.c_int32),
                ("stats", RowStatsT)]


class FfnT(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("R", C.c_void_p), ("out", C.c_void_p), ("f", C.c_void_p), ("h", C.c_void_p),
                ("M", C.c_int32), ("D", C.c_int32), ("F", C.c_int32), ("act", C.c_int32),
                ("alpha", C.c_float), ("p_in", C.c_float), ("salt_in", C.c_uint64), ("p_out", C.c_float),
                ("salt_out", C.c_uint64), ("drop_step", C.c_void_p), ("dtype", C.c_int32), ("hsplit", C.c_int32),
                ("ln_x", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("ln_mean", C.c_void_p),
                ("ln_rstd", C.c_void_p), ("ln_eps", C.c_float), ("reserved2", C.c_int32),
                ("lnb_x", C.c_void_p), ("lnb_gamma", C.c_void_p), ("lnb_mean", C.c_void_p), ("lnb_rstd", C.c_void_p),
                ("lnb_dres", C.c_void_p), ("lnb_ws", C.c_void_p), ("lnb_drop_out", C.c_void_p), ("lnb_drop_salt", C.c_uint64),
                ("lnb_drop_p", C.c_float), ("reserved3", C.c_int32)]


class RowProjT(C.Structure):
    _fields_ = [("a", C.c_void_p), ("lda", C.c_int64), ("w", C.c_void_p), ("bias", C.c_void_p), ("R", C.c_void_p),
                ("ldr", C.c_int64), ("out", C.c_void_p), ("ldo", C.c_int64),
                ("M", C.c_int32), ("K", C.c_int32), ("N", C.c_int32), ("a_act", C.c_int32),
                ("alpha", C.c_float), ("p_out", C.c_float), ("salt_out", C.c_uint64), ("drop_step", C.c_void_p),
                ("ln_x", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("ln_mean", C.c_void_p),
                ("ln_rstd", C.c_void_p), ("ln_eps", C.c_float), ("lnb_drop_p", C.c_float),
                ("a_scale", C.c_void_p), ("a_shift", C.c_void_p), ("a_out", C.c_void_p),
                ("lnb_x", C.c_void_p), ("lnb_gamma", C.c_void_p), ("lnb_mean", C.c_void_p), ("lnb_rstd", C.c_void_p),
                ("lnb_dres", C.c_void_p), ("lnb_ws", C.c_void_p), ("lnb_drop_out", C.c_void_p), ("lnb_drop_salt", C.c_uint64)]


class FfnPackT(C.Structure):
    _fields_ = [("w1", C.c_void_p), ("w2", C.c_void_p), ("fwd_first", C.c_void_p), ("fwd_second", C.c_void_p),
                ("bwd_first", C.c_void_p), ("bwd_second", C.c_void_p), ("D", C.c_int32), ("F", C.c_int32)]


class RowProjPackT(C.Structure):
    _fields_ = [("w", C.c_void_p), ("image", C.c_void_p), ("K", C.c_int32), ("N", C.c_int32), ("ldw", C.c_int32),
                ("trans", C.c_int32)]


class LstmSeqFwdT(C.Structure):
    _fields_ = [("gx", C.c_void_p), ("w_hh", C.c_void_p), ("b_hh", C.c_void_p), ("live", C.c_void_p),
                ("h_out", C.c_void_p), ("c_out", C.c_void_p), ("y", C.c_void_p), ("acts", C.c_void_p),
                ("reverse", C.c_int32), ("reserved", C.c_int32)]


class LstmSeqBwdT(C.Structure):
    _fields_ = [("dy", C.c_void_p), ("w_t", C.c_void_p), ("acts", C.c_void_p), ("c_out", C.c_void_p),
                ("live", C.c_void_p), ("dgates", C.c_void_p), ("reverse", C.c_int32), ("reserved", C.c_int32)]


_lib = None

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "espnet_amd.h")
_BY_VALUE = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
             "double": C.c_double}


def parse_prototypes(text):
    """header text -> {name: (restype, [argtypes])} for every `<type> eamd_*(<params>);`.  A parameter with a `*` is a
    c_void_p (it takes None, an address, byref(struct) and ctypes arrays); the by-value types are those of _BY_VALUE, anything
    else is an EamdError naming the prototype (the header is regular: this is not a C parser)."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"\b(\w+)\s+(eamd_\w+)\s*\(([^()]*)\)\s*;", text):
        def ctype(decl, named):
            if "*" in decl:
                return C.c_void_p
            words = [w for w in decl.split() if w != "const"]
            base = " ".join(words[:-1] if named else words)
            if base not in _BY_VALUE:
                raise EamdError(f"{name}: cannot bind by-value type '{base}' of '{decl.strip()}'")
            return _BY_VALUE[base]
        params = [] if params.strip() in ("", "void") else params.split(",")
        protos[name] = (ctype(ret, False), [ctype(p, True) for p in params])
    return protos


with open(HEADER_PATH) as _f:
    PROTOTYPES = parse_prototypes(_f.read())
# every symbol include/espnet_amd.h declares (tests check they are all exported)
SYMBOLS = list(PROTOTYPES)


def lib():
    """Load the HIP shared library (once) and give every entry point the header's prototype: ctypes then converts plain
    Python ints / floats to the declared widths and refuses a wrong argument count or type.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EamdError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C espnet_amd/csrc` (there is no CPU fallback)")
        handle = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(handle, name)  # AttributeError here = header/library mismatch
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr():
    """the current HIP stream of the current device, as an address.  torch.cuda.current_stream() builds a Stream object through
    several Python layers (2.8 us per call, paid by every launch of an eager decode step); the raw getter is one C call"""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


EAMD_EUNSUPPORTED = -2   # include/espnet_amd.h


def check(rc, what):
    if rc != 0:
        raise EamdError(f"{what} failed with code {rc}")


def ptr(t, offset=0):
    """Device address of a tensor (+ element offset) as an int; None -> NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise EamdError("espnet_amd kernels need GPU tensors (no CPU fallback in the product path)")
    if offset == 0:
        return t.data_ptr()
    return t.data_ptr() + offset * t.element_size()


def f32(t):
    if t.dtype != torch.float32:
        raise EamdError(f"expected float32 tensor, got {t.dtype}")
    return t
