"""The RNN kernel family (csrc/rnn.hip: LSTM / GRU cells, the one-launch LSTM step, 2x2 max-pool, location-aware attention
forward and its three backward stages, the AttLocRec conv + ReLU + arg-max front end, dot-product energies, softmax +
context) and the persistent whole-sequence LSTM (csrc/lstm_seq.hip), element-wise against float64.

The reference is tests/rnn_restatement.py (checked on the CPU by tests/test_rnn_restatement.py) evaluated in float64 from the
same fp32 input values.  Entry points are called through the C ABI with every output buffer filled with NaN and followed by
8 guard elements that must come back bit-identical; accumulating outputs start from non-zero values and are called twice;
a refused call (EAMD_EINVAL / EAMD_EUNSUPPORTED) must leave every output bit-identical to the fill.  Each case recomputes
the host dispatcher's predicate from the actual addresses and sizes and asserts the branch it is meant to take; misalignment
comes from a 4-byte offset view of a live allocation.

The measured quantity per element is |got - ref| / scale, where scale is the sum of the absolute values of the terms that
form the element (first-order propagated through sigmoid / tanh / softmax with their derivatives), plus 2^-103: a result
flushed or overflowed to zero below the smallest normal fp32 (sigmoid of -100) is one fp32 rounding of that floor.  Every
bound is a named constant, at most 4x the largest value observed under its name on an MI355X (noted beside it); outputs
formed by adds and multiplies alone must also sit under (n_terms + 8) * 2^-24.  Selections, masks, pass-throughs and the
dyadic-grid cases are bit-exact.  Every check prints "[rnn] <CONSTANT> <case>: ..." with the worst element's index."""
import math

import pytest
import torch

import rnn_restatement as rr


pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
INF = float("inf")
U24 = 2.0 ** -24
TINY = 2.0 ** -103
EINVAL, EUNSUPPORTED = -1, -2
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
FILL = {F32: NAN, I32: 0x7FC00000, U8: 0xA5}

# ---- named bounds: |got - ref| / scale; observed = the largest value seen under the name on an MI355X ------------------
GATE_TOL = 5.7e-7         # sigmoid / tanh gate values kept in acts (cells and the one-launch step)         observed 1.45e-7
CELL_FWD_TOL = 7.0e-7     # c, h, y of the LSTM and GRU cells                                              observed 1.75e-7
CELL_BWD_TOL = 8.4e-7     # dgates, dc_prev of the LSTM cell; dgx, dgh, dh_direct of the GRU cell           observed 2.11e-7
STEP_FWD_TOL = 3.5e-7     # c, h, y, acts of the one-launch step (MFMA reduction + cell)                    observed 8.94e-8
STEP_BWD_TOL = 7.3e-7     # dgates, dc_prev of the one-launch backward step                                observed 1.84e-7
STEP_DEAD_TOL = 3.1e-7    # dh_pass = dh_pass_in + dgates_next W_hh on dead rows (adds and multiplies)      observed 7.91e-8
ATT_CONV_TOL = 5.8e-7     # location features conv (adds and multiplies)                                   observed 1.45e-7
ATT_TH_TOL = 6.4e-7       # th = tanh(pre_enc + dec_proj + W_att conv)                                     observed 1.62e-7
ATT_E_TOL = 2.9e-7        # energies e (attloc) and dot energies                                           observed 7.27e-8
ATT_W_TOL = 1.3e-7        # softmax weights w                                                              observed 3.43e-8
ATT_CTX_TOL = 4.7e-8      # context vectors                                                                observed 1.18e-8
ATT_DE_TOL = 5.3e-7       # de of softmax + context backward                                               observed 1.33e-7
ATT_DENC_TOL = 4.7e-7     # d_enc_h / d_v (adds and multiplies)                                            observed 1.18e-7
ATT_DF_TOL = 7.1e-7       # df                                                                             observed 1.78e-7
ATT_DCONV_TOL = 2.8e-7    # dconv of the fused stage (adds and multiplies)                                 observed 7.02e-8
ATT_RED_TOL = 1.1e-6      # dgvec, d_dec_proj, dw_att: sums over frames / utterances onto non-zero values   observed 2.98e-7
ATT_DGB_TOL = 4.4e-7      # |dgb - dgb_before| / sum |de| (the exact gradient is 0)                         observed 1.10e-7
ATT_FUSED_TOL = 1.3e-6    # fused against unfused stage 1, same scales                                     observed 3.32e-7
ATT_DPREV_TOL = 1.8e-7    # d_prev of eamd_attloc_bwd_conv (adds and multiplies)                           observed 4.52e-8
ATT_DCONVW_TOL = 7.7e-7   # dconv_w of eamd_attloc_bwd_conv (atomics onto non-zero values)                 observed 1.94e-7
DOT_DSUM_TOL = 5.4e-8     # |dsum - dsum_before| of softmax + context backward (exactly 0 too), relative to the sum
                          # over the frames of the terms of de, scaling w (|dw| + sum w |dw|)             observed 1.37e-8
DOT_DK_TOL = 2.3e-7       # dk (one product)                                                               observed 5.95e-8
DOT_DQ_TOL = 1.7e-6       # dq (atomics onto non-zero values)                                              observed 4.46e-7
SEQ_FWD_TOL = 4.8e-7      # y, h, c, acts of every step of the persistent LSTM                             observed 1.22e-7
SEQ_BWD_TOL = 9.0e-7      # dgates of every step of the persistent LSTM backward                           observed 2.26e-7

OBSERVED = {}


@pytest.fixture(scope="module")
def ops():
    from espnet_amd import ops as o
    o.set_precision("fp32")
    return o


@pytest.fixture(scope="module")
def lib():
    from espnet_amd import _lib
    _lib.lib()
    yield _lib
    for k in sorted(OBSERVED):
        print(f"[rnn] largest observed under {k}: {OBSERVED[k]:.3e} (constant {globals()[k]:g})")


def apriori(n_terms):
    return (n_terms + 8) * U24


def cdiv(a, b):
    return -(-a // b)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def aligned(nbytes, *ts):
    """every tensor's (view's) address is a multiple of nbytes; None counts as NULL"""
    return all(t is None or t.data_ptr() % nbytes == 0 for t in ts)


def unravel(i, shape):
    idx = []
    for n in reversed(shape):
        idx.insert(0, i % n)
        i //= n
    return tuple(idx)


def ibits(t):
    """the bit patterns of an fp32 tensor (int32 / uint8 as they are), on the CPU"""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32) if t.dtype == F32 else t


class Out:
    """an output of `shape` inside a fill-patterned allocation: `off` elements in front (off = 1: a 4-byte offset view,
    misaligned for 16-byte accesses), 8 guard elements behind"""

    def __init__(self, *shape, dtype=F32, off=0):
        self.n, self.off, self.dtype = math.prod(shape), off, dtype
        self.buf = torch.full((off + self.n + 8,), FILL[dtype], dtype=dtype, device=DEV)
        self.v = self.buf[off:off + self.n].view(*shape)
        self.pat = ibits(torch.full((1,), FILL[dtype], dtype=dtype))[0]

    def guards(self, name):
        b = ibits(self.buf)
        pos = torch.arange(b.numel())
        bad = ((pos < self.off) | (pos >= self.off + self.n)) & (b != self.pat)
        assert not bool(bad.any()), f"{name}: guard element {int(bad.nonzero()[0]) - self.off} was overwritten"

    def untouched(self, name):
        bad = ibits(self.buf) != self.pat
        assert not bool(bad.any()), f"{name}: element {int(bad.nonzero()[0]) - self.off} written by a refused call"


class Acc:
    """an accumulating output: starts from known non-zero values, 8 guard elements behind that must keep theirs"""

    def __init__(self, *shape, seed=0, start=None):
        self.n = math.prod(shape)
        self.start = torch.randn(self.n + 8, generator=gen(1000 + seed)) if start is None else start.reshape(-1).float()
        assert self.start.numel() == self.n + 8
        self.buf = self.start.to(DEV)
        self.v = self.buf[:self.n].view(*shape)
        self.v0 = self.start[:self.n].view(*shape).double()

    def guards(self, name):
        assert_bits(f"{name} guard", self.buf[self.n:], self.start[self.n:])


def assert_bits(name, got, ref):
    """bit equality (fp32 by pattern), with the first differing element's index"""
    g, r = ibits(got).reshape(-1), ibits(ref.to(got.dtype) if ref.dtype != got.dtype else ref).reshape(-1)
    assert g.shape == r.shape, f"{name}: {g.shape} vs {r.shape}"
    bad = g != r
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {g.numel()} elements differ, first at {unravel(i, tuple(ref.shape))}: "
                             f"got 0x{int(g[i]) & 0xffffffff:x}, expected 0x{int(r[i]) & 0xffffffff:x}")


def assert_zero_bits(name, got):
    assert_bits(name, got, torch.zeros(got.shape, dtype=got.dtype))


def check(tolname, name, got, ref, scale, n_terms=None):
    """max over all elements of |got - ref| / scale in float64 with the worst element's index.  Where the reference is
    infinite the result must be the same infinity; a NaN in the result (an unwritten element) is an infinite error.
    n_terms: also assert the a-priori bound of an output formed by adds and multiplies alone."""
    tol = globals()[tolname]
    g = got.detach().double().cpu().reshape(ref.shape)
    r = ref.detach().double()
    assert not bool(torch.isnan(r).any()), f"{name}: the reference has a NaN"
    special = torch.isinf(r)
    if bool(special.any()):
        bad = special & ~(g == r)
        assert not bool(bad.any()), f"{name}: element {unravel(int(bad.reshape(-1).nonzero()[0]), tuple(ref.shape))} is not the reference's infinity"
        g, r = torch.where(special, torch.zeros_like(g), g), torch.where(special, torch.zeros_like(r), r)
    d = (g - r).abs()
    d = torch.where(torch.isfinite(g), d, torch.full_like(d, INF))
    s = scale.detach().double().expand_as(d)
    e = torch.where(d == 0, torch.zeros_like(d), d / s).reshape(-1)
    i = int(e.argmax()) if e.numel() else 0
    worst = float(e[i]) if e.numel() else 0.0
    idx = unravel(i, tuple(ref.shape))
    extra = "" if n_terms is None else f", a-priori {apriori(n_terms):.3g}"
    print(f"[rnn] {tolname} {name}: max err/scale {worst:.3e} at {idx} (tol {tol:g}{extra})")
    OBSERVED[tolname] = max(OBSERVED.get(tolname, 0.0), worst)
    assert worst <= tol, f"{name}: element {idx} error/scale {worst:.3e} > {tolname} = {tol:g}"
    if n_terms is not None:
        assert worst <= apriori(n_terms), f"{name}: {worst:.3e} above the a-priori bound of {n_terms} terms"
    return worst


_KEEP = []


def dev(t):
    """device copy that stays allocated until the test ends (an argument built in the call itself would be freed, and its
    block handed to the next copy, before the launch)"""
    if t is None:
        return None
    _KEEP.append(t.to(DEV))
    return _KEEP[-1]


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    _KEEP.clear()


def sp(lib):
    return lib.stream_ptr()


def live_rows(B):
    """rows 0, B - 1 and one middle row dead"""
    lv = torch.ones(B, dtype=U8)
    lv[0] = 0
    lv[B - 1] = 0
    lv[B // 2] = 0
    return lv


def with_extremes(x, start=1):
    """+-30 and +-100 among the N(0, 1) pre-activations"""
    flat = x.reshape(-1)
    pos = torch.arange(start, flat.numel(), 5)[:24]
    flat[pos] = torch.tensor([30.0, -30.0, 100.0, -100.0]).repeat(6)[:pos.numel()]
    return x


# =============================================================================================
# scales: first-order propagation of the sums of absolute values of the terms
# =============================================================================================
def lstm_fwd_scales(acts, c_prev, c, S=None, s_cprev=None):
    """acts / c: float64 reference values; S [B, 4H]: scale of the gate pre-activations (None: they are exact inputs);
    s_cprev: scale of c_prev (None: an exact input) -> scales of acts [B, 4H], c, h"""
    B, H = c.shape
    i, f, g, o = acts.reshape(B, 4, H).unbind(1)
    if S is None:
        S = torch.zeros(B, 4 * H, dtype=torch.float64)
    Si, Sf, Sg, So = S.reshape(B, 4, H).unbind(1)
    si, sf, sg, so = i + i * (1 - i) * Si, f + f * (1 - f) * Sf, g.abs() + (1 - g * g) * Sg, o + o * (1 - o) * So
    s_c = c_prev.abs() * sf + g.abs() * si + i * sg
    if s_cprev is not None:
        s_c = s_c + f * s_cprev
    tc = torch.tanh(c)
    s_h = tc.abs() * so + o * s_c
    return torch.cat([si, sf, sg, so], dim=1) + TINY, s_c + TINY, s_h + TINY


def lstm_bwd_scales(dy, s_dh, s_dc, acts, c_prev, c):
    """|dy| (None = 0), scales of the arriving dh and dc -> scales of dgates [B, 4H] and dc_prev"""
    B, H = c.shape
    i, f, g, o = acts.reshape(B, 4, H).unbind(1)
    dhv = s_dh + (0 if dy is None else dy.double().abs())
    tc = torch.tanh(c)
    dct = s_dc + dhv * o * (1 + tc * tc)
    s = torch.cat([dct * g.abs() * i * (1 + i), dct * c_prev.abs() * f * (1 + f), dct * i * (1 + g * g),
                   dhv * tc.abs() * o * (1 + o)], dim=1)
    return s + TINY, dct * f + TINY


def assert_zero_value(name, got):
    """== 0 as a value (a product with a zero factor may carry either sign)"""
    bad = got.detach().cpu().reshape(-1) != 0
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} elements are not zero, first at {int(bad.nonzero()[0]) if bool(bad.any()) else -1}"


def zabs(t, like):
    return torch.zeros_like(like) if t is None else t.double().abs()


# =============================================================================================
# a. LSTM and GRU cells
# =============================================================================================
CELL_SHAPES = [(1, 1), (3, 5), (5, 64), (7, 333), (64, 1024)]


@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_lstm_cell_vs_float64(lib, B, H):
    """eamd_lstm_cell_fwd / _bwd: live NULL and given (rows 0, B - 1 and a middle row dead), y NULL and given, backward with
    every accepted combination of NULL dy / dh / dc; pre-activations of +-30 and +-100 among N(0, 1).  The 65535-block cap
    of grid_for needs more than 16.7 M elements and is not reached here."""
    L, p = lib.lib(), lib.ptr
    g = gen(B * 7 + H)
    gates = with_extremes(torch.randn(B, 4 * H, generator=g))
    c_prev, h_prev = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g).tanh()
    gd, cpd, hpd = dev(gates), dev(c_prev), dev(h_prev)
    assert B * H <= 65535 * 256
    for live in (None, live_rows(B)):
        h_ref, c_ref, y_ref, a_ref = rr.lstm_cell_fwd(gates, c_prev, h_prev, live)
        s_a, s_c, s_h = lstm_fwd_scales(a_ref, c_prev.double(), rr.lstm_cell_fwd(gates, c_prev)[1])
        dead = torch.zeros(B, dtype=torch.bool) if live is None else live == 0
        for with_y in (True, False):
            name = f"lstm_cell_fwd {B}x{H} live={live is not None} y={with_y}"
            h, c, y, acts = Out(B, H), Out(B, H), Out(B, H), Out(B, 4 * H)
            rc = L.eamd_lstm_cell_fwd(p(gd), p(cpd), p(hpd), p(dev(live)), p(h.v), p(c.v), p(y.v) if with_y else None,
                                      p(acts.v), B, H, sp(lib))
            assert rc == 0
            assert bool(torch.isfinite(h.v).all()) and bool(torch.isfinite(c.v).all()) and bool(torch.isfinite(acts.v).all())
            check("GATE_TOL", name + " acts", acts.v, a_ref, s_a)
            check("CELL_FWD_TOL", name + " c", c.v, c_ref, torch.where(dead.unsqueeze(1), c_prev.double().abs() + TINY, s_c))
            check("CELL_FWD_TOL", name + " h", h.v, h_ref, torch.where(dead.unsqueeze(1), h_prev.double().abs() + TINY, s_h))
            assert_bits(name + " dead c == c_prev", c.v[dead], c_prev[dead])
            assert_bits(name + " dead h == h_prev", h.v[dead], h_prev[dead])
            if with_y:
                check("CELL_FWD_TOL", name + " y", y.v, y_ref, s_h)
                assert_zero_bits(name + " dead y == +0", y.v[dead])
                y.guards(name)
            else:
                y.untouched(name + " y NULL")
            for o in (h, c, acts):
                o.guards(name)
        # backward from the fp32 values of the forward
        acts32, c32 = a_ref.float(), c_ref.float()
        dy, dh, dc = (torch.randn(B, H, generator=g) for _ in range(3))
        for mask in range(1, 8):
            uy, uh, uc = dy if mask & 1 else None, dh if mask & 2 else None, dc if mask & 4 else None
            name = f"lstm_cell_bwd {B}x{H} live={live is not None} dy={mask & 1} dh={mask >> 1 & 1} dc={mask >> 2}"
            dg_ref, dcp_ref, dhp_ref = rr.lstm_cell_bwd(uy, uh, uc, acts32, c_prev, c32, live)
            s_dg, s_dcp = lstm_bwd_scales(uy, zabs(uh, c_ref), zabs(uc, c_ref), acts32.double(), c_prev.double(), c32.double())
            dgo, dcpo, dhpo = Out(B, 4 * H), Out(B, H), Out(B, H)
            rc = L.eamd_lstm_cell_bwd(p(dev(uy)), p(dev(uh)), p(dev(uc)), p(dev(acts32)), p(cpd), p(dev(c32)), p(dev(live)),
                                      p(dgo.v), p(dcpo.v), p(dhpo.v), B, H, sp(lib))
            assert rc == 0
            check("CELL_BWD_TOL", name + " dgates", dgo.v, dg_ref, s_dg)
            check("CELL_BWD_TOL", name + " dc_prev", dcpo.v, dcp_ref, torch.where(dead.unsqueeze(1), zabs(uc, c_ref) + TINY, s_dcp))
            assert_zero_bits(name + " dead dgates == +0", dgo.v[dead])
            assert_bits(name + " dead dc_prev has the bits of dc", dcpo.v[dead], (dc if uc is not None else torch.zeros(B, H))[dead])
            assert_bits(name + " dead dh_pass has the bits of dh", dhpo.v[dead], (dh if uh is not None else torch.zeros(B, H))[dead])
            assert_zero_bits(name + " live dh_pass == +0", dhpo.v[~dead])
            for o in (dgo, dcpo, dhpo):
                o.guards(name)
    # refusals: nothing to differentiate; live without h_prev / dh_pass
    outs = [Out(B, 4 * H), Out(B, H), Out(B, H), Out(B, H)]
    a32, lv = dev(torch.rand(B, 4 * H, generator=g)), dev(live_rows(B))
    assert L.eamd_lstm_cell_bwd(None, None, None, p(a32), p(cpd), p(cpd), None, p(outs[0].v), p(outs[1].v), p(outs[2].v), B, H, sp(lib)) == EINVAL
    assert L.eamd_lstm_cell_bwd(p(cpd), None, None, p(a32), p(cpd), p(cpd), p(lv), p(outs[0].v), p(outs[1].v), None, B, H, sp(lib)) == EINVAL
    assert L.eamd_lstm_cell_fwd(p(gd), p(cpd), None, p(lv), p(outs[1].v), p(outs[2].v), p(outs[3].v), p(outs[0].v), B, H, sp(lib)) == EINVAL
    for o in outs:
        o.untouched(f"refused lstm_cell {B}x{H}")


def gru_fwd_scales(gx, gh, h_prev, acts):
    B, H = h_prev.shape
    xr, xz, xn = gx.double().abs().reshape(B, 3, H).unbind(1)
    hr, hz, _ = gh.double().abs().reshape(B, 3, H).unbind(1)
    r, z, n, ghn = acts.reshape(B, 4, H).unbind(1)
    sr, sz = r + r * (1 - r) * (xr + hr), z + z * (1 - z) * (xz + hz)
    sn = n.abs() + (1 - n * n) * (xn + sr * ghn.abs())
    s_h = (1 + z) * sn + sz * (n.abs() + h_prev.double().abs())
    return torch.cat([sr, sz, sn, ghn.abs()], dim=1) + TINY, s_h + TINY


@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_gru_cell_vs_float64(lib, B, H):
    """eamd_gru_cell_fwd / _bwd with the same cases as the LSTM cell; acts = (r, z, n, gh_n), gh_n a bit-exact copy; on live
    rows the r- and z-blocks of dgx and dgh are the same values bit for bit"""
    L, p = lib.lib(), lib.ptr
    g = gen(B * 11 + H)
    gx, gh = with_extremes(torch.randn(B, 3 * H, generator=g)), with_extremes(torch.randn(B, 3 * H, generator=g), start=3)
    h_prev = torch.randn(B, H, generator=g).tanh()
    gxd, ghd, hpd = dev(gx), dev(gh), dev(h_prev)
    for live in (None, live_rows(B)):
        h_ref, y_ref, a_ref = rr.gru_cell_fwd(gx, gh, h_prev, live)
        s_a, s_h = gru_fwd_scales(gx, gh, h_prev, a_ref)
        dead = torch.zeros(B, dtype=torch.bool) if live is None else live == 0
        for with_y in (True, False):
            name = f"gru_cell_fwd {B}x{H} live={live is not None} y={with_y}"
            h, y, acts = Out(B, H), Out(B, H), Out(B, 4 * H)
            rc = L.eamd_gru_cell_fwd(p(gxd), p(ghd), p(hpd), p(dev(live)), p(h.v), p(y.v) if with_y else None, p(acts.v), B, H, sp(lib))
            assert rc == 0
            assert bool(torch.isfinite(h.v).all()) and bool(torch.isfinite(acts.v).all())
            check("GATE_TOL", name + " acts", acts.v, a_ref, s_a)
            assert_bits(name + " gh_n copy", acts.v[:, 3 * H:], gh[:, 2 * H:])
            check("CELL_FWD_TOL", name + " h", h.v, h_ref, torch.where(dead.unsqueeze(1), h_prev.double().abs() + TINY, s_h))
            assert_bits(name + " dead h == h_prev", h.v[dead], h_prev[dead])
            if with_y:
                check("CELL_FWD_TOL", name + " y", y.v, y_ref, s_h)
                assert_zero_bits(name + " dead y == +0", y.v[dead])
                y.guards(name)
            else:
                y.untouched(name + " y NULL")
            h.guards(name)
            acts.guards(name)
        acts32 = a_ref.float()
        dy, dh = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
        for mask in range(1, 4):
            uy, uh = dy if mask & 1 else None, dh if mask & 2 else None
            name = f"gru_cell_bwd {B}x{H} live={live is not None} dy={mask & 1} dh={mask >> 1}"
            dgx_ref, dgh_ref, dhd_ref = rr.gru_cell_bwd(uy, uh, acts32, h_prev, live)
            r, z, n, ghn = acts32.double().reshape(B, 4, H).unbind(1)
            d = zabs(uh, h_ref) + zabs(uy, h_ref)
            s_dn = d * (1 + z) * (1 + n * n)
            s_dz = d * (h_prev.double().abs() + n.abs()) * z * (1 + z)
            s_dr = s_dn * ghn.abs() * r * (1 + r)
            dgx, dgh, dhd = Out(B, 3 * H), Out(B, 3 * H), Out(B, H)
            rc = L.eamd_gru_cell_bwd(p(dev(uy)), p(dev(uh)), p(dev(acts32)), p(hpd), p(dev(live)), p(dgx.v), p(dgh.v), p(dhd.v), B, H, sp(lib))
            assert rc == 0
            check("CELL_BWD_TOL", name + " dgx", dgx.v, dgx_ref, torch.cat([s_dr, s_dz, s_dn], dim=1) + TINY)
            check("CELL_BWD_TOL", name + " dgh", dgh.v, dgh_ref, torch.cat([s_dr, s_dz, s_dn * r], dim=1) + TINY)
            check("CELL_BWD_TOL", name + " dh_direct", dhd.v, dhd_ref, torch.where(dead.unsqueeze(1), zabs(uh, h_ref), d * z) + TINY)
            assert_bits(name + " dgx r, z blocks == dgh r, z blocks", dgx.v[:, :2 * H], dgh.v[:, :2 * H].cpu())
            assert_zero_bits(name + " dead dgx == +0", dgx.v[dead])
            assert_zero_bits(name + " dead dgh == +0", dgh.v[dead])
            assert_bits(name + " dead dh_direct has the bits of dh", dhd.v[dead], (dh if uh is not None else torch.zeros(B, H))[dead])
            for o in (dgx, dgh, dhd):
                o.guards(name)
    outs = [Out(B, 3 * H), Out(B, 3 * H), Out(B, H)]
    assert L.eamd_gru_cell_bwd(None, None, p(ghd), p(hpd), None, p(outs[0].v), p(outs[1].v), p(outs[2].v), B, H, sp(lib)) == EINVAL
    for o in outs:
        o.untouched(f"refused gru_cell_bwd {B}x{H}")


# =============================================================================================
# b. one-launch LSTM step
# =============================================================================================
def lstm_step_waves(K):
    """lstm_step_waves of rnn.hip: the largest count <= 16 that leaves every wave a multiple of 16 reduction steps"""
    q = K // 16
    return next((d for d in range(16, 1, -1) if q % d == 0), 1)


def step_fwd_supported(B, H, gx, w_hh, h_prev):
    return H % 64 == 0 and B <= 64 and aligned(16, gx, w_hh, h_prev)


def step_bwd_supported(B, H, dgn, w_t):
    return H % 64 == 0 and B <= 64 and aligned(16, dgn, w_t)


# (B, H): every B-class (MT 1..4, full and ragged last tiles) and every per-wave reduction length
STEP_FWD_CASES = [(1, 64), (5, 320), (16, 768), (17, 1024), (33, 1088), (48, 64), (49, 320), (64, 1024), (64, 768), (17, 1088),
                  (33, 64), (49, 1024)]
STEP_BWD_CASES = [(1, 64), (5, 128), (16, 192), (17, 256), (33, 320), (48, 64), (49, 128), (64, 256), (64, 320), (17, 192),
                  (33, 128), (49, 64)]


def test_lstm_step_case_lists_cover_every_class():
    assert {b for b, _ in STEP_FWD_CASES} == {1, 5, 16, 17, 33, 48, 49, 64} == {b for b, _ in STEP_BWD_CASES}
    assert {h for _, h in STEP_FWD_CASES} == {64, 320, 768, 1024, 1088}
    assert {h // lstm_step_waves(h) for _, h in STEP_FWD_CASES} == {16, 32, 48, 64, 272}
    assert {h for _, h in STEP_BWD_CASES} == {64, 128, 192, 256, 320}
    assert all(lstm_step_waves(4 * h) == 16 for _, h in STEP_BWD_CASES)
    assert {4 * h // 16 for _, h in STEP_BWD_CASES} == {16, 32, 48, 64, 80}


def step_inputs(B, H, seed):
    g = gen(seed)
    gx = torch.randn(B, 4 * H, generator=g)
    w = torch.randn(4 * H, H, generator=g) / math.sqrt(H)
    b = torch.randn(4 * H, generator=g) * 0.5
    h_prev, c_prev = torch.randn(B, H, generator=g).tanh(), torch.randn(B, H, generator=g)
    return g, gx, w, b, h_prev, c_prev


@pytest.mark.parametrize("B,H", STEP_FWD_CASES)
def test_lstm_step_fwd_vs_float64(lib, B, H):
    """eamd_lstm_step_fwd, one step: gates = gx + b_hh + h_prev W_hh^T by MFMA over NW waves, then the cell.  b_hh, live and y
    each NULL and given.  Rows at or beyond B are clamped reads: the guards behind every [B, .] output stay untouched."""
    L, p = lib.lib(), lib.ptr
    g, gx, w, b, h_prev, c_prev = step_inputs(B, H, B * 13 + H)
    gxd, wd, bd, hpd, cpd = dev(gx), dev(w), dev(b), dev(h_prev), dev(c_prev)
    assert step_fwd_supported(B, H, gxd, wd, hpd)
    nw, mt = lstm_step_waves(H), cdiv(B, 16)
    print(f"[rnn] lstm_step_fwd B={B} H={H}: MT={mt}, {nw} waves x {H // nw} inputs, LDS {nw * mt * 16 * 17 * 4} bytes")
    for use_b, live, with_y in [(True, live_rows(B), True), (False, None, False), (True, None, True), (False, live_rows(B), False)]:
        name = f"lstm_step_fwd {B}x{H} b_hh={use_b} live={live is not None} y={with_y}"
        bb = b if use_b else None
        h_ref, c_ref, y_ref, a_ref = rr.lstm_step_fwd(gx, w, bb, h_prev, c_prev, live)
        S = gx.double().abs() + h_prev.double().abs() @ w.double().abs().t() + (b.double().abs() if use_b else 0)
        s_a, s_c, s_h = lstm_fwd_scales(a_ref, c_prev.double(), rr.lstm_step_fwd(gx, w, bb, h_prev, c_prev)[1], S)
        dead = torch.zeros(B, dtype=torch.bool) if live is None else live == 0
        h, c, y, acts = Out(B, H), Out(B, H), Out(B, H), Out(B, 4 * H)
        rc = L.eamd_lstm_step_fwd(p(gxd), p(wd), p(bd) if use_b else None, p(hpd), p(cpd), p(dev(live)), p(h.v), p(c.v),
                                  p(y.v) if with_y else None, p(acts.v), B, H, sp(lib))
        assert rc == 0, f"{name}: rc {rc}"
        check("STEP_FWD_TOL", name + " acts", acts.v, a_ref, s_a)
        check("STEP_FWD_TOL", name + " c", c.v, c_ref, torch.where(dead.unsqueeze(1), c_prev.double().abs() + TINY, s_c))
        check("STEP_FWD_TOL", name + " h", h.v, h_ref, torch.where(dead.unsqueeze(1), h_prev.double().abs() + TINY, s_h))
        assert_bits(name + " dead c == c_prev", c.v[dead], c_prev[dead])
        assert_bits(name + " dead h == h_prev", h.v[dead], h_prev[dead])
        if with_y:
            check("STEP_FWD_TOL", name + " y", y.v, y_ref, s_h)
            assert_zero_bits(name + " dead y == +0", y.v[dead])
            y.guards(name)
        else:
            y.untouched(name + " y NULL")
        for o in (h, c, acts):
            o.guards(name)


@pytest.mark.parametrize("B,H", STEP_BWD_CASES)
def test_lstm_step_bwd_vs_float64(lib, B, H):
    """eamd_lstm_step_bwd, one step: dgates_next NULL (first step) and each of dh_pass_in, dc, dy NULL.  With every row dead
    and dy = dc = NULL the kernel writes dh_pass = dh_pass_in + dgates_next W_hh untouched by any transcendental: held to
    (4H + 1 + 8) * 2^-24 of the sum of the absolute values of the terms."""
    L, p = lib.lib(), lib.ptr
    g, gx, w, b, h_prev, c_prev = step_inputs(B, H, B * 17 + H)
    live = live_rows(B)
    _, c_ref, _, a_ref = rr.lstm_step_fwd(gx, w, b, h_prev, c_prev, live)
    acts32, c32 = a_ref.float(), c_ref.float()
    w_t = w.t().contiguous()                                   # [H, 4H]
    dy, dpi, dc = (torch.randn(B, H, generator=g) for _ in range(3))
    dgn = torch.randn(B, 4 * H, generator=g)
    wtd, a32d, cpd, c32d = dev(w_t), dev(acts32), dev(c_prev), dev(c32)
    nw, mt = lstm_step_waves(4 * H), cdiv(B, 16)
    print(f"[rnn] lstm_step_bwd B={B} H={H}: MT={mt}, {nw} waves x {4 * H // nw} gate rows, LDS {nw * mt * 16 * 17 * 4} bytes")
    s_mm = dgn.double().abs() @ w.double().abs()
    cases = [("all", dy, dgn, dpi, dc, live), ("first step", dy, None, None, None, live), ("dh_pass_in NULL", dy, dgn, None, dc, live),
             ("dc NULL", dy, dgn, dpi, None, None), ("dy NULL", None, dgn, dpi, dc, live)]
    for tag, uy, un, ui, uc, lv in cases:
        name = f"lstm_step_bwd {B}x{H} {tag}"
        und = dev(un)
        assert step_bwd_supported(B, H, und, wtd)
        dg_ref, dcp_ref, dhp_ref = rr.lstm_step_bwd(uy, un, w, ui, uc, acts32, c_prev, c32, lv)
        s_dh = zabs(ui, c_ref) + (s_mm if un is not None else 0)
        s_dg, s_dcp = lstm_bwd_scales(uy, s_dh, zabs(uc, c_ref), acts32.double(), c_prev.double(), c32.double())
        dead = torch.zeros(B, dtype=torch.bool) if lv is None else lv == 0
        dgo, dcpo, dhpo = Out(B, 4 * H), Out(B, H), Out(B, H)
        rc = L.eamd_lstm_step_bwd(p(dev(uy)), p(und), p(wtd), p(dev(ui)), p(dev(uc)), p(a32d), p(cpd), p(c32d), p(dev(lv)),
                                  p(dgo.v), p(dcpo.v), p(dhpo.v), B, H, sp(lib))
        assert rc == 0, f"{name}: rc {rc}"
        check("STEP_BWD_TOL", name + " dgates", dgo.v, dg_ref, s_dg)
        check("STEP_BWD_TOL", name + " dc_prev", dcpo.v, dcp_ref, torch.where(dead.unsqueeze(1), zabs(uc, c_ref) + TINY, s_dcp))
        check("STEP_DEAD_TOL", name + " dh_pass", dhpo.v, dhp_ref, s_dh + TINY, n_terms=4 * H + 1)
        assert_zero_bits(name + " dead dgates == +0", dgo.v[dead])
        assert_zero_bits(name + " live dh_pass == +0", dhpo.v[~dead])
        assert_bits(name + " dead dc_prev has the bits of dc", dcpo.v[dead], (dc if uc is not None else torch.zeros(B, H))[dead])
        for o in (dgo, dcpo, dhpo):
            o.guards(name)
    # the MFMA reduction alone: every row dead
    name = f"lstm_step_bwd {B}x{H} all rows dead"
    alldead = torch.zeros(B, dtype=U8)
    dgo, dcpo, dhpo = Out(B, 4 * H), Out(B, H), Out(B, H)
    rc = L.eamd_lstm_step_bwd(None, p(dev(dgn)), p(wtd), p(dev(dpi)), None, p(a32d), p(cpd), p(c32d), p(dev(alldead)),
                              p(dgo.v), p(dcpo.v), p(dhpo.v), B, H, sp(lib))
    assert rc == 0
    check("STEP_DEAD_TOL", name + " dh_pass", dhpo.v, dpi.double() + dgn.double() @ w.double(), dpi.double().abs() + s_mm,
          n_terms=4 * H + 1)
    assert_zero_bits(name + " dgates == +0", dgo.v)
    assert_zero_bits(name + " dc_prev == +0", dcpo.v)
    for o in (dgo, dcpo, dhpo):
        o.guards(name)


def test_lstm_step_refusals(lib):
    """H = 96, B = 65, misaligned gx / w_hh / h_prev (forward), misaligned dgates_next / w_t (backward): EAMD_EUNSUPPORTED and
    every output bit-identical to the fill"""
    L, p = lib.lib(), lib.ptr

    def fwd(B, H, mis=None):
        t = {k: torch.zeros(n + 1, device=DEV) for k, n in (("gx", B * 4 * H), ("w", 4 * H * H), ("h", B * H))}
        v = {k: (b[1:] if k == mis else b[:-1]) for k, b in t.items()}
        cp = torch.zeros(B * H, device=DEV)
        outs = [Out(B, H), Out(B, H), Out(B, H), Out(B, 4 * H)]
        assert not step_fwd_supported(B, H, v["gx"], v["w"], v["h"])
        rc = L.eamd_lstm_step_fwd(p(v["gx"]), p(v["w"]), None, p(v["h"]), p(cp), None, p(outs[0].v), p(outs[1].v), p(outs[2].v),
                                  p(outs[3].v), B, H, sp(lib))
        assert rc == EUNSUPPORTED, f"forward B={B} H={H} misaligned={mis}: rc {rc}"
        for o in outs:
            o.untouched(f"refused lstm_step_fwd B={B} H={H} {mis}")

    def bwd(B, H, mis=None):
        t = {k: torch.zeros(n + 1, device=DEV) for k, n in (("dgn", B * 4 * H), ("w_t", 4 * H * H))}
        v = {k: (b[1:] if k == mis else b[:-1]) for k, b in t.items()}
        z = torch.zeros(B * 4 * H, device=DEV)
        outs = [Out(B, 4 * H), Out(B, H), Out(B, H)]
        assert not step_bwd_supported(B, H, v["dgn"], v["w_t"])
        rc = L.eamd_lstm_step_bwd(p(z), p(v["dgn"]), p(v["w_t"]), None, None, p(z), p(z), p(z), None, p(outs[0].v), p(outs[1].v),
                                  p(outs[2].v), B, H, sp(lib))
        assert rc == EUNSUPPORTED, f"backward B={B} H={H} misaligned={mis}: rc {rc}"
        for o in outs:
            o.untouched(f"refused lstm_step_bwd B={B} H={H} {mis}")

    for f in (fwd, bwd):
        f(4, 96)
        f(65, 64)
    for mis in ("gx", "w", "h"):
        fwd(4, 64, mis)
    for mis in ("dgn", "w_t"):
        bwd(4, 64, mis)


# =============================================================================================
# c. 2x2 ceil-mode max-pool
# =============================================================================================
@pytest.mark.parametrize("shape", [(2, 9, 7, 128), (1, 1, 1, 3), (3, 2, 5, 65)])
@pytest.mark.parametrize("neg_inf", [False, True])
def test_maxpool_bits(lib, shape, neg_inf):
    """inputs from {-2, -1, 0, 1} * 2^-3 (ties in most windows), with windows of all -inf: y, idx and dx bit for bit"""
    L, p = lib.lib(), lib.ptr
    B, H, W, C = shape
    g = gen(sum(shape))
    x = (torch.randint(-2, 2, shape, generator=g).float()) / 8
    if neg_inf:
        x[:, 0:2, 0:2, :] = -INF
        x[:, H - 1, W - 1, ::2] = -INF
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    y_ref, idx_ref = rr.maxpool2x2_fwd(x)
    ties = int((rr._pool_windows(x.double())[0] == y_ref.unsqueeze(0)).sum(0).gt(1).sum())
    assert H * W == 1 or ties > 0
    name = f"maxpool {shape} -inf={neg_inf}"
    y, idx = Out(B, Ho, Wo, C), Out(B, Ho, Wo, C, dtype=U8)
    xd = dev(x)
    assert L.eamd_maxpool2x2_fwd(p(xd), p(y.v), p(idx.v), B, H, W, C, sp(lib)) == 0
    assert_bits(name + " y", y.v, y_ref.float())
    assert_bits(name + " idx", idx.v, idx_ref)
    dy = torch.randn(B, Ho, Wo, C, generator=g)
    dx = Out(B, H, W, C)
    assert L.eamd_maxpool2x2_bwd(p(dev(dy)), p(idx.v), p(dx.v), B, H, W, C, sp(lib)) == 0
    assert_bits(name + " dx", dx.v, rr.maxpool2x2_bwd(dy, idx_ref, shape).float())
    for o in (y, idx, dx):
        o.guards(name)


# =============================================================================================
# d. eamd_attloc_fwd
# =============================================================================================
def attloc_fwd_branch(C, R, K, A, pre_enc, th, dec_proj, gvec):
    """the dispatch of eamd_attloc_fwd"""
    if 0 < C <= 16 and R == 1 and K <= 255 and A % 4 == 0 and A <= 1024 and aligned(16, pre_enc, th, dec_proj, gvec):
        return "fwd8<10>" if C == 10 else "fwd8<16>"
    return "generic"


def make_lens(mode, B, T, g):
    if mode == "full":
        return torch.full((B,), T, dtype=I32)
    lens = torch.randint(1, T + 1, (B,), generator=g).int()
    lens[0] = T
    if mode == "one":
        lens[B - 1] = 1
    elif T > 1:
        lens[B - 1] = max(1, T // 2)
    return lens


def attloc_inputs(B, T, A, C, K, R, E, lens_mode, seed):
    g = gen(seed)
    lens = make_lens(lens_mode, B, T, g)
    d = dict(lens=lens, pre=torch.randn(B, T, A, generator=g), dec=torch.randn(B, A, generator=g),
             gvec=torch.randn(A, generator=g), gb=torch.randn(1, generator=g), enc=torch.randn(B, T, E, generator=g),
             prev=None, cw=None, wa=None)
    if C:
        prev = torch.rand(B, R, T, generator=g) * rr.frame_mask(lens, T).unsqueeze(1)
        d["prev"] = (prev / prev.sum(2, keepdim=True)).float()
        d["cw"] = torch.randn(C, R, K, generator=g)
        d["wa"] = torch.randn(A, C, generator=g) / math.sqrt(C)
    return d


def softmax_scales(e, s_e, w, scaling):
    """scale of w = softmax(scaling * e): the rounding of the exponent's argument and the propagated error of e"""
    fin = torch.isfinite(e)
    ea = torch.where(fin, e.abs(), torch.zeros_like(e))
    m = torch.where(fin, e, torch.full_like(e, -INF)).max(dim=1, keepdim=True).values.abs()
    se = abs(scaling) * (torch.where(fin, s_e, torch.zeros_like(e)) + ea + m)
    return w * (1 + se + (w * se).sum(1, keepdim=True)) + TINY


# name: B, T, A, C, K, R, E, lens, scaling, misaligned pre_enc, branch
ATTLOC_FWD_CASES = [
    ("fwd8_10", 3, 70, 60, 10, 41, 1, 65, "short", 2.0, False, "fwd8<10>"),
    ("fwd8_10_T1_A1024", 1, 1, 1024, 10, 3, 1, 130, "full", 1.0, False, "fwd8<10>"),
    ("fwd8_16_C1", 2, 7, 4, 1, 3, 1, 1, "full", 1.0, False, "fwd8<16>"),
    ("fwd8_16_C4_K201", 2, 8, 64, 4, 201, 1, 63, "one", 2.0, False, "fwd8<16>"),
    ("fwd8_16_C16_A1020", 2, 9, 1020, 16, 1, 1, 64, "short", 1.0, False, "fwd8<16>"),
    ("generic_C0", 2, 9, 8, 0, 0, 1, 5, "short", 2.0, False, "generic"),
    ("generic_C17", 2, 8, 8, 17, 3, 1, 3, "one", 1.0, False, "generic"),
    ("generic_C64", 2, 7, 12, 64, 5, 1, 3, "short", 1.0, False, "generic"),
    ("generic_R3", 2, 9, 8, 10, 5, 3, 3, "short", 2.0, False, "generic"),
    ("generic_A6", 2, 9, 6, 10, 3, 1, 3, "full", 1.0, False, "generic"),
    ("generic_A1028", 2, 3, 1028, 10, 3, 1, 3, "short", 1.0, False, "generic"),
    ("generic_K257", 2, 9, 8, 10, 257, 1, 3, "short", 1.0, False, "generic"),
    ("generic_misaligned", 2, 9, 8, 10, 3, 1, 3, "short", 1.0, True, "generic"),
]


@pytest.mark.parametrize("case", ATTLOC_FWD_CASES, ids=[c[0] for c in ATTLOC_FWD_CASES])
def test_attloc_fwd_vs_float64(lib, case):
    """e, th, conv, w, ctx on the eight-frame kernels (<10> and the padded <16>) and the per-frame kernel, each reason for the
    latter alone.  Masked frames: e has the bits of -inf, w == +0, th and conv are still written and right."""
    name, B, T, A, C, K, R, E, lens_mode, scaling, mis, branch = case
    L, p = lib.lib(), lib.ptr
    d = attloc_inputs(B, T, A, C, K, R, E, lens_mode, len(name) * 31 + T)
    pre_buf = torch.zeros(B * T * A + 1, device=DEV)
    pre = (pre_buf[1:] if mis else pre_buf[:-1]).view(B, T, A)
    pre.copy_(d["pre"])
    dd = {k: dev(v) for k, v in d.items()}
    e, th, w, ctx = Out(B, T), Out(B, T, A), Out(B, T), Out(B, E)
    conv = Out(B, T, max(C, 1))
    assert attloc_fwd_branch(C, R, K, A, pre, th.v, dd["dec"], dd["gvec"]) == branch, f"{name}: wrong branch"
    rc = L.eamd_attloc_fwd(p(dd["prev"]), p(dd["cw"]), p(dd["wa"]), p(pre), p(dd["dec"]), p(dd["gvec"]), p(dd["gb"]), p(dd["lens"]),
                           p(dd["enc"]), scaling, p(e.v), p(th.v), p(conv.v) if C else None, p(w.v), p(ctx.v), B, T, A, C, K, R, E,
                           sp(lib))
    assert rc == 0
    e_ref, th_ref, conv_ref, w_ref, ctx_ref = rr.attloc_fwd(d["prev"], d["cw"], d["wa"], d["pre"], d["dec"], d["gvec"], d["gb"],
                                                            d["lens"], d["enc"], scaling)
    s_f = d["pre"].double().abs() + d["dec"].double().abs().unsqueeze(1)
    if C:
        s_conv = rr.loc_conv(d["prev"].abs(), d["cw"].abs())
        check("ATT_CONV_TOL", f"attloc_fwd {name} conv", conv.v, conv_ref, s_conv + TINY, n_terms=R * K)
        s_f = s_f + s_conv @ d["wa"].double().abs().t()
        conv.guards(name)
    else:
        conv.untouched(name + " conv NULL")
    s_th = th_ref.abs() + (1 - th_ref * th_ref) * s_f + TINY
    check("ATT_TH_TOL", f"attloc_fwd {name} th", th.v, th_ref, s_th)
    s_e = s_th @ d["gvec"].double().abs() + d["gb"].double().abs()
    check("ATT_E_TOL", f"attloc_fwd {name} e", e.v, e_ref, s_e)
    masked = ~rr.frame_mask(d["lens"], T)
    assert lens_mode == "full" or bool(masked.any())
    assert_bits(f"attloc_fwd {name} masked e == -inf", e.v[masked], torch.full((int(masked.sum()),), -INF))
    assert_zero_bits(f"attloc_fwd {name} masked w == +0", w.v[masked])
    s_w = softmax_scales(e_ref, s_e, w_ref, scaling)
    check("ATT_W_TOL", f"attloc_fwd {name} w", w.v, w_ref, s_w)
    check("ATT_CTX_TOL", f"attloc_fwd {name} ctx", ctx.v, ctx_ref, torch.einsum("bt,bte->be", s_w, d["enc"].double().abs()) + TINY)
    for o in (e, th, w, ctx):
        o.guards(name)


def test_attloc_fwd_refusals(lib):
    """C = 65, even K, T = 15361 (more frames than the softmax row holds in LDS; refused before any launch, so only e and w
    are allocated at size) -> EAMD_EUNSUPPORTED; C > 0 without conv_w -> EAMD_EINVAL; all outputs keep the fill"""
    L, p = lib.lib(), lib.ptr
    z = torch.zeros(4096, device=DEV)
    lens = torch.ones(2, dtype=I32, device=DEV)
    for tag, T, C, K, cw, want in [("C=65", 4, 65, 3, z, EUNSUPPORTED), ("even K", 4, 10, 4, z, EUNSUPPORTED),
                                   ("T=15361", 15361, 10, 3, z, EUNSUPPORTED), ("conv_w NULL", 4, 10, 3, None, EINVAL)]:
        B, A, E = 1, 4, 2
        e, w = Out(B, T), Out(B, T)
        th, conv, ctx = Out(16), Out(16), Out(16)
        rc = L.eamd_attloc_fwd(p(z), p(cw), p(z), p(z), p(z), p(z), p(z), p(lens), p(z), 1.0, p(e.v), p(th.v), p(conv.v), p(w.v),
                               p(ctx.v), B, T, A, C, K, 1, E, sp(lib))
        assert rc == want, f"{tag}: rc {rc}"
        for o in (e, w, th, conv, ctx):
            o.untouched(f"refused attloc_fwd {tag}")


# =============================================================================================
# e. eamd_attloc_bwd_energy and eamd_attloc_bwd_energy_conv
# =============================================================================================
def fused_unroll(C):
    return "<10>" if C == 10 else "<4>" if C == 4 else "<16>"


def fused_supported(T, A, C, th, df, gvec, ws):
    return T * 4 <= 60 * 1024 and C <= 16 and A % 4 == 0 and A <= 1024 and aligned(16, th, df, gvec, ws)


# name: B, T, A, C, E, accumulate, dw_ext given, slabs = B * ceil(T / 32), unroll
ATTLOC_BWD_CASES = [
    ("slabs1", 1, 1, 1024, 10, 1, 0, True, 1, "<10>"),
    ("slabs4", 4, 3, 1024, 4, 5, 1, False, 4, "<4>"),
    ("slabs4_T33", 2, 33, 60, 16, 64, 1, True, 4, "<16>"),
    ("slabs31", 31, 31, 4, 1, 3, 0, True, 31, "<16>"),
    ("slabs32", 32, 32, 60, 3, 2, 1, True, 32, "<16>"),
    ("slabs33", 11, 70, 60, 16, 4, 0, True, 33, "<16>"),
    ("slabs36", 12, 70, 4, 10, 65, 1, False, 36, "<10>"),
    ("slabs65", 13, 133, 60, 4, 3, 0, True, 65, "<4>"),
]


@pytest.mark.parametrize("case", ATTLOC_BWD_CASES, ids=[c[0] for c in ATTLOC_BWD_CASES])
def test_attloc_bwd_energy_vs_float64(lib, case):
    """stage 1 of the backward, unfused and fused (dconv and dw_att folded in), both against float64 and against each other.
    dgvec, dgb, d_dec_proj, dw_att (and d_enc_h / df under accumulate) start non-zero and every entry is called twice.  Chunk
    lengths 1, 2 and 3 modulo the four-frame groups; slab counts at the edges of the reduce kernel's 32-slab loop; T = 133
    gives five chunks per utterance (the d_dec_proj loop)."""
    name, B, T, A, C, E, accumulate, with_ext, slabs, unroll = case
    L, p = lib.lib(), lib.ptr
    assert B * cdiv(T, 32) == slabs and fused_unroll(C) == unroll
    d = attloc_inputs(B, T, A, C, 3, 1, E, "short" if B > 1 else "full", slabs * 7 + T)
    scaling = 2.0 if accumulate else 1.0
    _, th64, conv64, w64, _ = rr.attloc_fwd(d["prev"], d["cw"], d["wa"], d["pre"], d["dec"], d["gvec"], d["gb"], d["lens"], d["enc"], scaling)
    th, conv, w = th64.float(), conv64.float(), w64.float()
    g = gen(slabs)
    dctx, dw_ext = torch.randn(B, E, generator=g), (torch.randn(B, T, generator=g) if with_ext else None)
    ref = rr.attloc_bwd_energy_conv(dctx, dw_ext, w, d["enc"], th, d["gvec"], scaling, conv, d["wa"])
    de_ref, deh_ref, df_ref, dgvec_ref, dgb_ref, ddec_ref, dconv_ref, dwatt_ref = ref
    masked = ~rr.frame_mask(d["lens"], T)
    # scales
    wd_, enc_a, gv_a = w.double(), d["enc"].double().abs(), d["gvec"].double().abs()
    s_dw = torch.einsum("bte,be->bt", enc_a, dctx.double().abs()) + (dw_ext.double().abs() if with_ext else 0)
    s_de = scaling * wd_ * (s_dw + (wd_ * s_dw).sum(1, keepdim=True))
    s_deh = wd_.unsqueeze(2) * dctx.double().abs().unsqueeze(1)
    s_df = s_de.unsqueeze(2) * gv_a * (1 + th.double() ** 2)
    s_dgvec = torch.einsum("bt,bta->a", s_de, th.double().abs())
    s_ddec = s_df.sum(1)
    s_dconv = s_df @ d["wa"].double().abs()
    s_dwatt = torch.einsum("bta,btc->ac", s_df, conv.double().abs())
    dv = {k: dev(v) for k, v in dict(dctx=dctx, dw_ext=dw_ext, w=w, enc=d["enc"], th=th, gvec=d["gvec"], conv=conv, wa=d["wa"]).items()}
    dgb0 = torch.full((9,), 2.0 ** -10)

    def common(tag, de, deh, df, dgvec, dgb, ddec, deh0=None, df0=None):
        nm = f"attloc_bwd {name} {tag}"
        check("ATT_DE_TOL", nm + " de", de.v, de_ref, s_de + TINY)
        assert_zero_value(nm + " masked de == 0", de.v[masked])
        if deh0 is None:
            check("ATT_DENC_TOL", nm + " d_enc_h", deh.v, deh_ref, s_deh + TINY, n_terms=1)
            check("ATT_DF_TOL", nm + " df", df.v, df_ref, s_df + TINY)
            assert_zero_value(nm + " masked df == 0", df.v[masked])
        else:
            check("ATT_DENC_TOL", nm + " d_enc_h accumulated", deh.v, deh0 + 2 * deh_ref, deh0.abs() + 2 * s_deh, n_terms=3)
            check("ATT_DF_TOL", nm + " df accumulated", df.v, df0 + 2 * df_ref, df0.abs() + 2 * s_df)
            assert_bits(nm + " masked df unchanged", df.v[masked], df0[masked].float())
        check("ATT_RED_TOL", nm + " dgvec", dgvec.v, dgvec.v0 + 2 * dgvec_ref, dgvec.v0.abs() + 2 * s_dgvec)
        check("ATT_RED_TOL", nm + " d_dec_proj", ddec.v, ddec.v0 + 2 * ddec_ref, ddec.v0.abs() + 2 * s_ddec)
        check("ATT_DGB_TOL", nm + " dgb", dgb.v, dgb.v0, (2 * de_ref.abs().sum() + TINY).reshape(1))
        for o in (de, deh, df, dgvec, dgb, ddec):
            o.guards(nm)

    # unfused: d_enc_h and df are overwritten
    de_u, deh_u, df_u = Out(B, T), Out(B, T, E), Out(B, T, A)
    dgvec_u, dgb_u, ddec_u = Acc(A, seed=1), Acc(1, start=dgb0), Acc(B, A, seed=2)
    for _ in range(2):
        rc = L.eamd_attloc_bwd_energy(p(dv["dctx"]), p(dv["dw_ext"]), p(dv["w"]), p(dv["enc"]), p(dv["th"]), p(dv["gvec"]), scaling,
                                      p(de_u.v), p(deh_u.v), p(df_u.v), p(dgvec_u.v), p(dgb_u.v), p(ddec_u.v), B, T, A, E, sp(lib))
        assert rc == 0
    common("unfused", de_u, deh_u, df_u, dgvec_u, dgb_u, ddec_u)
    # fused
    nbytes = L.eamd_attloc_bwd_workspace(B, T, A, C)
    assert nbytes == rr.attloc_bwd_workspace(B, T, A, C)
    ws = Out(nbytes // 4)
    de_f, dconv_f = Out(B, T), Out(B, T, C)
    dgvec_f, dgb_f, ddec_f, dwatt_f = Acc(A, seed=1), Acc(1, start=dgb0), Acc(B, A, seed=2), Acc(A, C, seed=3)
    if accumulate:
        deh_f, df_f = Acc(B, T, E, seed=4), Acc(B, T, A, seed=5)
    else:
        deh_f, df_f = Out(B, T, E), Out(B, T, A)
    assert fused_supported(T, A, C, dv["th"], df_f.v, dv["gvec"], ws.v)
    for _ in range(2):
        rc = L.eamd_attloc_bwd_energy_conv(p(dv["dctx"]), p(dv["dw_ext"]), p(dv["w"]), p(dv["enc"]), p(dv["th"]), p(dv["gvec"]), scaling,
                                           p(dv["conv"]), p(dv["wa"]), p(de_f.v), p(deh_f.v), p(df_f.v), p(dconv_f.v), p(dgvec_f.v),
                                           p(dgb_f.v), p(ddec_f.v), p(dwatt_f.v), p(ws.v), accumulate, B, T, A, C, E, sp(lib))
        assert rc == 0
    common(f"fused{unroll} accumulate={accumulate}", de_f, deh_f, df_f, dgvec_f, dgb_f, ddec_f,
           deh_f.v0 if accumulate else None, df_f.v0 if accumulate else None)
    nm = f"attloc_bwd {name} fused{unroll}"
    check("ATT_DCONV_TOL", nm + " dconv", dconv_f.v, dconv_ref, s_dconv + TINY, n_terms=E + T + A + 8)
    check("ATT_RED_TOL", nm + " dw_att", dwatt_f.v, dwatt_f.v0 + 2 * dwatt_ref, dwatt_f.v0.abs() + 2 * s_dwatt)
    for o in (dconv_f, dwatt_f, ws):
        o.guards(nm)
    # fused against unfused
    assert_bits(nm + " de fused == unfused", de_f.v, de_u.v.cpu())
    check("ATT_FUSED_TOL", nm + " dgvec vs unfused", dgvec_f.v, dgvec_u.v.double().cpu(), dgvec_u.v0.abs() + 2 * s_dgvec)
    check("ATT_FUSED_TOL", nm + " d_dec_proj vs unfused", ddec_f.v, ddec_u.v.double().cpu(), ddec_u.v0.abs() + 2 * s_ddec)
    if not accumulate:
        check("ATT_FUSED_TOL", nm + " df vs unfused", df_f.v, df_u.v.double().cpu(), s_df + TINY)
        assert_bits(nm + " d_enc_h fused == unfused", deh_f.v, deh_u.v.cpu())


def test_attloc_bwd_energy_conv_refusals(lib):
    """C = 17, A = 6, A = 1028, th or workspace misaligned -> EAMD_EUNSUPPORTED, every output keeps the fill"""
    L, p = lib.lib(), lib.ptr
    z = torch.zeros(2 * 4 * 1028 * 20 + 1, device=DEV)
    for tag, A, C, mis in [("C=17", 8, 17, None), ("A=6", 6, 10, None), ("A=1028", 1028, 10, None), ("th misaligned", 8, 10, "th"),
                           ("workspace misaligned", 8, 10, "ws")]:
        B, T, E = 2, 4, 3
        ws = Out(B * A * (C + 2), off=1 if mis == "ws" else 0)
        th = z[1:] if mis == "th" else z
        outs = [Out(B, T), Out(B, T, E), Out(B, T, A), Out(B, T, C), Out(A), Out(1), Out(B, A), Out(A, C)]
        assert not fused_supported(T, A, C, th, outs[2].v, z, ws.v)
        rc = L.eamd_attloc_bwd_energy_conv(p(z), None, p(z), p(z), p(th), p(z), 1.0, p(z), p(z), *(p(o.v) for o in outs), p(ws.v), 0,
                                           B, T, A, C, E, sp(lib))
        assert rc == EUNSUPPORTED, f"{tag}: rc {rc}"
        for o in outs + [ws]:
            o.untouched(f"refused attloc_bwd_energy_conv {tag}")


# =============================================================================================
# f. eamd_attloc_bwd_conv
# =============================================================================================
@pytest.mark.parametrize("B,T,C,K,R", [(2, 7, 3, 3, 1), (3, 5, 10, 65, 3), (1, 70, 4, 201, 1), (2, 70, 2, 65, 3), (3, 9, 16, 201, 3)])
def test_attloc_bwd_conv_vs_float64(lib, B, T, C, K, R):
    """d_prev (written) and dconv_w (atomics onto non-zero values, called twice): R rows of history, K past the 64 lanes over k,
    T below and above F = (K - 1) / 2, B R T no multiple of the four rows of a workgroup"""
    L, p = lib.lib(), lib.ptr
    g = gen(B + T + C + K + R)
    dconv, cw = torch.randn(B, T, C, generator=g), torch.randn(C, R, K, generator=g)
    prev = torch.rand(B, R, T, generator=g)
    prev = (prev / prev.sum(2, keepdim=True)).float()
    name = f"attloc_bwd_conv B={B} T={T} C={C} K={K} R={R}"
    assert (B, T, C, K, R) == (2, 70, 2, 65, 3) or (B * R * T) % 4 != 0
    d_prev, dcw = Out(B, R, T), Acc(C, R, K, seed=K)
    for _ in range(2):
        rc = L.eamd_attloc_bwd_conv(p(dev(dconv)), p(dev(cw)), p(dev(prev)), p(d_prev.v), p(dcw.v), B, T, C, K, R, sp(lib))
        assert rc == 0
    dp_ref, dw_ref = rr.attloc_bwd_conv(dconv, cw, prev)
    s_dp, s_dw = rr.attloc_bwd_conv(dconv.abs(), cw.abs(), prev)
    check("ATT_DPREV_TOL", name + " d_prev", d_prev.v, dp_ref, s_dp + TINY, n_terms=C * min(K, 2 * T))
    check("ATT_DCONVW_TOL", name + " dconv_w", dcw.v, dcw.v0 + 2 * dw_ref, dcw.v0.abs() + 2 * s_dw, n_terms=2 * (B * T + 1))
    d_prev.guards(name)
    dcw.guards(name)
    out = Out(B, R, T)
    assert L.eamd_attloc_bwd_conv(p(dev(dconv)), p(dev(cw)), p(dev(prev)), p(out.v), p(dcw.v), B, T, C, K + 1, R, sp(lib)) == EINVAL
    out.untouched(name + " even K refused")


# =============================================================================================
# g. eamd_attloc_convmax_fwd / _bwd
# =============================================================================================
@pytest.mark.parametrize("B,C,T,K", [(1, 1, 1, 1), (1, 3, 63, 5), (2, 2, 64, 201), (1, 5, 65, 5), (3, 10, 200, 201), (5, 6, 200, 1),
                                     (1, 3, 65, 201)])
def test_attloc_convmax_bits(lib, B, C, T, K):
    """inputs on a dyadic grid (small integers * 2^-6, att_prev zero past each length): fp32 sums are exact in any order, so
    ties are real and go to the earliest frame; pooled, idx and the accumulated d_prev / dconv_w are bit-exact.  Row 0 of
    conv_w is nowhere positive: pooled == 0 and no gradient."""
    L, p = lib.lib(), lib.ptr
    g = gen(B * 3 + C + T + K)
    lens = make_lens("short", B, T, g)
    prev = (torch.randint(0, 4, (B, T), generator=g).float() / 64) * rr.frame_mask(lens, T)
    cw = torch.randint(-4, 5, (C, K), generator=g).float() / 64
    if C > 1 or T > 1:
        cw[0] = -cw[0].abs()
    name = f"convmax B={B} C={C} T={T} K={K}"
    assert B * C in (1, 3, 4, 5, 30)
    pooled_ref, idx_ref = rr.convmax_fwd(prev, cw)
    if T >= 63 and K <= 5:
        conv = rr.loc_conv(prev, cw)
        assert int((conv == conv.max(dim=1, keepdim=True).values).sum(1).gt(1).sum()) > 0, "no tie in this case"
    pooled, idx = Out(B, C), Out(B, C, dtype=I32)
    pd, cd = dev(prev), dev(cw)
    assert L.eamd_attloc_convmax_fwd(p(pd), p(cd), p(pooled.v), p(idx.v), B, T, C, K, sp(lib)) == 0
    assert_bits(name + " pooled", pooled.v, pooled_ref.float())
    assert_bits(name + " idx", idx.v, idx_ref)
    if C > 1 or T > 1:
        assert_zero_bits(name + " pooled of the non-positive row", pooled.v[:, 0])
    dpool = torch.randint(-8, 9, (B, C), generator=g).float() / 8
    dp0 = torch.randint(-8, 9, (B * T + 8,), generator=g).float() / 8
    dw0 = torch.randint(-8, 9, (C * K + 8,), generator=g).float() / 8
    d_prev, dcw = Acc(B, T, start=dp0), Acc(C, K, start=dw0)
    for _ in range(2):
        rc = L.eamd_attloc_convmax_bwd(p(dev(dpool)), p(pooled.v), p(idx.v), p(pd), p(cd), p(d_prev.v), p(dcw.v), B, T, C, K, sp(lib))
        assert rc == 0
    dp_ref, dw_ref = rr.convmax_bwd(dpool, pooled_ref, idx_ref, prev, cw)
    assert_bits(name + " d_prev", d_prev.v, (d_prev.v0 + 2 * dp_ref).float())
    assert_bits(name + " dconv_w", dcw.v, (dcw.v0 + 2 * dw_ref).float())
    if C > 1 or T > 1:
        assert_bits(name + " dconv_w of the non-positive row", dcw.v[0], dw0[:K])
    for o in (pooled, idx, d_prev, dcw):
        o.guards(name)
    r = Out(B, C)
    assert L.eamd_attloc_convmax_fwd(p(pd), p(cd), p(r.v), p(idx.v), B, T, C, K + 1, sp(lib)) == EINVAL
    r.untouched(name + " even K refused")


# =============================================================================================
# h. dot-product attention
# =============================================================================================
@pytest.mark.parametrize("B,T,A,E", [(1, 1, 1, 1), (3, 9, 63, 64), (2, 255, 64, 65), (1, 257, 65, 130), (2, 8, 320, 1), (1, 256, 1, 64),
                                     (1, 1500, 64, 65)])
def test_dot_attention_vs_float64(lib, B, T, A, E):
    """eamd_att_dot_energy_fwd -> eamd_att_ctx_fwd -> eamd_att_ctx_bwd -> eamd_att_dot_energy_bwd, each judged from the fp32
    values it is given: masked e is -inf, dk is written, dq and dsum accumulate onto non-zero values (called twice)"""
    L, p = lib.lib(), lib.ptr
    g = gen(B * 5 + T + A + E)
    lens = make_lens("short", B, T, g)
    k, q, v = torch.randn(B, T, A, generator=g).tanh(), torch.randn(B, A, generator=g).tanh(), torch.randn(B, T, E, generator=g)
    kd, qd, vd, ld = dev(k), dev(q), dev(v), dev(lens)
    name = f"dot B={B} T={T} A={A} E={E}"
    masked = ~rr.frame_mask(lens, T)
    scaling = 2.0
    e = Out(B, T)
    assert L.eamd_att_dot_energy_fwd(p(kd), p(qd), p(ld), p(e.v), B, T, A, sp(lib)) == 0
    e_ref = rr.att_dot_energy_fwd(k, q, lens)
    check("ATT_E_TOL", name + " e", e.v, e_ref, torch.einsum("bta,ba->bt", k.double().abs(), q.double().abs()) + TINY, n_terms=A)
    assert_bits(name + " masked e == -inf", e.v[masked], torch.full((int(masked.sum()),), -INF))
    e32 = e.v.cpu()
    w, ctx = Out(B, T), Out(B, E)
    assert L.eamd_att_ctx_fwd(p(e.v), p(vd), scaling, p(w.v), p(ctx.v), B, T, E, sp(lib)) == 0
    w_ref, ctx_ref = rr.att_ctx_fwd(e32, v, scaling)
    s_w = softmax_scales(e32.double(), torch.zeros(B, T, dtype=torch.float64), w_ref, scaling)
    check("ATT_W_TOL", name + " w", w.v, w_ref, s_w)
    check("ATT_CTX_TOL", name + " ctx", ctx.v, ctx_ref, torch.einsum("bt,bte->be", s_w, v.double().abs()) + TINY)
    assert_zero_bits(name + " masked w == +0", w.v[masked])
    w32 = w.v.cpu()
    dctx, dw_ext = torch.randn(B, E, generator=g), torch.randn(B, T, generator=g)
    de, d_v, dsum = Out(B, T), Out(B, T, E), Acc(1, start=torch.full((9,), 2.0 ** -20))
    for _ in range(2):
        assert L.eamd_att_ctx_bwd(p(dev(dctx)), p(dev(dw_ext)), p(w.v), p(vd), scaling, p(de.v), p(d_v.v), p(dsum.v), B, T, E, sp(lib)) == 0
    de_ref, dv_ref, _ = rr.att_ctx_bwd(dctx, dw_ext, w32, v, scaling)
    wd_ = w32.double()
    s_dw = torch.einsum("bte,be->bt", v.double().abs(), dctx.double().abs()) + dw_ext.double().abs()
    s_de = scaling * wd_ * (s_dw + (wd_ * s_dw).sum(1, keepdim=True))
    check("ATT_DE_TOL", name + " de", de.v, de_ref, s_de + TINY)
    check("ATT_DENC_TOL", name + " d_v", d_v.v, dv_ref, wd_.unsqueeze(2) * dctx.double().abs().unsqueeze(1) + TINY, n_terms=1)
    check("DOT_DSUM_TOL", name + " dsum", dsum.v, dsum.v0, (2 * s_de.sum() + TINY).reshape(1))
    assert_zero_value(name + " masked de == 0", de.v[masked])
    de32 = de.v.cpu()
    dk, dq = Out(B, T, A), Acc(B, A, seed=T)
    for _ in range(2):
        assert L.eamd_att_dot_energy_bwd(p(de.v), p(kd), p(qd), p(dk.v), p(dq.v), B, T, A, sp(lib)) == 0
    dk_ref, dq_ref = rr.att_dot_energy_bwd(de32, k, q)
    check("DOT_DK_TOL", name + " dk", dk.v, dk_ref, dk_ref.abs() + TINY, n_terms=1)
    check("DOT_DQ_TOL", name + " dq", dq.v, dq.v0 + 2 * dq_ref, dq.v0.abs() + 2 * rr.att_dot_energy_bwd(de32.abs(), k.abs(), q)[1],
          n_terms=2 * T + 2 * cdiv(T, 8) + 1)
    for o in (e, w, ctx, de, d_v, dsum, dk, dq):
        o.guards(name)


def test_att_ctx_refusals(lib):
    """T = 15361: EAMD_EUNSUPPORTED before any launch, outputs keep the fill"""
    L, p = lib.lib(), lib.ptr
    B, T, E = 1, 15361, 1
    z = torch.zeros(T, device=DEV)
    w, ctx, de, d_v, dsum = Out(B, T), Out(B, E), Out(B, T), Out(B, T, E), Out(1)
    assert L.eamd_att_ctx_fwd(p(z), p(z), 1.0, p(w.v), p(ctx.v), B, T, E, sp(lib)) == EUNSUPPORTED
    assert L.eamd_att_ctx_bwd(p(z), None, p(z), p(z), 1.0, p(de.v), p(d_v.v), p(dsum.v), B, T, E, sp(lib)) == EUNSUPPORTED
    for o in (w, ctx, de, d_v, dsum):
        o.untouched("refused att_ctx T=15361")


# =============================================================================================
# i. persistent whole-sequence LSTM
# =============================================================================================
def seq_fwd_variant(njobs, B, H, cus):
    """the tile chooser of eamd_lstm_seq_fwd -> (MT, NT, KQ), or None where it answers EAMD_EUNSUPPORTED"""
    if H % 64 != 0 or B > 64:
        return None
    kq = next((c for c in (1, 2, 4) if H % (16 * c) == 0 and H // (16 * c) <= 16), None)
    if kq is None:
        return None
    nw = H // (16 * kq)
    best, pick = 0, None
    for m in (1, 2, 4):
        for n in (4, 2, 1):
            if H % (4 * n) != 0 or 16 * m * 4 * n > 64 * nw:
                continue
            if m > 1 and 16 * (m // 2) >= B:
                continue
            wgs = njobs * (H // (4 * n)) * cdiv(B, 16 * m)
            if wgs > cus or wgs > 960 or H // (4 * n) > 256:
                continue
            if wgs > best:
                best, pick = wgs, (m, n, kq)
    return pick


def seq_bwd_variant(njobs, B, H, cus):
    """eamd_lstm_seq_bwd -> KQ, or None"""
    if H % 64 != 0 or B > 64:
        return None
    K = 4 * H
    kq = next((c for c in (1, 2, 4, 8, 16) if K % (16 * c) == 0 and K // (16 * c) <= 16), None)
    if kq is None or K // (16 * kq) < 4:
        return None
    wgs = njobs * (H // 16) * cdiv(B, 16)
    if wgs > cus or wgs > 960 or H // 16 > 256:
        return None
    return kq


# (njobs, B, H): one small shape per forward instantiation reachable at 256 compute units, in the order
# (1,1,1) (1,1,2) (1,1,4) (1,2,1) (1,2,2) (1,2,4) (1,4,2) (1,4,4) (2,1,1) (2,1,2) (2,2,2) (2,2,4)
# and (2, 5, 128) for the backward KQ = 2, which none of them reaches
SEQ_SHAPES = [(1, 1, 64), (1, 1, 320), (1, 1, 576), (2, 49, 192), (2, 17, 320), (2, 1, 576), (2, 49, 320), (2, 17, 576),
              (2, 33, 192), (1, 33, 384), (2, 33, 384), (1, 33, 704), (2, 5, 128)]
SEQ_VARIANTS_256 = [(1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 2, 1), (1, 2, 2), (1, 2, 4), (1, 4, 2), (1, 4, 4), (2, 1, 1), (2, 1, 2),
                    (2, 2, 2), (2, 2, 4), (1, 1, 1)]
SEQ_BWD_KQ = {64: 1, 128: 2, 192: 4, 320: 8, 576: 16}


def device_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def seq_scales_fwd(gx, w, b, live, reverse, acts, c, h):
    """first-order scales of every step's acts, c, h given the float64 reference (state errors carried along the walk)"""
    T, B, H4 = gx.shape
    H = H4 // 4
    wa = w.double().abs()
    s_hp, s_cp = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
    cp = torch.zeros(B, H, dtype=torch.float64)
    sa, sc, sh = [None] * T, [None] * T, [None] * T
    for s in range(T):
        t = T - 1 - s if reverse else s
        S = gx[t].double().abs() + (b.double().abs() if b is not None else 0) + s_hp @ wa.t()
        lv = torch.ones(B, 1, dtype=torch.bool) if live is None else live[t].reshape(B, 1) != 0
        # the would-be cell value of a dead row is not kept: scales from the kept state
        i, f, g, o = acts[t].reshape(B, 4, H).unbind(1)
        c_live = f * cp + i * g
        a_s, c_s, h_s = lstm_fwd_scales(acts[t], cp, c_live, S, s_cp)
        sa[t] = a_s
        s_cp = torch.where(lv, c_s, s_cp + TINY)
        s_hp = torch.where(lv, h_s, s_hp + TINY)
        sc[t], sh[t] = s_cp, s_hp
        cp = c[t]
    return torch.stack(sa), torch.stack(sc), torch.stack(sh)


def seq_scales_bwd(dy, w, acts, c, live, reverse):
    T, B, H = c.shape
    wa = w.double().abs()
    s_dg, s_dc, s_pass = None, torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
    out = [None] * T
    for s in range(T):
        t = s if reverse else T - 1 - s
        pt = t + 1 if reverse else t - 1
        cp = c[pt].double() if 0 <= pt < T else torch.zeros(B, H, dtype=torch.float64)
        s_dh = s_pass + (s_dg @ wa if s_dg is not None else 0)
        lv = torch.ones(B, 1, dtype=torch.bool) if live is None else live[t].reshape(B, 1) != 0
        g_s, dcp_s = lstm_bwd_scales(dy[t], s_dh, s_dc, acts[t].double(), cp, c[t].double())
        s_dg = torch.where(lv, g_s, torch.zeros_like(g_s))
        s_dc = torch.where(lv, dcp_s, s_dc)
        s_pass = torch.where(lv, torch.zeros_like(s_dh), s_dh)
        out[t] = s_dg + TINY
    return torch.stack(out)


@pytest.mark.parametrize("idx", range(len(SEQ_SHAPES)), ids=[f"{j}x{b}x{h}" for j, b, h in SEQ_SHAPES])
def test_lstm_seq_vs_float64(ops, lib, idx):
    """ops.lstm_seq_fwd / _bwd with NaN-filled outputs: y, the state h / c after every step (the final state among them), acts
    and dgates of every step against the float64 sequence restatement; the chooser's variant is asserted; the status word
    is 0; a second launch is bit-identical; dead rows are bit-exact.  These kernels wait on flags between workgroups: each
    launch runs as it is, nothing loops or retries."""
    njobs, B, H = SEQ_SHAPES[idx]
    cus = device_cus()
    if not ops.lstm_seq_ok(njobs, B, H):
        print(f"[rnn] lstm_seq {njobs}x{B}x{H}: not admitted by ops.lstm_seq_ok at {cus} compute units")
        pytest.skip(f"lstm_seq_ok declines {njobs}x{B}x{H} at {cus} compute units")
    fv, bv = seq_fwd_variant(njobs, B, H, cus), seq_bwd_variant(njobs, B, H, cus)
    assert fv is not None and bv is not None
    if cus == 256:
        assert fv == SEQ_VARIANTS_256[idx], f"{njobs}x{B}x{H}: forward variant {fv}"
    assert bv == SEQ_BWD_KQ.get(H, bv)
    T = 3 if idx % 2 == 0 else 5
    masked = idx % 3 != 1
    print(f"[rnn] lstm_seq {njobs}x{B}x{H} T={T} masked={masked}: forward (MT,NT,KQ)={fv}, backward KQ={bv}, {cus} compute units")
    g = gen(idx * 101 + H)
    jobs = []
    for j in range(njobs):
        reverse = (j == 1) if njobs == 2 else (idx % 4 >= 2)
        gx = torch.randn(T, B, 4 * H, generator=g)
        w = torch.randn(4 * H, H, generator=g) / math.sqrt(H)
        b = torch.randn(4 * H, generator=g) * 0.5 if (idx + j) % 2 == 0 else None
        live = None
        if masked:
            lens = torch.randint(1, T + 1, (B,), generator=g)
            lens[0], lens[B - 1] = T, 1
            live = (torch.arange(T).unsqueeze(1) < lens.unsqueeze(0)).to(U8)
        dy = torch.randn(T, B, H, generator=g)
        jobs.append(dict(gx=gx, w=w, b=b, live=live, reverse=reverse, dy=dy,
                         d={k: dev(v) for k, v in dict(gx=gx, w=w, b=b, live=live, dy=dy, w_t=w.t().contiguous()).items()}))
    assert njobs == 1 or {jb["reverse"] for jb in jobs} == {False, True}

    def run_fwd():
        outs = [dict(h=Out(T, B, H), c=Out(T, B, H), y=Out(T, B, H), acts=Out(T, B, 4 * H)) for _ in jobs]
        ops.lstm_seq_fwd([(jb["d"]["gx"], jb["d"]["w"], jb["d"]["b"], jb["d"]["live"], o["h"].v, o["c"].v, o["y"].v, o["acts"].v,
                           jb["reverse"]) for jb, o in zip(jobs, outs)], T, B, H)
        assert ops.lstm_seq_status() == 0
        return outs

    f1 = run_fwd()
    f2 = run_fwd()
    for j, (jb, o, o2) in enumerate(zip(jobs, f1, f2)):
        name = f"lstm_seq_fwd {njobs}x{B}x{H} {fv} job {j} reverse={jb['reverse']}"
        y_ref, h_ref, c_ref, a_ref = rr.lstm_seq_fwd(jb["gx"], jb["w"], jb["b"], jb["live"], jb["reverse"])
        s_a, s_c, s_h = seq_scales_fwd(jb["gx"], jb["w"], jb["b"], jb["live"], jb["reverse"], a_ref, c_ref, h_ref)
        check("SEQ_FWD_TOL", name + " acts", o["acts"].v, a_ref, s_a)
        check("SEQ_FWD_TOL", name + " c", o["c"].v, c_ref, s_c)
        check("SEQ_FWD_TOL", name + " h", o["h"].v, h_ref, s_h)
        check("SEQ_FWD_TOL", name + " y", o["y"].v, y_ref, s_h)
        for k in ("h", "c", "y", "acts"):
            o[k].guards(name + " " + k)
            assert_bits(name + f" second launch {k}", o2[k].v, o[k].v.cpu())
        if jb["live"] is not None:
            dead = jb["live"] == 0
            assert bool(dead.any())
            assert_zero_bits(name + " dead y == +0", o["y"].v[dead])
            hc, cc = o["h"].v.cpu(), o["c"].v.cpu()
            for s in range(T):
                t = T - 1 - s if jb["reverse"] else s
                tp = t + 1 if jb["reverse"] else t - 1
                hp = hc[tp] if 0 <= tp < T else torch.zeros(B, H)
                cp = cc[tp] if 0 <= tp < T else torch.zeros(B, H)
                assert_bits(name + f" dead h carried at frame {t}", hc[t][dead[t]], hp[dead[t]])
                assert_bits(name + f" dead c carried at frame {t}", cc[t][dead[t]], cp[dead[t]])

    def run_bwd():
        outs = [Out(T, B, 4 * H) for _ in jobs]
        ops.lstm_seq_bwd([(jb["d"]["dy"], jb["d"]["w_t"], f["acts"].v, f["c"].v, jb["d"]["live"], o.v, jb["reverse"])
                          for jb, f, o in zip(jobs, f1, outs)], T, B, H)
        assert ops.lstm_seq_status() == 0
        return outs

    b1 = run_bwd()
    b2 = run_bwd()
    for j, (jb, f, o, o2) in enumerate(zip(jobs, f1, b1, b2)):
        name = f"lstm_seq_bwd {njobs}x{B}x{H} KQ={bv} job {j} reverse={jb['reverse']}"
        acts32, c32 = f["acts"].v.cpu(), f["c"].v.cpu()
        dg_ref = rr.lstm_seq_bwd(jb["dy"], jb["w"], acts32, c32, jb["live"], jb["reverse"])
        check("SEQ_BWD_TOL", name + " dgates", o.v, dg_ref, seq_scales_bwd(jb["dy"], jb["w"], acts32, c32, jb["live"], jb["reverse"]))
        o.guards(name)
        assert_bits(name + " second launch", o2.v, o.v.cpu())
        if jb["live"] is not None:
            assert_zero_bits(name + " dead dgates == +0", o.v[jb["live"] == 0])


def test_lstm_seq_variant_coverage(ops):
    """the forward instantiations the shapes above reach == the ones reachable over every (njobs <= 2, B <= 64, H <= 1024)
    that ops.lstm_seq_ok admits on this device; likewise the backward KQ"""
    cus = device_cus()
    reach_f, reach_b = {}, {}
    for njobs in (1, 2):
        for B in range(1, 65):
            for H in range(64, 1025, 64):
                if ops.lstm_seq_ok(njobs, B, H):
                    fv, bv = seq_fwd_variant(njobs, B, H, cus), seq_bwd_variant(njobs, B, H, cus)
                    assert fv is not None and bv is not None, f"lstm_seq_ok admits {njobs}x{B}x{H}, the chooser does not"
                    reach_f.setdefault(fv, (njobs, B, H))
                    reach_b.setdefault(bv, (njobs, B, H))
    admitted = [s for s in SEQ_SHAPES if ops.lstm_seq_ok(*s)]
    seen_f = {seq_fwd_variant(*s, cus) for s in admitted}
    seen_b = {seq_bwd_variant(*s, cus) for s in admitted}
    every = {(m, n, k) for m in (1, 2, 4) for n in (1, 2, 4) for k in (1, 2, 4)}
    print(f"[rnn] lstm_seq at {cus} compute units: reachable forward (MT,NT,KQ) {sorted(reach_f)}; never reached {sorted(every - set(reach_f))}; "
          f"reachable backward KQ {sorted(reach_b)}")
    if cus == 256:
        assert sorted(reach_f) == sorted(set(SEQ_VARIANTS_256))
        assert not any(m == 4 for m, _, _ in reach_f)
    assert seen_f == set(reach_f), f"forward variants not exercised: {sorted(set(reach_f) - seen_f)} (e.g. {[reach_f[v] for v in sorted(set(reach_f) - seen_f)]})"
    assert seen_b == set(reach_b), f"backward KQ not exercised: {sorted(set(reach_b) - seen_b)}"
