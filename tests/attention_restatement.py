"""The fused attention launches of csrc/attn_f32.hip and csrc/attn_fused.hip (shared code: csrc/attn_common.h), restated stage by
stage in float64: what each launch computes from the values it is given, the per-element magnitudes its rounding errors scale
with, and which kernel instantiation a shape is dispatched to.  Test infrastructure only - the product tree never imports it,
and no GPU is involved.

Layouts are the kernels': operands are [B, T, H, dk] (heads side by side in a row), positions [T2, H, dk], and the score-shaped
tensors P / Pd / dS / dbd are [H, B, T1, T2] (pair z = h * B + b; the kernels' rows have ldp >= T2 columns, the pad is zero).

Forward (one launch):   ac = qu k^T;  with positions bd = qv pos^T moved by the legacy rel_shift taken over Ts (attn_common.h: the
                        forward map shift_dst and its inverse attn_shift_src = shift_src; zero outside the Ts x Ts square and on
                        query rows >= Ts);  s = scale (ac + shifted bd), -inf at masked keys;  P = softmax(s), zeros on a fully
                        masked row;  Pd = keep P inv with keep = dropout_restatement.keep_mask indexed by the element's position in
                        the [H, B, T1, ldp] tensor;  ctx = Pd v.
Query-side backward:    dP = (dctx v^T) keep inv;  dS = scale P (dP - rowsum(P dP));  dbd = the inverse scatter of dS (zero outside
                        the square, zero at the head of row 0);  dq = dS k.
Key side:               dv = Pd^T dctx;  dk = dS^T qu;  dpos += sum_b dbd^T qv.

Error magnitudes, with u = 2^-23 (the tests multiply them by the ceilings named below):
  * a contraction that only multiplies and adds in fp32 sits under (K + 8) u of sum |a| |b|         (contract() returns both)
  * P sits under p (2 delta_i + (T2 + 16) u), delta_i = (dk + 8) u max over the live keys of row i of scale sum |q| |k|
    (both score terms with positions)                                                                (forward()["P_bound"])
  * dS sits under (dk + T2 + 16) u of scale p (A + sum_j p A), A = inv keep sum |dctx| |v| the magnitude of dP: the dP ceiling
    (dk + 8) u A carried through scale p (|dP| + sum p |dP|), plus the T2 + 8 additions of the row sum  (backward_q()["dS_mag"])
"""
import torch

import dropout_restatement as dr

ATT_DK = 64
ATT_MAXK = 512            # keys per row of the short kernels
ATT_LONG_MAXK = 4096      # of the long-row kernels
ATT_PLD = 68              # row stride (floats) of a tile buffer in LDS
U23 = 2.0 ** -23


# ---- dispatch (attn_common.h: attn_nkt, attn_long_lds; attn_f32.hip: long_geom, launch_fwd_long, launch_bwd_long) ---------------
def attn_nkt(T2):
    return 8 if T2 <= 128 else 16 if T2 <= 256 else 32


def attn_long_lds(lq, nw, nkt):
    return (lq * (nkt * 16 + 4) + nw * 16 * ATT_PLD + 2 * nw * lq) * 4


def long_geom(T2):
    nkt = (T2 + 15) // 16
    lq, nw = 16, 4
    if attn_long_lds(16, 4, nkt) > 160 * 1024:
        lq = 8
    if attn_long_lds(lq, 4, nkt) > 80 * 1024:
        nw = 8 if attn_long_lds(lq, 8, nkt) <= 160 * 1024 else 6 if attn_long_lds(lq, 6, nkt) <= 160 * 1024 else 4
    return lq, nw


def route(dtype, rel, T1, T2):
    """(forward instantiation, query-side backward instantiation) of eamd_attn_fwd[_f32] / eamd_attn_bwd_q[_f32] for storage type
    dtype ("f32" | "bf16").  The short backward kernels have no REL parameter (dbd is a run-time pointer); the name keeps `rel`
    because the scatter is its own code path.  The long backward runs four waves where the forward runs six."""
    assert dtype in ("f32", "bf16") and 1 <= T2 <= ATT_LONG_MAXK and T1 >= 1 and (not rel or T1 == T2)
    r = "rel" if rel else "abs"
    if T2 <= ATT_MAXK:
        n = attn_nkt(T2)
        return f"short_{dtype}_fwd<{r},nkt={n}>", f"short_{dtype}_bwd_q<{r},nkt={n}>"
    lq, nw = long_geom(T2)
    return f"long_{dtype}_fwd<{r},lq={lq},nw={nw}>", f"long_{dtype}_bwd_q<{r},lq={lq},nw={8 if nw == 8 else 4}>"


def route_kv(dtype, rel):
    """the key-side launch: eamd_attn_bwd_kv (bf16), eamd_attn_bwd_kv_f32 without / with dbd, qv and dpos"""
    assert dtype in ("f32", "bf16") and not (rel and dtype == "bf16")
    return f"kv_{dtype}<{'rel' if rel else 'abs'}>"


def all_routes():
    """every instantiation an admissible shape can reach"""
    out = set()
    for dtype in ("f32", "bf16"):
        for rel in (False, True):
            for T2 in range(1, ATT_LONG_MAXK + 1):
                out.update(route(dtype, rel, T2, T2))
        out.add(route_kv(dtype, False))
    out.add(route_kv("f32", True))
    return out


# ---- the legacy rel_shift over Ts (attn_common.h:96-127) -----------------------------------------------------------------------
def shift_dst(i, m, Ts):
    """forward map as the forward kernels write it at their stores: bd[i][m] -> shifted[row][j], or None where the guard
    m < Ts && i < Ts && row >= 0 drops it"""
    lim = Ts - 1 - i
    row, j = (i, m - lim) if m >= lim else (i - 1, m + i + 1)
    return (row, j) if (m < Ts and i < Ts and row >= 0) else None


def shift_src(i, j, Ts):
    """attn_shift_src: shifted[i][j] (i, j < Ts) is column c of row R of [0 | bd]: bd[R][c - 1], or the zero column (c == 0)"""
    return (i, Ts + j - i) if j <= i else (i + 1, j - i - 1)


def _src_grid(T, Ts):
    i = torch.arange(T).view(T, 1).expand(T, T)
    j = torch.arange(T).view(1, T).expand(T, T)
    low = j <= i
    R = torch.where(low, i, i + 1)
    c = torch.where(low, Ts + j - i, j - i - 1)
    valid = (i < Ts) & (j < Ts) & (c != 0)
    return i, j, R, c, valid


def rel_shift(bd, Ts):
    """[..., T, T] -> the shifted term: zero outside the Ts x Ts square, on rows >= Ts and where the zero column lands"""
    T = bd.shape[-1]
    _, _, R, c, valid = _src_grid(T, Ts)
    out = bd[..., R.clamp(max=T - 1), (c - 1).clamp(0, T - 1)]
    return torch.where(valid, out, torch.zeros((), dtype=bd.dtype))


def rel_unshift(g, Ts):
    """the inverse scatter of a gradient of the shifted term: dbd [..., T, T]"""
    T = g.shape[-1]
    i, j, R, c, valid = _src_grid(T, Ts)
    out = torch.zeros_like(g)
    out[..., R[valid], c[valid] - 1] = g[..., i[valid], j[valid]]
    return out


# ---- stages ------------------------------------------------------------------------------------------------------------------
def keep_tensor(step, salt, p, H, B, T1, T2, ldp):
    """bool [H, B, T1, T2]: the attention-dropout mask of a launch whose P rows have ldp columns"""
    m = dr.keep_mask(step, salt, H * B * T1 * ldp, p)
    return torch.from_numpy(m).view(H, B, T1, ldp)[..., :T2]


def drop_inv(p):
    return float(dr.drop_inv(dr.drop_thr16(p)))


def live_of(mask, B, T1, T2):
    """mask: None or integer [1 | B, 1 | T1, T2], any non-zero byte is live -> bool [1, B, T1, T2]"""
    if mask is None:
        return torch.ones(1, B, T1, T2, dtype=torch.bool)
    return (mask != 0).expand(B, T1, T2).unsqueeze(0)


def forward(qu, k, scale, qv=None, pos=None, mask=None, Ts=None, dk_ceiling=ATT_DK):
    """-> dict(s, P, P_bound, live).  qu / qv [B, T1, H, dk], k [B, T2, H, dk], pos [T2, H, dk], all float64"""
    B, T1, H, _ = qu.shape
    T2 = k.shape[1]
    s = torch.einsum("bihd,bjhd->hbij", qu, k)
    mag = torch.einsum("bihd,bjhd->hbij", qu.abs(), k.abs())
    if pos is not None:
        Ts = T2 if Ts is None else Ts
        s = s + rel_shift(torch.einsum("bihd,jhd->hbij", qv, pos), Ts)
        mag = mag + rel_shift(torch.einsum("bihd,jhd->hbij", qv.abs(), pos.abs()), Ts)
    live = live_of(mask, B, T1, T2)
    s = torch.where(live, s * scale, torch.full((), float("-inf"), dtype=s.dtype))
    mx = s.max(dim=-1, keepdim=True).values
    dead = torch.isinf(mx)
    e = torch.where(dead, torch.zeros_like(s), torch.exp(s - torch.where(dead, torch.zeros_like(mx), mx)))
    den = e.sum(dim=-1, keepdim=True)
    P = e / torch.where(dead, torch.ones_like(den), den)
    delta = (dk_ceiling + 8) * U23 * torch.where(live, mag * abs(scale), torch.zeros_like(mag)).max(dim=-1, keepdim=True).values
    return dict(s=s, P=P, P_bound=P * (2 * delta + (T2 + 16) * U23), live=live.expand(H, B, T1, T2))


def contract(spec, a, b):
    """-> (einsum(a, b), einsum(|a|, |b|)): a product and the magnitude its (K + 8) u ceiling multiplies"""
    return torch.einsum(spec, a, b), torch.einsum(spec, a.abs(), b.abs())


def context(Pd, v):
    """ctx [B, T1, H, dk] = Pd v"""
    return contract("hbij,bjhd->bihd", Pd, v)


def backward_q(dctx, v, P, scale, keep=None, inv=1.0, Ts=None, rel=False):
    """-> dict(dP, dS, dS_mag, dbd).  P [H, B, T1, T2] as the launch reads it; keep bool of that shape or None"""
    dP, A = contract("bihd,bjhd->hbij", dctx, v)
    if keep is not None:
        dP, A = dP * keep * inv, A * keep * inv
    dS = scale * P * (dP - (P * dP).sum(dim=-1, keepdim=True))
    dS_mag = abs(scale) * P.abs() * (A + (P.abs() * A).sum(dim=-1, keepdim=True))
    dbd = rel_unshift(dS, dS.shape[-1] if Ts is None else Ts) if rel else None
    return dict(dP=dP, dS=dS, dS_mag=dS_mag, dbd=dbd)


def dq_of(dS, k):
    return contract("hbij,bjhd->bihd", dS, k)


def key_side(Pd, dS, dctx, qu, dbd=None, qv=None):
    """-> dict(dv, dv_mag, dk, dk_mag[, dpos, dpos_mag]): dv / dk [B, T2, H, dk], dpos [T2, H, dk] (the sum the launch ADDS)"""
    out = {}
    out["dv"], out["dv_mag"] = contract("hbij,bihd->bjhd", Pd, dctx)
    out["dk"], out["dk_mag"] = contract("hbij,bihd->bjhd", dS, qu)
    if dbd is not None:
        out["dpos"], out["dpos_mag"] = contract("hbij,bihd->jhd", dbd, qv)
    return out
