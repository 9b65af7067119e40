"""The memory-linear attention forward (csrc/attn_stream.hip, ops.attn_fwd_stream) element by element against the float64
restatement tests/attention_restatement.py, and the attention block that reaches it without autograd.  Operands are column
blocks of NaN-filled buffers and ctx sits inside one: everything outside its extent must still be NaN.  q is amplified so that
the scaled scores span about +-30; a planted direction puts the row maximum on key 0 for odd queries, on the last key for even.
Per element |got - ref| <= c * ceiling, ceiling = sum_j P_bound_ij |v_j| + (nlive_i + ntiles + 8) 2^-23 sum_j P_ij |v_j| from the
restatement's own terms (ntiles = ceil(T2 / KT) rescale multiplications); a bf16 output must be the RNE rounding of a value
within that distance (the rule of test_gpu_attention_kernels.py:106-134)."""
import functools
import math

import pytest
import torch

import attention_restatement as ar

pytestmark = pytest.mark.gpu

DEV, DK, U23, TINY = "cuda", 64, 2.0 ** -23, 2.0 ** -114
BF16, F32 = torch.bfloat16, torch.float32
QB, KT = 64, 32                      # ops.ATTN_STREAM_QB / ATTN_STREAM_KT (asserted below): the shapes are written against them
TOL_STREAM_F32 = 0.0147              # attn_stream_kernel<float>     observed 3.690e-3
TOL_STREAM_BF16 = 0.0052             # attn_stream_kernel<bf16_t>    observed 1.318e-3
MASKS = [None, "len", "causal", "dead_row", "tiles"]
# (B, H, T1, T2, rel, shift_len)
SHAPES = [(2, 2, 1, 1, True, None), (2, 2, 17, 17, True, None),
          (2, 2, 63, 63, True, None),          # QB - 1
          (2, 2, 65, 65, True, None),          # QB + 1 = 2 KT + 1
          (2, 2, 101, 101, True, None),        # 3 KT + 5
          (2, 2, 101, 101, True, 94),          # shift_len = T - 7, keys >= Ts masked
          (2, 2, 1, 101, False, None),         # (1, 3 KT + 5): cached decoding
          (2, 2, 67, 31, False, None),         # (QB + 3, KT - 1)
          (2, 2, 5, 64, False, None)]          # (5, 2 KT)
CASES = [s + (m,) for s in SHAPES for m in MASKS if not (s[5] is not None and m != "len")] + [(1, 1, 4100, 4100, True, None, None)]


def make_mask(kind, B, T1, T2, Ts):
    """uint8 [1 | B, 1 | T1, T2] or None"""
    j = torch.arange(T2)
    if kind is None:
        return None
    if kind == "len":            # key padding, another length per batch entry, nothing live from Ts on
        lens = torch.linspace(Ts, max(1, Ts // 2), B).long()
        return (j[None, :] < lens[:, None]).to(torch.uint8).view(B, 1, T2)
    if kind == "causal":
        lim = (torch.arange(T1) * (T2 - 1)) // max(T1 - 1, 1)
        return (j[None, :] <= lim[:, None]).to(torch.uint8).view(1, T1, T2).contiguous()
    m = torch.ones(B, T1, T2, dtype=torch.uint8)
    if kind == "dead_row":       # one fully masked row
        m[0, T1 // 2] = 0
        return m
    m = torch.ones(1, 1, T2, dtype=torch.uint8)      # "tiles": the first key tile and a middle one masked for every row
    m[..., :KT] = 0
    ntiles = -(-T2 // KT)
    if ntiles >= 3:
        m[..., ntiles // 2 * KT:(ntiles // 2 + 1) * KT] = 0
    return m


@functools.lru_cache(maxsize=None)
def case(B, H, T1, T2, rel, ts, mask):
    """inputs (bf16-exact fp32 values) and the float64 reference with its ceiling, once per case for both storage types"""
    D = H * DK
    g = torch.Generator().manual_seed(T1 * 131 + T2 * 7 + B)
    rnd = lambda rows: (0.5 * torch.randn(rows, D, generator=g)).to(BF16).float()
    w = torch.where(torch.rand(D, generator=g) < 0.5, -0.5, 0.5)
    sgn = torch.where(torch.arange(B * T1) % T1 % 2 == 1, 1.0, -1.0)[:, None]
    qu, k, v = (32.0 * rnd(B * T1) + 16.0 * sgn * w).to(BF16).float(), rnd(B * T2), rnd(B * T2)
    k.view(B, T2, D)[:, 0], k.view(B, T2, D)[:, T2 - 1] = w, -w
    qv, pos = ((32.0 * rnd(B * T1)).to(BF16).float(), rnd(T2)) if rel else (None, None)
    Ts = T2 if ts is None else ts
    m8 = make_mask(mask, B, T1, T2, Ts)
    f64 = lambda t, T: t.double().view(B, T, H, DK)
    f = ar.forward(f64(qu, T1), f64(k, T2), 1.0 / math.sqrt(DK), f64(qv, T1) if rel else None,
                   pos.double().view(T2, H, DK) if rel else None, m8, Ts)
    ref, mag = ar.context(f["P"], f64(v, T2))
    nlive = f["live"].sum(-1).permute(1, 2, 0).unsqueeze(-1)                              # [B, T1, H, 1]
    bound = ar.context(f["P_bound"], f64(v, T2).abs())[0] + (nlive + -(-T2 // KT) + 8) * U23 * mag
    dead = ~f["live"].any(-1).permute(1, 2, 0)                                            # [B, T1, H]
    return dict(qu=qu, qv=qv, k=k, v=v, pos=pos, m8=m8, ref=ref.reshape(B * T1, D), bound=bound.reshape(B * T1, D) + TINY,
                dead=dead.reshape(B * T1, H))


def place(dt, ld, *cols):
    """(tensor, element offset, row stride) views of column blocks (offset, values) inside one NaN-filled [rows + 2, ld] buffer"""
    flat = torch.full((cols[0][1].shape[0] + 2, ld), float("nan"), dtype=dt, device=DEV)
    for off, x in cols:
        flat[1:-1, off:off + x.shape[1]] = x.to(dt)
    return [(flat, ld + off, ld) for off, _ in cols]


def compare(name, tolname, got, ref, bound):
    """max |got - ref| / bound, printed and asserted (bf16: the distance from ref to the nearest value that rounds to got)"""
    tol = min(globals()[tolname], 1.0)
    g = got.double().cpu()
    assert bool(torch.isfinite(g).all()), f"{name}: the output is not finite"
    d = (g - ref).abs()
    if got.dtype == BF16:
        d = (d - torch.where(g == 0, torch.zeros_like(g), torch.exp2(torch.floor(torch.log2(g.abs().clamp(min=TINY))) - 8))).clamp(min=0)
        rne = lambda x: x.float().to(BF16).double()
        assert bool(((g >= rne(ref - tol * bound)) & (g <= rne(ref + tol * bound))).all()), f"{name}: not the bf16 rounding of a value within {tolname}"
    worst = float((d / bound).max())
    print(f"[attn_stream] {name}: max err/ceiling {worst:.3e} (constant {tolname} = {tol:g})")
    assert worst <= tol, f"{name}: error/ceiling {worst:.3e} > {tolname} = {tol:g}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,H,T1,T2,rel,ts,mask", CASES, ids=lambda x: str(x))
def test_kernel_against_float64(dtype, B, H, T1, T2, rel, ts, mask):
    from espnet_amd import ops
    assert (ops.ATTN_STREAM_QB, ops.ATTN_STREAM_KT) == (QB, KT)
    c = case(B, H, T1, T2, rel, ts, mask)
    dt, D = {"f32": F32, "bf16": BF16}[dtype], H * DK
    if T1 == T2:
        q3, k3, v3 = place(dt, 3 * D + 8, (0, c["qu"]), (D, c["k"]), (2 * D, c["v"]))
    else:
        (q3,), (k3, v3) = place(dt, D + 8, (0, c["qu"])), place(dt, 2 * D + 8, (0, c["k"]), (D, c["v"]))
    qv3, p3 = (place(dt, D + 8, (0, c["qv"]))[0], place(dt, D + 16, (8, c["pos"]))[0]) if rel else (None, None)
    mdev = None if c["m8"] is None else c["m8"].to(DEV)
    tsd = None if ts is None else torch.tensor([ts], dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        cflat = torch.full((B * T1 + 2, D + 12), float("nan"), dtype=dt, device=DEV)
        r = ops.attn_fwd_stream(q3, qv3, k3, v3, p3, mdev, B, T1, T2, H, DK, scale=1.0 / math.sqrt(DK), shift_len=tsd,
                                out=(cflat, D + 12 + 4, D + 12))
        assert r is cflat, "the library declined the operands"
        torch.cuda.synchronize()
        outs.append(cflat.clone())
    name = f"{dtype} B{B} H{H} {T1}x{T2} {'rel' if rel else 'abs'} ts={ts} mask={mask}"
    bits = torch.int16 if dt == BF16 else torch.int32
    assert torch.equal(outs[0].view(bits), outs[1].view(bits)), f"{name}: two launches differ"
    guard = torch.ones_like(cflat, dtype=torch.bool)
    guard[1:-1, 4:4 + D] = False
    assert bool(torch.isnan(cflat[guard]).all()), f"{name}: ctx was written outside its extent"
    got = cflat[1:-1, 4:4 + D]
    assert bool((got.reshape(B * T1, H, DK)[c["dead"].to(DEV)] == 0).all()), f"{name}: a fully masked row is not exactly zero"
    compare(name, "TOL_STREAM_" + dtype.upper(), got, c["ref"], c["bound"])


def test_argument_checks_launch_nothing():
    from espnet_amd import _lib
    L = _lib.lib()
    assert (L.eamd_attn_stream_qb(), L.eamd_attn_stream_kt()) == (QB, KT)
    good = dict(qu=0x10000, ldq=256, qv=0x20000, ldqv=256, k=0x30000, ldk=256, v=0x40000, ldv=256, pos=0x50000, ldpos=256, mask=None,
                mb=0, mi=0, ctx=0x70000, ldc=256, B=2, H=4, T1=5000, T2=5000, dk=64, scale=0.125, shift_len=None, stream=None)
    for fn in (L.eamd_attn_fwd_stream, L.eamd_attn_fwd_stream_f32):        # made-up addresses: no row may be a valid call
        for change, code in ((dict(dk=32), -2), (dict(T1=90), -2), (dict(ctx=None), -1), (dict(qv=None), -1), (dict(ldk=258), -2)):
            assert fn(*dict(good, **change).values()) == code, change


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("bf16", 1e-2)])       # test_gpu_model.py's bounds for a layer output
def test_layers_agree_with_the_stored_path(prec, tol):
    """eval-mode Conformer EncoderLayer (rel-pos, D = 256, H = 4) and Transformer DecoderLayer (self + source attention, T1 != T2)
    under no_grad at T' = 70 on a padded batch: streamed (threshold 0) against the stored-P kernels (default threshold)"""
    import espnet_amd
    from espnet_amd import functional as F_
    from espnet_amd.nets import modules as M
    torch.manual_seed(3)
    ff = lambda act=None: M.PositionwiseFeedForward(256, 512, 0.0, act)  # noqa: E731
    enc = M.ConformerEncoderLayer(256, M.RelPositionMultiHeadedAttention(4, 256, 0.0), ff(M.Swish()), ff(M.Swish()),
                                  M.ConvolutionModule(256, 15, M.Swish()), 0.0).to(DEV).eval()
    dec = M.DecoderLayer(256, M.MultiHeadedAttention(4, 256, 0.0), M.MultiHeadedAttention(4, 256, 0.0), ff(), 0.0).to(DEV).eval()
    x, pos, tgt = torch.randn(2, 70, 256, device=DEV), torch.randn(1, 70, 256, device=DEV), torch.randn(2, 9, 256, device=DEV)
    xmask = M.make_non_pad_mask([70, 51]).unsqueeze(1)
    tmask = M.subsequent_mask(9).unsqueeze(0).expand(2, 9, 9).contiguous()
    espnet_amd.set_precision(prec)
    default, res = F_.ATTN_STREAM_KEYS, []
    try:
        for keys in (default, 0):
            F_.ATTN_STREAM_KEYS = keys
            with torch.no_grad():
                (y, _), _ = enc((x, pos), xmask)
                res.append((y, dec(tgt, tmask, y, xmask)[0]))
    finally:
        F_.ATTN_STREAM_KEYS = default
        espnet_amd.set_precision("fp32")
    for name, a, b in zip(("encoder layer", "decoder layer"), res[1], res[0]):
        e = float((a.double() - b.double()).norm() / b.double().norm())
        print(f"[attn_stream] {name} [{prec}] streamed vs stored: rel_l2 {e:.3e} (tol {tol:g})")
        assert e <= tol, (name, e)


@pytest.mark.parametrize("T,own", [(4608, None), (4100, 4000)])
def test_rel_pos_block_past_4096_keys(T, own):
    """one rel-pos mha_block (B = 1, D = 256, H = 4, fp32) under no_grad at the default threshold: the peak stays below ONE
    [H, T', T'] fp32 tensor (340 MB at 4608; the GEMM + softmax route allocates at least that, the streamed one ~40 MB), and a
    shape-bucketed batch (ops.time_bound set: its own length 4000 of 4100) is no longer refused"""
    from espnet_amd import ops
    from espnet_amd.nets import modules as M
    torch.manual_seed(5)
    norm, att = M.LayerNorm(256).to(DEV), M.RelPositionMultiHeadedAttention(4, 256, 0.0).to(DEV).eval()
    x, pos = torch.randn(1, T, 256, device=DEV), torch.randn(1, T, 256, device=DEV)
    mask = None if own is None else M.make_non_pad_mask([own], T).unsqueeze(1)
    ops.set_time_bound(None if own is None else torch.tensor([own], dtype=torch.int32, device=DEV))
    try:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            y = M.mha_block(norm, att, x, None, pos, mask)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    finally:
        ops.set_time_bound(None)
    print(f"[attn_stream] mha_block T'={T}: peak rise {rise / 2 ** 20:.1f} MB")
    assert bool(torch.isfinite(y[:, :own or T]).all()) and rise < 4 * T * T * 4
