"""Memory-linear attention training (csrc/attn_stream.hip with the row statistic, csrc/attn_stream_bwd.hip; ops.attn_fwd_stream(lse=),
ops.attn_bwd_stream) element by element against the float64 restatement tests/attention_restatement.py, and the attention blocks
that reach it with autograd.  Inputs, masks and the NaN-guarded buffers are those of test_gpu_attn_stream.py; the backward is fed
the ctx and lse its own forward wrote.  Per element |got - ref| <= c * ceiling with the ceilings of case(): the restatement's
magnitudes carried through dS = scale P (dP - delta), where delta = dctx . ctx inherits the forward's ctx ceiling and, in bf16
storage, the half-ulp 2^-9 |ctx| of the stored ctx.  bf16 outputs obey the RNE rule of test_gpu_attn_stream.compare."""
import functools
import math

import pytest
import torch

import attention_restatement as ar
from test_gpu_attn_stream import BF16, DEV, DK, F32, KT, TINY, U23, make_mask, place

pytestmark = pytest.mark.gpu

B, H, D, SCALE = 2, 2, 2 * DK, 1.0 / math.sqrt(DK)
# c per output and storage type: at most 4x the worst error/ceiling observed on the MI355X over the 90 cases (observed beside it)
TOL = {("lse", "f32"): 0.013, ("lse", "bf16"): 0.013,      # attn_stream_kernel<., false, true>     observed 3.253e-3, 3.253e-3
       ("dq", "f32"): 0.0008, ("dq", "bf16"): 0.7,         # stream_bwd_q_kernel                    observed 2.000e-4, 1.789e-1
       ("dk", "f32"): 0.0023, ("dk", "bf16"): 0.67,        # stream_bwd_kv_kernel                   observed 5.921e-4, 1.676e-1
       ("dv", "f32"): 0.021, ("dv", "bf16"): 0.010}        #                                        observed 5.455e-3, 2.581e-3
MASKS = [None, "len", "causal", "dead_row", "tiles"]
SHAPES = [(1, 1), (17, 17), (63, 63), (65, 65), (101, 101), (1, 101), (67, 31), (5, 64), (97, 130)]


@functools.lru_cache(maxsize=None)
def case(T1, T2, mask):
    """inputs (bf16-exact fp32 values) and the float64 references with their ceilings per storage type, once per case"""
    g = torch.Generator().manual_seed(T1 * 131 + T2 * 7 + B)
    rnd = lambda rows: (0.5 * torch.randn(rows, D, generator=g)).to(BF16).float()
    w = torch.where(torch.rand(D, generator=g) < 0.5, -0.5, 0.5)
    sgn = torch.where(torch.arange(B * T1) % T1 % 2 == 1, 1.0, -1.0)[:, None]
    qu, k, v, dctx = (32.0 * rnd(B * T1) + 16.0 * sgn * w).to(BF16).float(), rnd(B * T2), rnd(B * T2), rnd(B * T1)
    k.view(B, T2, D)[:, 0], k.view(B, T2, D)[:, T2 - 1] = w, -w
    m8 = make_mask(mask, B, T1, T2, T2)
    q64, k64, v64, d64 = (t.double().view(B, -1, H, DK) for t in (qu, k, v, dctx))
    f = ar.forward(q64, k64, SCALE, mask=m8)
    P, Pb = f["P"], f["P_bound"]
    dead = ~f["live"].any(-1)                                                             # [H, B, T1]
    lse = torch.where(dead, torch.zeros(()).double(), torch.logsumexp(f["s"], -1))
    c = dict(qu=qu, k=k, v=v, dctx=dctx, m8=m8, dead=dead.permute(1, 2, 0).reshape(B * T1, H), lse=lse.reshape(-1),
             lse_bound=(Pb.sum(-1) + 8 * U23 * lse.abs()).reshape(-1) + TINY)
    cx, cmag = ar.context(P, v64)
    nlive = f["live"].sum(-1).permute(1, 2, 0).unsqueeze(-1)
    cbound = ar.context(Pb, v64.abs())[0] + (nlive + -(-T2 // KT) + 8) * U23 * cmag      # the forward's ceiling on ctx
    bq = ar.backward_q(d64, v64, P, SCALE)
    A = ar.contract("bihd,bjhd->hbij", d64, v64)[1]
    ks = ar.key_side(P, bq["dS"], d64, q64)
    flat = lambda t, T: t.reshape(B * T, D)
    c["dv"] = (flat(ks["dv"], T2), flat(ar.key_side(Pb, bq["dS"], d64.abs(), q64)["dv"] + (T1 + 8) * U23 * ks["dv_mag"], T2) + TINY)
    for dt, half_ulp in (("f32", 0.0), ("bf16", 2.0 ** -9)):
        derr = (d64.abs() * (cbound + ((DK + 8) * U23 + half_ulp) * cx.abs())).sum(-1).permute(2, 0, 1).unsqueeze(-1)   # [H, B, T1, 1]
        dSb = (DK + T2 + 16) * U23 * bq["dS_mag"] + SCALE * (Pb * (A + (P * A).sum(-1, keepdim=True))
                                                               + P * ((Pb * A).sum(-1, keepdim=True) + derr))
        dq, dqm = ar.dq_of(bq["dS"], k64)
        c["dq", dt] = (flat(dq, T1), flat(ar.dq_of(dSb, k64.abs())[0] + (T2 + 8) * U23 * dqm, T1) + TINY)
        c["dk", dt] = (flat(ks["dk"], T2), flat(ar.key_side(P, dSb, d64, q64.abs())["dk"] + (T1 + 8) * U23 * ks["dk_mag"], T2) + TINY)
    c["dv", "f32"] = c["dv", "bf16"] = c.pop("dv")
    return c


def compare(name, what, dtype, got, ref, bound):
    """max |got - ref| / bound, printed and asserted (bf16: the distance from ref to the nearest value that rounds to got)"""
    tol = min(TOL[what, dtype], 1.0)
    g = got.double().cpu()
    assert bool(torch.isfinite(g).all()), f"{name}: {what} is not finite"
    d = (g - ref).abs()
    if got.dtype == BF16:
        d = (d - torch.where(g == 0, torch.zeros_like(g), torch.exp2(torch.floor(torch.log2(g.abs().clamp(min=TINY))) - 8))).clamp(min=0)
        rne = lambda x: x.float().to(BF16).double()
        assert bool(((g >= rne(ref - tol * bound)) & (g <= rne(ref + tol * bound))).all()), f"{name}: {what} is not the bf16 rounding of a value within its ceiling"
    worst = float((d / bound).max())
    print(f"[attn_stream_train] {name}: {what} {dtype} max err/ceiling {worst:.3e} (constant {tol:g})")
    assert worst <= tol, f"{name}: {what} error/ceiling {worst:.3e} > {tol:g}"


def guarded(dt, rows, ld, blocks):
    """one NaN-filled [rows + 2, ld] buffer, views of its column blocks at the given offsets, and the mask of what lies outside them"""
    flat = torch.full((rows + 2, ld), float("nan"), dtype=dt, device=DEV)
    outside = torch.ones_like(flat, dtype=torch.bool)
    for off in blocks:
        outside[1:-1, off:off + D] = False
    return flat, [(flat, ld + off, ld) for off in blocks], outside


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mask", MASKS, ids=str)
@pytest.mark.parametrize("T1,T2", SHAPES)
def test_kernels_against_float64(dtype, T1, T2, mask):
    from espnet_amd import ops
    c = case(T1, T2, mask)
    dt = {"f32": F32, "bf16": BF16}[dtype]
    if T1 == T2:
        q3, k3, v3 = place(dt, 3 * D + 8, (0, c["qu"]), (D, c["k"]), (2 * D, c["v"]))
    else:
        (q3,), (k3, v3) = place(dt, D + 8, (0, c["qu"])), place(dt, 2 * D + 8, (0, c["k"]), (D, c["v"]))
    (d3,) = place(dt, D + 16, (8, c["dctx"]))
    mdev = None if c["m8"] is None else c["m8"].to(DEV)
    name = f"{T1}x{T2} mask={mask}"
    runs = []
    for _ in range(2):
        cflat, (c3,), cout = guarded(dt, B * T1, D + 16, [8])        # an operand of the backward: 16-byte rows and offset
        lflat = torch.full((H * B * T1 + 2,), float("nan"), device=DEV)
        assert ops.attn_fwd_stream(q3, None, k3, v3, None, mdev, B, T1, T2, H, DK, scale=SCALE, out=c3, lse=lflat[1:-1]) is cflat
        if T1 == T2:
            gflat, (dq3, dk3, dv3), gout = guarded(dt, B * T1, 3 * D + 12, [4, 4 + D, 4 + 2 * D])
            bufs = [(gflat, gout)]
        else:
            (qf, (dq3,), qo), (kf, (dk3, dv3), ko) = guarded(dt, B * T1, D + 12, [4]), guarded(dt, B * T2, 2 * D + 12, [4, 4 + D])
            bufs = [(qf, qo), (kf, ko)]
        assert ops.attn_bwd_stream(d3, c3, q3, k3, v3, mdev, lflat[1:-1], dq3, dk3, dv3, B, T1, T2, H, DK, SCALE), "the library declined the operands"
        torch.cuda.synchronize()
        runs.append([lflat] + [b for b, _ in bufs])
        for buf, outside in bufs + [(cflat, cout)]:
            assert bool(torch.isnan(buf[outside]).all()), f"{name}: written outside an output's extent"
        assert bool(torch.isnan(lflat[[0, -1]]).all()), f"{name}: lse written outside its extent"
    for x, y in zip(*runs):
        bits = torch.int16 if x.dtype == BF16 else torch.int32
        assert torch.equal(x.view(bits), y.view(bits)), f"{name}: two launches differ"
    block = lambda v3_, T: v3_[0][1:-1, v3_[1] - v3_[2]:v3_[1] - v3_[2] + D].reshape(B * T, D)
    dq = block(dq3, T1)
    assert bool((dq.reshape(B * T1, H, DK)[c["dead"].to(DEV)] == 0).all()), f"{name}: dq of a fully masked row is not exactly zero"
    assert bool((lflat[1:-1].cpu()[c["dead"].view(B, T1, H).permute(2, 0, 1).reshape(-1)] == 0).all()), f"{name}: lse of a dead row"
    compare(name, "lse", dtype, lflat[1:-1], c["lse"], c["lse_bound"])
    compare(name, "dq", dtype, dq, *c["dq", dtype])
    compare(name, "dk", dtype, block(dk3, T2), *c["dk", dtype])
    compare(name, "dv", dtype, block(dv3, T2), *c["dv", dtype])


def test_argument_checks_launch_nothing():
    from espnet_amd import _lib
    L = _lib.lib()
    good = dict(dctx=0x10000, ldd=256, ctx=0x20000, ldc=256, qu=0x30000, ldq=256, k=0x40000, ldk=256, v=0x50000, ldv=256, mask=None,
                mb=0, mi=0, lse=0x60000, ws=0x70000, dq=0x80000, lddq=256, dk_out=0x90000, lddk=256, dv=0xa0000, lddv=256, B=2, H=4,
                T1=5000, T2=5000, dk=64, scale=0.125, stream=None)
    for fn in (L.eamd_attn_bwd_stream, L.eamd_attn_bwd_stream_f32):        # made-up addresses: no row may be a valid call
        for change, code in ((dict(dk=32), -2), (dict(lse=None), -1), (dict(dq=None), -1), (dict(dctx=None), -1), (dict(ldk=258), -2)):
            assert fn(*dict(good, **change).values()) == code, change
    fwd = dict(qu=0x10000, ldq=256, qv=None, ldqv=0, k=0x30000, ldk=256, v=0x40000, ldv=256, pos=None, ldpos=0, mask=None, mb=0, mi=0,
               ctx=0x70000, ldc=256, B=2, H=4, T1=5000, T2=5000, dk=64, scale=0.125, shift_len=None, lse=0x80000, stream=None)
    for fn in (L.eamd_attn_fwd_stream_lse, L.eamd_attn_fwd_stream_lse_f32):
        for change, code in ((dict(dk=32), -2), (dict(lse=None), -1), (dict(ctx=None), -1), (dict(ldk=258), -2)):
            assert fn(*dict(fwd, **change).values()) == code, change


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("bf16", 1e-2)])       # test_layers_agree_with_the_stored_path's bounds
def test_layers_agree_with_the_stored_path(prec, tol):
    """training-mode Transformer encoder layer and decoder layer (self-attention under subsequent_mask, source attention T1 = 9
    against T2 = 70 on a padded batch), dropout 0: output, input gradients and every parameter gradient, streamed (threshold 0)
    against the stored-P kernels (default threshold).  The key bias has NO gradient (a constant added to every key moves a
    row's scores together), so both paths return rounding noise there: it is measured against the value bias's gradient, the
    column sum over the same rows.  The feed-forward blocks use Swish: behind a ReLU the bf16 difference between two correct
    attention paths flips whole gates (a handful of the decoder's 18 x 512 moved its w_1 gradient by 3e-2), which says nothing
    about attention"""
    import espnet_amd
    from espnet_amd import functional as F_
    from espnet_amd.nets import modules as M
    torch.manual_seed(3)
    ff = lambda: M.PositionwiseFeedForward(256, 512, 0.0, M.Swish())  # noqa: E731
    enc = M.TransformerEncoderLayer(256, M.MultiHeadedAttention(4, 256, 0.0), ff(), 0.0).to(DEV).train()
    dec = M.DecoderLayer(256, M.MultiHeadedAttention(4, 256, 0.0), M.MultiHeadedAttention(4, 256, 0.0), ff(), 0.0).to(DEV).train()
    x, mem, tgt = (torch.randn(2, n, 256, device=DEV, requires_grad=True) for n in (70, 70, 9))
    gy, gz = torch.randn(2, 70, 256, device=DEV), torch.randn(2, 9, 256, device=DEV)
    xmask = M.make_non_pad_mask([70, 51]).unsqueeze(1)
    tmask = M.subsequent_mask(9).unsqueeze(0).expand(2, 9, 9).contiguous()
    params = [(f"{m}.{n}", p) for m, layer in (("enc", enc), ("dec", dec)) for n, p in layer.named_parameters()]
    espnet_amd.set_precision(prec)
    default, res = F_.ATTN_STREAM_TRAIN_KEYS, []
    try:
        for keys in (default, 0):
            F_.ATTN_STREAM_TRAIN_KEYS = keys
            for t in [x, mem, tgt] + [p for _, p in params]:
                t.grad = None
            y, _ = enc(x, xmask)
            z = dec(tgt, tmask, mem, xmask)[0]
            torch.autograd.backward([y, z], [gy, gz])
            res.append(dict([("y", y.detach()), ("z", z.detach()), ("dx", x.grad), ("dmem", mem.grad), ("dtgt", tgt.grad)]
                            + [(n, p.grad) for n, p in params]))
    finally:
        F_.ATTN_STREAM_TRAIN_KEYS = default
        espnet_amd.set_precision("fp32")
    for name, b in res[0].items():
        den = res[0][name.replace("linear_k.bias", "linear_v.bias")].double().norm()
        e = float((res[1][name].double() - b.double()).norm() / den)
        print(f"[attn_stream_train] {name} [{prec}] streamed vs stored: rel_l2 {e:.3e} (tol {tol:g})")
        assert e <= tol, (name, e)


def test_block_past_4096_keys_trains_in_linear_memory():
    """one mha_block without relative positions (B = 1, D = 256, H = 4, fp32) at T' = 4608, default threshold, forward + backward:
    the peak stays below ONE [H, T', T'] fp32 tensor (340 MB; the GEMM + softmax route allocates several)"""
    from espnet_amd.nets import modules as M
    torch.manual_seed(5)
    T = 4608
    norm, att = M.LayerNorm(256).to(DEV), M.MultiHeadedAttention(4, 256, 0.0).to(DEV).train()
    x = torch.randn(1, T, 256, device=DEV, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    M.mha_block(norm, att, x, None, None, None).square().sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"[attn_stream_train] mha_block T'={T} forward + backward: peak rise {rise / 2 ** 20:.1f} MB")
    grads = [x.grad] + [p.grad for p in list(norm.parameters()) + list(att.parameters())]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and rise < 4 * T * T * 4
