"""Memory-linear attention training WITH relative positions (csrc/attn_stream_bwd_rel.hip; ops.attn_bwd_stream_rel) element by
element against the float64 restatement tests/attention_restatement.py, and the Conformer blocks that reach it with autograd.
Inputs, masks and guarded buffers are those of test_gpu_attn_stream.py / test_gpu_attn_stream_train.py; the backward is fed the
ctx and lse its own forward wrote.  The ceilings are test_gpu_attn_stream_train.case()'s, with the position term's magnitudes in
the score ceiling (ar.forward does that) and dS carried through the inverse shift into dqv = dbd pos and dpos = sum_b dbd^T qv."""
import functools

import pytest
import torch

import attention_restatement as ar
import test_gpu_attn_stream_train as st
from test_gpu_attn_stream import BF16, DEV, DK, F32, KT, TINY, U23, make_mask, place
from test_gpu_attn_stream_train import B, D, H, SCALE, compare, guarded

pytestmark = pytest.mark.gpu

# c per output and storage type: at most 4x the worst error/ceiling observed on the MI355X over the 58 cases (observed beside it)
# (bf16 storage takes delta from its own fp32 sweep, not from the rounded ctx: the 2^-9 |ctx| the bf16 ceilings allow is not used)
st.TOL.update({("dqu", "f32"): 0.0009, ("dqu", "bf16"): 0.00079,        # rel_bwd_q_kernel                   observed 2.358e-4, 1.991e-4
               ("dqv", "f32"): 0.0014, ("dqv", "bf16"): 0.0013,         #  + rel_bwd_dqv_shift_kernel        observed 3.583e-4, 3.440e-4
               ("rel_dk", "f32"): 0.0018, ("rel_dk", "bf16"): 0.0007,   # rel_bwd_kv_kernel                  observed 4.518e-4, 1.750e-4
               ("rel_dv", "f32"): 0.018, ("rel_dv", "bf16"): 0.013,     #                                    observed 4.706e-3, 3.492e-3
               ("dpos", "f32"): 0.042, ("dpos", "bf16"): 0.042})        # rel_bwd_dpos_kernel + _sum_kernel  observed 1.057e-2, 1.057e-2
MASKS = [None, "len", "dead_row", "causal"]
CASES = [(T, m, None) for T in (1, 2, 17, 63, 65, 101, 130) for m in MASKS] + [(101, "len", 70)]


@functools.lru_cache(maxsize=None)
def case(T, mask, ts):
    """inputs (bf16-exact fp32 values) and the float64 references with their ceilings per storage type, once per case"""
    g = torch.Generator().manual_seed(T * 138 + B)
    rnd = lambda rows: (0.5 * torch.randn(rows, D, generator=g)).to(BF16).float()
    w = torch.where(torch.rand(D, generator=g) < 0.5, -0.5, 0.5)
    sgn = torch.where(torch.arange(B * T) % T % 2 == 1, 1.0, -1.0)[:, None]
    qu, k, v, dctx = (32.0 * rnd(B * T) + 16.0 * sgn * w).to(BF16).float(), rnd(B * T), rnd(B * T), rnd(B * T)
    k.view(B, T, D)[:, 0], k.view(B, T, D)[:, T - 1] = w, -w
    qv, pos, dpos0 = (32.0 * rnd(B * T)).to(BF16).float(), rnd(T), rnd(T)
    Ts = T if ts is None else ts
    m8 = make_mask(mask, B, T, T, Ts)
    q64, w64, k64, v64, d64 = (t.double().view(B, T, H, DK) for t in (qu, qv, k, v, dctx))
    p64 = pos.double().view(T, H, DK)
    f = ar.forward(q64, k64, SCALE, w64, p64, m8, Ts)
    P, Pb = f["P"], f["P_bound"]
    c = dict(qu=qu, qv=qv, k=k, v=v, pos=pos, dctx=dctx, dpos0=dpos0, m8=m8, dead=(~f["live"].any(-1)).permute(1, 2, 0).reshape(B * T, H))
    cx, cmag = ar.context(P, v64)
    nlive = f["live"].sum(-1).permute(1, 2, 0).unsqueeze(-1)
    cbound = ar.context(Pb, v64.abs())[0] + (nlive + -(-T // KT) + 8) * U23 * cmag       # the forward's ceiling on ctx
    bq = ar.backward_q(d64, v64, P, SCALE, Ts=Ts, rel=True)
    A = ar.contract("bihd,bjhd->hbij", d64, v64)[1]
    ks = ar.key_side(P, bq["dS"], d64, q64, dbd=bq["dbd"], qv=w64)
    dqv, dqvm = ar.contract("hbij,jhd->bihd", bq["dbd"], p64)
    flat = lambda t: t.reshape(-1, D)
    dv = (flat(ks["dv"]), flat(ar.key_side(Pb, bq["dS"], d64.abs(), q64)["dv"] + (T + 8) * U23 * ks["dv_mag"]) + TINY)
    for dt, half_ulp in (("f32", 0.0), ("bf16", 2.0 ** -9)):
        derr = (d64.abs() * (cbound + ((DK + 8) * U23 + half_ulp) * cx.abs())).sum(-1).permute(2, 0, 1).unsqueeze(-1)   # [H, B, T, 1]
        dSb = (DK + T + 16) * U23 * bq["dS_mag"] + SCALE * (Pb * (A + (P * A).sum(-1, keepdim=True))
                                                             + P * ((Pb * A).sum(-1, keepdim=True) + derr))
        dbdb = ar.rel_unshift(dSb, Ts)                                                   # the ceiling travels with its element
        dq, dqm = ar.dq_of(bq["dS"], k64)
        c["dqu", dt] = (flat(dq), flat(ar.dq_of(dSb, k64.abs())[0] + (T + 8) * U23 * dqm) + TINY)
        c["dqv", dt] = (flat(dqv), flat(torch.einsum("hbij,jhd->bihd", dbdb, p64.abs()) + (T + 8) * U23 * dqvm) + TINY)
        c["rel_dk", dt] = (flat(ks["dk"]), flat(ar.key_side(P, dSb, d64, q64.abs())["dk"] + (T + 8) * U23 * ks["dk_mag"]) + TINY)
        c["rel_dv", dt] = dv
        # the batch sum is added into a non-zero destination: one more rounding of the result
        c["dpos", dt] = (flat(ks["dpos"]) + dpos0.double(), flat(torch.einsum("hbij,bihd->jhd", dbdb, w64.abs())
                                                                 + (B * T + 8) * U23 * (ks["dpos_mag"] + dpos0.double().abs().view(T, H, DK))) + TINY)
    return c


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("T,mask,ts", CASES, ids=str)
def test_kernels_against_float64(dtype, T, mask, ts):
    """dqv of a dead row is NOT zero in general - qv_i also enters row i - 1's scores through the upper part of the shift - so
    it is asserted exactly zero where the restatement's is (T = 1, and T = 2 where the upper part is empty)"""
    from espnet_amd import ops
    c = case(T, mask, ts)
    dt = {"f32": F32, "bf16": BF16}[dtype]
    q3, k3, v3 = place(dt, 3 * D + 8, (0, c["qu"]), (D, c["k"]), (2 * D, c["v"]))
    (w3,), (p3,), (d3,) = place(dt, D + 8, (0, c["qv"])), place(dt, D + 16, (8, c["pos"])), place(dt, D + 16, (8, c["dctx"]))
    mdev = None if c["m8"] is None else c["m8"].to(DEV)
    tsd = None if ts is None else torch.tensor([ts], dtype=torch.int32, device=DEV)
    name = f"T={T} mask={mask} ts={ts}"
    runs = []
    for _ in range(2):
        cflat, (c3,), cout = guarded(dt, B * T, D + 16, [8])
        lse = torch.empty(H * B * T, device=DEV)
        assert ops.attn_fwd_stream(q3, w3, k3, v3, p3, mdev, B, T, T, H, DK, scale=SCALE, shift_len=tsd, out=c3, lse=lse) is cflat
        qflat, (dqu3, dqv3), qout = guarded(F32, B * T, 2 * D + 12, [4, 4 + D])
        kflat, (dk3, dv3), kout = guarded(dt, B * T, 2 * D + 12, [4, 4 + D])
        pflat, (dp3,), pout = guarded(F32, T, D + 12, [4])
        pflat[1:-1, 4:4 + D] = c["dpos0"].to(DEV)
        assert ops.attn_bwd_stream_rel(d3, c3, q3, w3, k3, v3, p3, mdev, lse, dqu3, dqv3, dk3, dv3, dp3, B, T, T, H, DK, SCALE,
                                       shift_len=tsd), "the library declined the operands"
        torch.cuda.synchronize()
        for buf, outside in ((qflat, qout), (kflat, kout), (pflat, pout), (cflat, cout)):
            assert bool(torch.isnan(buf[outside]).all()), f"{name}: written outside an output's extent"
        runs.append([qflat, kflat, pflat])
    for x, y in zip(*runs):
        bits = torch.int16 if x.dtype == BF16 else torch.int32
        assert torch.equal(x.view(bits), y.view(bits)), f"{name}: two launches differ"
    block = lambda v3_: v3_[0][1:-1, v3_[1] - v3_[2]:v3_[1] - v3_[2] + D]
    dead = c["dead"].to(DEV)
    assert bool((block(dqu3).reshape(B * T, H, DK)[dead] == 0).all()), f"{name}: dqu of a fully masked row is not exactly zero"
    zero = dead[:, :, None] & (c["dqv", dtype][0].view(B * T, H, DK) == 0).to(DEV)
    assert bool((block(dqv3).reshape(B * T, H, DK)[zero] == 0).all()), f"{name}: dqv of a fully masked row is not exactly zero"
    for what, view in (("dqu", dqu3), ("dqv", dqv3), ("rel_dk", dk3), ("rel_dv", dv3), ("dpos", dp3)):
        compare(name, what, dtype, block(view), *c[what, dtype])


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("bf16", 1e-2)])       # test_layers_agree_with_the_stored_path's bounds
def test_conformer_encoder_agrees_with_the_stored_path(prec, tol):
    """training-mode 2-layer Conformer encoder (rel-pos, macaron Swish feed-forwards, dropout 0) on arena parameters, so linear_pos
    runs as the shared projection and dpos is added into its gradient block; T' = 70 on a padded batch [70, 51]: output and every
    parameter gradient (the front end returns no gradient for the features; its own parameters' gradients carry the gradient at
    the layers' input through the whole subsampling stack), streamed (threshold 0) against the stored-P kernels (default
    threshold).  linear_k.bias has no gradient (test_gpu_attn_stream_train): it is measured against linear_v.bias's norm.
    The layers carry no convolution module: behind its training-mode BatchNorm every channel's gradient sums to zero over the
    rows, so the bias gradients in front of it (depthwise_conv.bias: exactly zero; pointwise_conv1.bias, norm_conv.bias: what the
    GLU leaves of the cancellation) are rounding noise in bf16 on EITHER route - measured with the module in, norm_conv.bias of the
    bf16 stored route is 1.011e-2 from its fp32 value, the streamed one 1.081e-2, the two 1.057e-2 apart - which says nothing
    about attention, as the ReLU gates of test_gpu_attn_stream_train's docstring do not."""
    import espnet_amd
    from espnet_amd import functional as F_, ops, train
    from espnet_amd.nets import modules as M
    torch.manual_seed(3)
    enc = M.ConformerEncoder(20, 256, 4, 512, 2, 0.0, 0.0, 0.0, macaron_style=True, pos_enc_layer_type="rel_pos",
                             selfattention_layer_type="rel_selfattn").to(DEV).train()
    flat = train.FlatParams(enc)
    x = torch.randn(2, 283, 20, device=DEV, requires_grad=True)              # 283 frames -> T' = 70, 207 -> 51
    xmask = M.make_non_pad_mask([283, 207]).unsqueeze(1)
    gy = torch.randn(2, 70, 256, device=DEV)
    espnet_amd.set_precision(prec)
    default, res, rec = F_.ATTN_STREAM_TRAIN_REL_KEYS, [], []
    try:
        for keys in (default, 0):
            F_.ATTN_STREAM_TRAIN_REL_KEYS = keys
            flat.zero_grad()
            ops._gemm_record = rec if keys == 0 else None
            y, _ = enc(x, xmask)
            y.backward(gy)
            ops._gemm_record = None
            assert x.grad is None       # the conv2d front end treats the features as data: embed.*'s gradients stand for dx
            res.append(dict([("y", y.detach())] + [(n, p._eamd_grad.clone()) for n, p in enc.named_parameters()]))
    finally:
        ops._gemm_record = None
        F_.ATTN_STREAM_TRAIN_REL_KEYS = default
        espnet_amd.set_precision("fp32")
    kinds = [r[0]["kind"] for r in rec if isinstance(r[0], dict)]
    assert any(n.startswith("eamd_attn_fwd_stream_lse") for n in kinds) and any(n.startswith("eamd_attn_bwd_stream_rel") for n in kinds)
    assert not any(n.startswith("eamd_attn_bwd_q") for n in kinds), kinds
    for name, b in res[0].items():
        den = res[0][name.replace("linear_k.bias", "linear_v.bias")].double().norm()
        e = float((res[1][name].double() - b.double()).norm() / den)
        print(f"[attn_stream_rel_train] {name} [{prec}] streamed vs stored: rel_l2 {e:.3e} (tol {tol:g})")
        assert e <= tol, (name, e)


def test_rel_pos_block_past_4096_keys_trains_in_linear_memory():
    """one rel-pos mha_block (B = 1, D = 256, H = 4, fp32) at T' = 4608, default thresholds, forward + backward: the peak stays
    below ONE [H, T', T'] fp32 tensor (340 MB; the GEMM + softmax route allocates several)"""
    from espnet_amd.nets import modules as M
    torch.manual_seed(5)
    T = 4608
    norm, att = M.LayerNorm(256).to(DEV), M.RelPositionMultiHeadedAttention(4, 256, 0.0).to(DEV).train()
    x, pos = torch.randn(1, T, 256, device=DEV, requires_grad=True), torch.randn(1, T, 256, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    M.mha_block(norm, att, x, None, pos, None).square().sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"[attn_stream_rel_train] rel-pos mha_block T'={T} forward + backward: peak rise {rise / 2 ** 20:.1f} MB")
    grads = [x.grad] + [p.grad for p in list(norm.parameters()) + list(att.parameters())]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and rise < 4 * T * T * 4


def test_argument_checks_launch_nothing():
    from espnet_amd import _lib
    L = _lib.lib()
    good = dict(dctx=0x10000, ldd=256, ctx=0x20000, ldc=256, qu=0x30000, ldq=256, qv=0x40000, ldqv=256, k=0x50000, ldk=256, v=0x60000,
                ldv=256, pos=0x70000, ldpos=256, mask=None, mb=0, mi=0, lse=0x80000, shift_len=None, delta_ws=0x90000, dqv_ws=0xa0000,
                dpos_ws=0xb0000, dqu=0xc0000, lddqu=256, dqv=0xd0000, lddqv=256, dk_out=0xe0000, lddk=256, dv=0xf0000, lddv=256,
                dpos=0x100000, lddpos=256, B=2, H=4, T1=5000, T2=5000, dk=64, scale=0.125, stream=None)
    for fn in (L.eamd_attn_bwd_stream_rel, L.eamd_attn_bwd_stream_rel_f32):        # made-up addresses: no row may be a valid call
        for change, code in ((dict(dqv=None), -1), (dict(pos=None), -1), (dict(lse=None), -1), (dict(dk=32), -2), (dict(T1=90), -2),
                             (dict(ldqv=258), -2)):
            assert fn(*dict(good, **change).values()) == code, change
