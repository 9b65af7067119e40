"""Attention dropout inside the memory-linear attention kernels (the *_drop entry points of csrc/attn_stream.hip, attn_stream_bwd.hip and
attn_stream_bwd_rel.hip; ops.attn_fwd_stream / attn_bwd_stream / attn_bwd_stream_rel with drop=(p, salt)) against float64 torch
autograd on the CPU under the keep mask tests/dropout_restatement.py draws for P's stored layout [H, B, T1, ldp], ldp = _ldp(T2).
Inputs, masks and ceilings are those of test_gpu_attn_stream_train.case / test_gpu_attn_stream_rel_train.case at p = 0: dropout only
rescales the surviving terms by 1 / (1 - p), so per element |got - ref| <= c * ceiling / (1 - p) with c NO LARGER than the constant
those files hold for the same quantity and storage - and at most 4x the error/ceiling observed on the MI355X, noted beside each.
T1 = 70 x T2 = 100: a ragged last query block and key tile and ldp = 104 > T2; the masks are case()'s key padding (second utterance
shorter) and its fully masked query row, one case each: the ceilings are per mask."""
import pytest
import torch

import attention_restatement as ar
import test_gpu_attn_stream_rel_train as rt
import test_gpu_attn_stream_train as st
from test_gpu_attn_stream import BF16, DEV, DK, F32, KT, TINY, U23, place
from test_gpu_attn_stream_train import B, D, H, SCALE, compare, guarded

gpu = pytest.mark.gpu
T1, T2, T, TS, SALT, LDP = 70, 100, 100, 70, 11, 104
DT = {"f32": F32, "bf16": BF16}
# c of (quantity, storage), in units of ceiling / (1 - p): at most 4x the worst error/ceiling observed on the MI355X over the cases
# below (beside it), each below the p = 0 constant of the files above (ctx: test_gpu_attn_stream.TOL_STREAM_*)
TOL = {("ctx", "f32"): 0.0096, ("ctx", "bf16"): 0.0028,         # observed 2.401e-3, 7.143e-4   (p = 0 constants 0.0147, 0.0052)
       ("lse", "f32"): 0.0114, ("lse", "bf16"): 0.0114,         # observed 2.872e-3, 2.872e-3   (0.013, 0.013)
       ("dq", "f32"): 0.00046, ("dq", "bf16"): 0.63,            # observed 1.168e-4, 1.578e-1   (0.0008, 0.7)
       ("dk", "f32"): 0.0015, ("dk", "bf16"): 0.56,             # observed 3.814e-4, 1.422e-1   (0.0023, 0.67)
       ("dv", "f32"): 0.0147, ("dv", "bf16"): 0.0042,           # observed 3.697e-3, 1.064e-3   (0.021, 0.010)
       ("dqu", "f32"): 0.00053, ("dqu", "bf16"): 0.00042,       # observed 1.335e-4, 1.066e-4   (0.0009, 0.00079)
       ("dqv", "f32"): 0.00085, ("dqv", "bf16"): 0.00071,       # observed 2.134e-4, 1.792e-4   (0.0014, 0.0013)
       ("rel_dk", "f32"): 0.00067, ("rel_dk", "bf16"): 0.00014,  # observed 1.691e-4, 3.565e-5   (0.0018, 0.0007)
       ("rel_dv", "f32"): 0.0091, ("rel_dv", "bf16"): 0.0021,   # observed 2.282e-3, 5.274e-4   (0.018, 0.013)
       ("dpos", "f32"): 0.00079, ("dpos", "bf16"): 0.00067}     # observed 1.995e-4, 1.682e-4   (0.042, 0.042)


def reference(c, p, step, Tq, Tk, ts=None):
    """float64 autograd of ctx = (softmax(mask(scale (qu k^T + rel_shift(qv pos^T)))) o keep / (1 - p)) v -> ctx, its p = 0 ceiling
    (test_gpu_attn_stream.case's formula), lse and the gradients"""
    x = {n: c[n].double().view(*((Tk,) if n == "pos" else (B, -1)), H, DK).requires_grad_() for n in ("qu", "qv", "k", "v", "pos") if n in c}
    s = torch.einsum("bihd,bjhd->hbij", x["qu"], x["k"])
    if "pos" in x:
        s = s + ar.rel_shift(torch.einsum("bihd,jhd->hbij", x["qv"], x["pos"]), ts)
    live = ar.live_of(c["m8"], B, Tq, Tk).expand(H, B, Tq, Tk)
    dead = ~live.any(-1, keepdim=True)
    s = torch.where(live, s * SCALE, torch.full((), float("-inf")).double()).masked_fill(dead, 0.0)
    P = torch.softmax(s, -1) * ~dead
    ctx = torch.einsum("hbij,bjhd->bihd", P * ar.keep_tensor(step, SALT, p, H, B, Tq, Tk, LDP) * ar.drop_inv(p), x["v"])
    ctx.backward(c["dctx"].double().view(B, Tq, H, DK))
    with torch.no_grad():
        f = ar.forward(x["qu"], x["k"], SCALE, x.get("qv"), x.get("pos"), c["m8"], ts)
        bound = ar.context(f["P_bound"], x["v"].abs())[0] + (live.sum(-1).permute(1, 2, 0).unsqueeze(-1) + -(-Tk // KT) + 8) * U23 * ar.context(f["P"], x["v"])[1]
    lse = torch.logsumexp(s.detach(), -1).masked_fill(dead[..., 0], 0.0)
    return dict({n: t.grad.reshape(-1, D) for n, t in x.items()}, ctx=ctx.detach().reshape(-1, D), ctx_bound=bound.reshape(-1, D) + TINY, lse=lse.reshape(-1))


def check(name, what, dtype, p, got, ref, ceiling):
    st.TOL["drop", dtype] = TOL[what, dtype]
    compare(f"{name} {what}", "drop", dtype, got, ref, ceiling / (1.0 - p))


def launch(c, dt, drop, rel, ts=None):
    """forward + backward through ops with drop -> the output blocks and lse"""
    from espnet_amd import ops
    Tq, Tk = (T, T) if rel else (T1, T2)
    (q3,), (k3, v3), (d3,) = place(dt, D + 8, (0, c["qu"])), place(dt, 2 * D + 8, (0, c["k"]), (D, c["v"])), place(dt, D + 16, (8, c["dctx"]))
    w3, p3 = (place(dt, D + 8, (0, c["qv"]))[0], place(dt, D + 16, (8, c["pos"]))[0]) if rel else (None, None)
    mdev = None if c["m8"] is None else c["m8"].to(DEV)
    tsd = None if ts is None else torch.tensor([ts], dtype=torch.int32, device=DEV)
    cflat, (c3,), cout = guarded(dt, B * Tq, D + 16, [8])
    lse = torch.full((H * B * Tq,), float("nan"), device=DEV)
    assert ops.attn_fwd_stream(q3, w3, k3, v3, p3, mdev, B, Tq, Tk, H, DK, scale=SCALE, shift_len=tsd, out=c3, lse=lse, drop=drop) is cflat
    (qf, (dq3, dw3), qo), (kf, (dk3, dv3), ko) = guarded(F32 if rel else dt, B * Tq, 2 * D + 12, [4, 4 + D]), guarded(dt, B * Tk, 2 * D + 12, [4, 4 + D])
    if rel:
        pf, (dp3,), po = guarded(F32, T, D + 12, [4])
        pf[1:-1, 4:4 + D] = c["dpos0"].to(DEV)
        assert ops.attn_bwd_stream_rel(d3, c3, q3, w3, k3, v3, p3, mdev, lse, dq3, dw3, dk3, dv3, dp3, B, T, T, H, DK, SCALE, shift_len=tsd,
                                       drop=drop)
    else:
        pf, dp3, po = qf, dw3, qo
        qf[1:-1, 4 + D:4 + 2 * D] = 0                          # the unused second block
        assert ops.attn_bwd_stream(d3, c3, q3, k3, v3, mdev, lse, dq3, dk3, dv3, B, Tq, Tk, H, DK, SCALE, drop=drop)
    torch.cuda.synchronize()
    for buf, outside in ((cflat, cout), (qf, qo), (kf, ko), (pf, po)):
        assert bool(torch.isnan(buf[outside]).all()), "written outside an output's extent"
    block = lambda v_: v_[0][1:-1, v_[1] - v_[2]:v_[1] - v_[2] + D]
    return dict(ctx=block(c3), lse=lse, dk=block(dk3), dv=block(dv3), dq=block(dq3), dqv=block(dw3), dpos=block(dp3))


def step_now():
    from espnet_amd import ops
    return int(ops.rng_state(torch.zeros(1, device=DEV).device))


@gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mask", ["len", "dead_row"])
def test_cross_shape_against_float64(mask, dtype, p):
    c, name = st.case(T1, T2, mask), f"{T1}x{T2} {mask} p={p}"
    ref, got = reference(c, p, step_now(), T1, T2), launch(c, DT[dtype], (p, SALT), False)
    assert torch.equal(got["lse"], launch(c, DT[dtype], None, False)["lse"]), f"{name}: lse is not the p = 0 value"
    dead = c["dead"].to(DEV)
    assert all(bool((got[n].reshape(B * T1, H, DK)[dead] == 0).all()) for n in ("ctx", "dq")), f"{name}: a fully masked row is not exactly zero"
    check(name, "ctx", dtype, p, got["ctx"], ref["ctx"], ref["ctx_bound"])
    check(name, "lse", dtype, 0.0, got["lse"], c["lse"], c["lse_bound"])
    for what, r in (("dq", "qu"), ("dk", "k"), ("dv", "v")):
        check(name, what, dtype, p, got[what], ref[r], c[what, dtype][1])


@gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rel_pos_against_float64(dtype, p):
    c, name = rt.case(T, "len", TS), f"rel T={T} ts={TS} p={p}"
    ref, got = reference(c, p, step_now(), T, T, TS), launch(c, DT[dtype], (p, SALT), True, TS)
    ref["pos"] = ref["pos"] + c["dpos0"].double()              # dpos is added into a pre-filled buffer
    check(name, "ctx", dtype, p, got["ctx"], ref["ctx"], ref["ctx_bound"])
    for what, g, r in (("dqu", "dq", "qu"), ("dqv", "dqv", "qv"), ("rel_dk", "dk", "k"), ("rel_dv", "dv", "v"), ("dpos", "dpos", "pos")):
        check(name, what, dtype, p, got[g], ref[r], c[what, dtype][1])


@gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_drop_p_zero_has_the_bits_of_the_plain_entry_points(dtype):
    for c, rel, ts in ((st.case(T1, T2, "len"), False, None), (rt.case(T, "len", TS), True, TS)):
        a, b = launch(c, DT[dtype], (0.0, SALT), rel, ts), launch(c, DT[dtype], None, rel, ts)
        for n in a:
            v = torch.int16 if a[n].dtype == BF16 else torch.int32
            assert torch.equal(a[n].contiguous().view(v), b[n].contiguous().view(v)), (rel, n)


@gpu
@pytest.mark.parametrize("prec,tol", [("fp32", 1.7e-6), ("bf16", 1e-2)])     # observed 4.346e-7, 3.294e-3 (p = 0 files: 2e-5, 1e-2)
def test_route_is_streamed_and_agrees_with_the_stored_route(prec, tol):
    """attention dropout 0.1, thresholds 0: attn_block_fwd streams with and without positions, and a MultiHeadedAttention and a
    rel-pos block (padded batch [70, 51]), forward + backward at one (step, salt), agree with the stored route - the same mask"""
    import espnet_amd
    from espnet_amd import functional as F_
    from espnet_amd.nets import modules as M
    torch.manual_seed(3)
    norm = M.LayerNorm(256).to(DEV)
    blocks = [(M.MultiHeadedAttention(4, 256, 0.1).to(DEV).train(), None),
              (M.RelPositionMultiHeadedAttention(4, 256, 0.1).to(DEV).train(), torch.randn(1, 70, 256, device=DEV))]
    x, gy = torch.randn(2, 70, 256, device=DEV, requires_grad=True), torch.randn(2, 70, 256, device=DEV)
    xmask = M.make_non_pad_mask([70, 51]).unsqueeze(1).to(DEV)
    names = ("ATTN_STREAM_KEYS", "ATTN_STREAM_TRAIN_KEYS", "ATTN_STREAM_TRAIN_REL_KEYS", "ATTN_STREAM_DROP_KEYS")
    default, res = [getattr(F_, n) for n in names], []
    espnet_amd.set_precision(prec)
    try:
        for keys in (default, [0, 0, 0, 0]):
            for n, k in zip(names, keys):
                setattr(F_, n, k)
            out = {}
            for att, pos in blocks:
                for t in [x] + list(att.parameters()):
                    t.grad = None
                y = M.mha_block(norm, att, x, None, pos, xmask)
                y.backward(gy)
                tag = "rel." if pos is not None else "abs."
                out.update({tag + "y": y.detach(), tag + "dx": x.grad.clone()}, **{tag + n: q.grad.clone() for n, q in att.named_parameters()})
            res.append(out)
        q = torch.randn(2 * 70, 256, device=DEV).to(F_.ops.act_dtype())
        for qv, pp in ((None, None), (q, q[:70])):
            for grad in (False, True):
                kept = F_.attn_block_fwd(q, qv, q, q, pp, None, 2, 70, 70, 4, 64, (0.1, SALT), None, grad, False, True)[1]
                assert kept.route == "stream" and (kept.lse is not None) == grad
        F_.ATTN_STREAM_DROP_KEYS = default[3]                  # its own threshold: dropout alone keeps the stored route up to it
        assert F_.attn_block_fwd(q, None, q, q, None, None, 2, 70, 70, 4, 64, (0.1, SALT), None, True, False, True)[1].route != "stream"
    finally:
        for n, k in zip(names, default):
            setattr(F_, n, k)
        espnet_amd.set_precision("fp32")
    for name, b in res[0].items():
        den = res[0][name.replace("linear_k.bias", "linear_v.bias")].double().norm()
        e = float((res[1][name].double() - b.double()).norm() / den)
        print(f"[attn_stream_dropout] {name} [{prec}] streamed vs stored: rel_l2 {e:.3e} (tol {tol:g})")
        assert e <= tol, (name, e)


def test_drop_arguments_are_refused_before_any_launch():
    from espnet_amd import _lib
    L = _lib.lib()
    dims, drop = dict(B=2, H=4, T1=5000, T2=5000, dk=64, scale=0.125), dict(drop_p=0.1, drop_step=0x200000, drop_salt=3, stream=None)
    fwd = dict(qu=0x10000, ldq=256, qv=None, ldqv=0, k=0x30000, ldk=256, v=0x40000, ldv=256, pos=None, ldpos=0, mask=None, mb=0, mi=0,
               ctx=0x70000, ldc=256, **dims, shift_len=None, lse=0x80000, **drop)
    bwd = dict(dctx=0x10000, ldd=256, ctx=0x20000, ldc=256, qu=0x30000, ldq=256, k=0x40000, ldk=256, v=0x50000, ldv=256, mask=None, mb=0,
               mi=0, lse=0x60000, ws=0x70000, dq=0x80000, lddq=256, dk_out=0x90000, lddk=256, dv=0xa0000, lddv=256, **dims, **drop)
    rel = dict(dctx=0x10000, ldd=256, ctx=0x20000, ldc=256, qu=0x30000, ldq=256, qv=0x40000, ldqv=256, k=0x50000, ldk=256, v=0x60000,
               ldv=256, pos=0x70000, ldpos=256, mask=None, mb=0, mi=0, lse=0x80000, shift_len=None, delta_ws=0x90000, dqv_ws=0xa0000,
               dpos_ws=0xb0000, dqu=0xc0000, lddqu=256, dqv=0xd0000, lddqv=256, dk_out=0xe0000, lddk=256, dv=0xf0000, lddv=256,
               dpos=0x100000, lddpos=256, **dims, **drop)
    rows = ((dict(drop_p=1.0), -1), (dict(drop_p=-0.1), -1), (dict(drop_step=None), -1), (dict(dk=32), -2), (dict(ldk=258), -2), (dict(k=None), -1))
    for good, stem in ((fwd, "eamd_attn_fwd_stream_drop"), (bwd, "eamd_attn_bwd_stream_drop"), (rel, "eamd_attn_bwd_stream_rel_drop")):
        for fn in (getattr(L, stem), getattr(L, stem + "_f32")):           # made-up addresses: no row may be a valid call
            for change, code in rows:
                assert fn(*dict(good, **change).values()) == code, (stem, change)
