"""tests/attention_restatement.py against torch.autograd in float64 built from the reference's formulas (the oracle's rel_shift,
the mask -> finfo.min -> softmax -> zero-fill sequence of forward_attention), its shift map against its inverse, and route()
at every boundary of the dispatch classes.  No GPU."""
import math

import pytest
import torch

import attention_restatement as ar


def _autograd_case(oracle, B, H, T1, T2, rel, Ts, mask, keep, inv, seed):
    """the reference's attention core in float64 with autograd; with Ts < T the positional term is the oracle's rel_shift of the
    Ts x Ts problem, zero elsewhere (rows >= Ts carry no positional term)"""
    dk = 8
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    leaf = lambda t: t.clone().requires_grad_(True)
    qu, k, v, dctx = rn(B, T1, H, dk), rn(B, T2, H, dk), rn(B, T2, H, dk), rn(B, T1, H, dk)
    qv, pos = (rn(B, T1, H, dk), rn(T2, H, dk)) if rel else (None, None)
    scale = 1.0 / math.sqrt(dk)
    Q, K, V = leaf(qu), leaf(k), leaf(v)
    sc = torch.einsum("bihd,bjhd->bhij", Q, K)
    bd = None
    if rel:
        QV, Pm = leaf(qv), leaf(pos)
        bd = torch.einsum("bihd,jhd->bhij", QV, Pm)
        bd.retain_grad()
        sh = torch.zeros_like(sc)
        sh[:, :, :Ts, :Ts] = oracle.rel_shift(bd[:, :, :Ts, :Ts])
        sc = sc + sh
    sc = sc * scale
    if mask is not None:
        m = (mask != 0).expand(B, -1, T2).unsqueeze(1).eq(0)
        attn = torch.softmax(sc.masked_fill(m, torch.finfo(torch.float32).min), dim=-1).masked_fill(m, 0.0)
    else:
        attn = torch.softmax(sc, dim=-1)
    attn.retain_grad()
    pd = attn if keep is None else attn * keep.permute(1, 0, 2, 3) * inv
    ctx = torch.einsum("bhij,bjhd->bihd", pd, V)
    ctx.backward(dctx)

    # the restatement, stage by stage, each stage from the previous stage's values
    f = ar.forward(qu, k, scale, qv, pos, mask, Ts, dk_ceiling=dk)
    close = lambda a, b, what: torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-12, msg=lambda m_: f"{what}: {m_}")
    hb = lambda t: t.detach().permute(1, 0, 2, 3)
    close(f["P"], hb(attn), "P")
    Pd = f["P"] if keep is None else f["P"] * keep * inv
    close(ar.context(Pd, v)[0], ctx.detach(), "ctx")
    bq = ar.backward_q(dctx, v, f["P"], scale, keep, inv, Ts, rel)
    close(ar.dq_of(bq["dS"], k)[0], Q.grad, "dq")
    ks = ar.key_side(Pd, bq["dS"], dctx, qu, bq["dbd"], qv)
    close(ks["dv"], V.grad, "dv")
    close(ks["dk"], K.grad, "dk")
    assert bool((f["P_bound"] >= 0).all()) and bool((bq["dS_mag"] >= bq["dS"].abs() * (1 - 1e-12)).all())
    if rel:
        close(bq["dbd"], hb(bd.grad), "dbd")
        close(ar.dq_of(bq["dbd"], pos.unsqueeze(0).expand(B, -1, -1, -1))[0], QV.grad, "dqv")
        close(ks["dpos"], Pm.grad, "dpos")
        assert bool((bq["dbd"][..., Ts:, :] == 0).all()) and bool((bq["dbd"][..., Ts:] == 0).all())
        assert bool((bq["dbd"][..., 0, :Ts - 1] == 0).all())


@pytest.mark.parametrize("B,H,T1,T2,rel,Ts,mk,p", [
    (2, 2, 5, 5, True, 5, None, 0.0), (2, 1, 7, 7, True, 4, "len", 0.0), (1, 3, 6, 6, True, 1, "len", 0.5),
    (3, 2, 4, 9, False, None, "dead", 0.0), (2, 2, 1, 3, False, None, "holes", 0.1), (1, 1, 1, 1, True, 1, None, 0.0),
    (2, 2, 9, 9, True, 8, "len", 0.1), (2, 1, 6, 6, False, None, "causal", 0.0)])
def test_restatement_matches_autograd(oracle, B, H, T1, T2, rel, Ts, mk, p):
    mask = None
    if mk == "len":             # keys >= Ts are masked: the kernels' precondition for a shorter shift
        lens = torch.tensor([(Ts or T2) - (b % 2) * ((Ts or T2) // 2) for b in range(B)])
        mask = (torch.arange(T2)[None, :] < lens[:, None]).to(torch.uint8).view(B, 1, T2)
    elif mk == "dead":
        mask = torch.ones(B, 1, T2, dtype=torch.uint8)
        mask[1] = 0
    elif mk == "holes":
        mask = torch.tensor([[[2, 0, 255]]], dtype=torch.uint8)
    elif mk == "causal":
        mask = torch.tril(torch.ones(T1, T2)).to(torch.uint8).view(1, T1, T2)
    keep, inv = None, 1.0
    if p > 0:
        ldp = (T2 + 7) // 8 * 8
        keep, inv = ar.keep_tensor(7, 3, p, H, B, T1, T2, ldp), ar.drop_inv(p)
        assert 0 < int(keep.sum()) < keep.numel()
    _autograd_case(oracle, B, H, T1, T2, rel, Ts, mask, keep, inv, seed=T1 * 31 + T2)


@pytest.mark.parametrize("Ts", [1, 2, 5, 17])
def test_shift_map_and_inverse(oracle, Ts):
    """shift_dst and shift_src are inverse to each other on the Ts x Ts square, the only places no bd element reaches are the
    zero column (i, i + 1), the only bd elements that reach nothing are the head of row 0, and the map is the oracle's rel_shift"""
    reached = {}
    for i in range(Ts):
        for m in range(Ts):
            d = ar.shift_dst(i, m, Ts)
            if d is None:
                assert i == 0 and m < Ts - 1
                continue
            assert 0 <= d[0] < Ts and 0 <= d[1] < Ts and d not in reached
            reached[d] = (i, m)
            assert ar.shift_src(d[0], d[1], Ts) == (i, m + 1)
    for i in range(Ts):
        for j in range(Ts):
            R, c = ar.shift_src(i, j, Ts)
            if c == 0:
                assert j == i + 1 and (i, j) not in reached
            else:
                assert reached[(i, j)] == (R, c - 1)
    T = Ts + 2
    bd = torch.arange(1, T * T + 1, dtype=torch.float64).view(1, 1, T, T)
    want = torch.zeros_like(bd)
    want[..., :Ts, :Ts] = oracle.rel_shift(bd[..., :Ts, :Ts].contiguous())
    assert torch.equal(ar.rel_shift(bd, Ts), want)
    back = ar.rel_unshift(want, Ts)
    head = torch.zeros_like(bd, dtype=torch.bool)
    head[..., 0, :Ts - 1] = True
    inside = torch.zeros_like(head)
    inside[..., :Ts, :Ts] = True
    assert torch.equal(back, torch.where(inside & ~head, bd, torch.zeros_like(bd)))


LONG_CLASSES = [(513, 992, 16, 4), (993, 1984, 16, 8), (1985, 2128, 16, 6), (2129, 2272, 16, 4), (2273, 4000, 8, 8), (4001, 4096, 8, 6)]


def test_route_boundaries():
    for lo, hi, nkt in ((1, 128, 8), (129, 256, 16), (257, 512, 32)):
        for T2 in (lo, hi):
            for dtype in ("f32", "bf16"):
                for rel in (False, True):
                    r = "rel" if rel else "abs"
                    assert ar.route(dtype, rel, T2, T2) == (f"short_{dtype}_fwd<{r},nkt={nkt}>", f"short_{dtype}_bwd_q<{r},nkt={nkt}>")
    for lo, hi, lq, nw in LONG_CLASSES:
        for T2 in (lo, hi):
            assert ar.long_geom(T2) == (lq, nw), T2
            assert ar.attn_long_lds(lq, nw, (T2 + 15) // 16) <= 160 * 1024
            fw, bw = ar.route("bf16", False, 19, T2)
            assert fw == f"long_bf16_fwd<abs,lq={lq},nw={nw}>" and bw == f"long_bf16_bwd_q<abs,lq={lq},nw={8 if nw == 8 else 4}>"
    # the LDS budget is exact at the class edges: one more key tile does not fit the smaller class
    assert ar.attn_long_lds(16, 4, 992 // 16) <= 80 * 1024 < ar.attn_long_lds(16, 4, 993 // 16 + 1)
    assert ar.attn_long_lds(16, 8, 1984 // 16) <= 160 * 1024 < ar.attn_long_lds(16, 8, 1985 // 16 + 1)
    assert ar.attn_long_lds(16, 6, 2128 // 16) <= 160 * 1024 < ar.attn_long_lds(16, 6, 2129 // 16 + 1)
    assert ar.attn_long_lds(16, 4, 2272 // 16) <= 160 * 1024 < ar.attn_long_lds(16, 4, 2273 // 16 + 1)
    assert ar.attn_long_lds(8, 8, 4000 // 16) <= 160 * 1024 < ar.attn_long_lds(8, 8, 4001 // 16 + 1)
    routes = ar.all_routes()
    # 3 short tile counts and 6 forward / 4 backward long geometries, x rel x dtype; 3 key-side launches.  The forward's
    # <lq=8, nw=4> is instantiated but no admissible T2 reaches it: eight queries never fit twice in 80 KB, and six waves always fit
    assert len(routes) == 4 * (3 + 3) + 4 * (5 + 4) + 3
    assert not any("fwd" in r and "lq=8,nw=4" in r for r in routes)
    assert ar.route_kv("f32", True) in routes
