"""tests/rnn_restatement.py is right independently of the kernels: every hand-written backward against torch.autograd of
the restated forward in float64 (relative 1e-10), the cells against torch.nn.LSTMCell / GRUCell, the masked sequence against
torch.nn.LSTM on a packed sequence, the pool against F.max_pool2d(ceil_mode=True).  Runs without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import rnn_restatement as rr


REL = 1e-10


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def close(name, got, ref):
    assert got.shape == ref.shape, f"{name}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    mag = max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-300)
    assert err <= REL * mag, f"{name}: max error {err:.3e} against max |ref| {mag:.3e}"


def grads(outs, couts, ins):
    """gradients of sum_i <outs_i, couts_i> with respect to ins (None -> zeros)"""
    loss = sum((o * c).sum() for o, c in zip(outs, couts) if c is not None)
    gs = torch.autograd.grad(loss, ins, allow_unused=True, retain_graph=True)
    return [torch.zeros_like(i) if g is None else g for g, i in zip(gs, ins)]


def live_vec(B):
    lv = torch.ones(B, dtype=torch.uint8)
    lv[0] = 0
    lv[B - 1] = 0
    lv[B // 2] = 0
    return lv


@pytest.mark.parametrize("B,H", [(1, 1), (3, 5), (7, 33)])
@pytest.mark.parametrize("masked", [False, True])
def test_lstm_cell_bwd_vs_autograd(B, H, masked):
    g = gen(B * 100 + H)
    gates, cp, hp = (rnd(g, B, 4 * H).requires_grad_(), rnd(g, B, H).requires_grad_(), rnd(g, B, H).requires_grad_())
    live = live_vec(B) if masked and B > 1 else None
    h, c, y, acts = rr.lstm_cell_fwd(gates, cp, hp, live)
    for dy, dh, dc in [(rnd(g, B, H), rnd(g, B, H), rnd(g, B, H)), (None, rnd(g, B, H), None), (rnd(g, B, H), None, None),
                       (None, None, rnd(g, B, H))]:
        dg_ref, dcp_ref, dhp_ref = grads((y, h, c), (dy, dh, dc), (gates, cp, hp))
        dg, dcp, dhp = rr.lstm_cell_bwd(dy, dh, dc, acts.detach(), cp.detach(), c.detach(), live)
        # the restated dgates are gradients of the pre-activations in acts' layout
        close("dgates", dg, dg_ref)
        close("dc_prev", dcp, dcp_ref)
        close("dh_pass", dhp, dhp_ref)


@pytest.mark.parametrize("B,H", [(1, 1), (3, 5), (7, 33)])
@pytest.mark.parametrize("masked", [False, True])
def test_gru_cell_bwd_vs_autograd(B, H, masked):
    g = gen(B * 100 + H + 1)
    gx, gh, hp = rnd(g, B, 3 * H).requires_grad_(), rnd(g, B, 3 * H).requires_grad_(), rnd(g, B, H).requires_grad_()
    live = live_vec(B) if masked and B > 1 else None
    h, y, acts = rr.gru_cell_fwd(gx, gh, hp, live)
    for dy, dh in [(rnd(g, B, H), rnd(g, B, H)), (None, rnd(g, B, H)), (rnd(g, B, H), None)]:
        dgx_ref, dgh_ref, dhp_ref = grads((y, h), (dy, dh), (gx, gh, hp))
        dgx, dgh, dhd = rr.gru_cell_bwd(dy, dh, acts.detach(), hp.detach(), live)
        close("dgx", dgx, dgx_ref)
        close("dgh", dgh, dgh_ref)
        close("dh_direct", dhd, dhp_ref)      # gh is an input here, so all of dL/dh_prev is the direct share


def test_cells_vs_torch_nn():
    g = gen(5)
    B, I, H = 4, 6, 9
    x, h0, c0 = rnd(g, B, I), rnd(g, B, H), rnd(g, B, H)
    lstm = torch.nn.LSTMCell(I, H).double()
    gates = x @ lstm.weight_ih.t() + lstm.bias_ih + h0 @ lstm.weight_hh.t() + lstm.bias_hh
    h, c, y, _ = rr.lstm_cell_fwd(gates, c0)
    h_ref, c_ref = lstm(x, (h0, c0))
    close("LSTMCell h", h.detach(), h_ref.detach())
    close("LSTMCell c", c.detach(), c_ref.detach())
    close("LSTMCell y", y.detach(), h_ref.detach())
    h2 = rr.lstm_step_fwd(x @ lstm.weight_ih.t() + lstm.bias_ih, lstm.weight_hh, lstm.bias_hh, h0, c0)[0]
    close("lstm_step h", h2.detach(), h_ref.detach())
    gru = torch.nn.GRUCell(I, H).double()
    hg, yg, _ = rr.gru_cell_fwd(x @ gru.weight_ih.t() + gru.bias_ih, h0 @ gru.weight_hh.t() + gru.bias_hh, h0)
    close("GRUCell h", hg.detach(), gru(x, h0).detach())
    close("GRUCell y", yg.detach(), gru(x, h0).detach())


@pytest.mark.parametrize("reverse", [False, True])
def test_lstm_seq_vs_packed_nn_lstm(reverse):
    """one direction of a bidirectional torch.nn.LSTM on a packed sequence: y (zero past each length), the final state, and
    through autograd the gradient of gx = dgates"""
    g = gen(7)
    T, B, I, H = 6, 5, 4, 8
    lens = torch.tensor([6, 1, 4, 6, 3])
    live = (torch.arange(T).unsqueeze(1) < lens.unsqueeze(0)).to(torch.uint8)
    lstm = torch.nn.LSTM(I, H, bidirectional=True).double()
    sfx = "_reverse" if reverse else ""
    w_ih, w_hh = getattr(lstm, "weight_ih_l0" + sfx), getattr(lstm, "weight_hh_l0" + sfx)
    b_ih, b_hh = getattr(lstm, "bias_ih_l0" + sfx), getattr(lstm, "bias_hh_l0" + sfx)
    x = rnd(g, T, B, I)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens, enforce_sorted=False)
    out, (hn, cn) = lstm(packed)
    y_ref = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)[0][:, :, H:] if reverse else \
        torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)[0][:, :, :H]
    gx = (x @ w_ih.t() + b_ih).detach().requires_grad_()
    y, h, c, acts = rr.lstm_seq_fwd(gx, w_hh.detach(), b_hh.detach(), live, reverse)
    last = 0 if reverse else T - 1
    close("y", y.detach(), y_ref.detach())
    close("h_n", h[last].detach(), hn[1 if reverse else 0].detach())
    close("c_n", c[last].detach(), cn[1 if reverse else 0].detach())
    dy = rnd(g, T, B, H)
    (dgx_ref,) = torch.autograd.grad((y * dy).sum(), gx)
    dg = rr.lstm_seq_bwd(dy, w_hh.detach(), acts.detach(), c.detach(), live, reverse)
    close("dgates", dg, dgx_ref)
    # unmasked
    y2, h2, c2, acts2 = rr.lstm_seq_fwd(gx, w_hh.detach(), None, None, reverse)
    (dgx2,) = torch.autograd.grad((y2 * dy).sum(), gx)
    close("dgates unmasked", rr.lstm_seq_bwd(dy, w_hh.detach(), acts2.detach(), c2.detach(), None, reverse), dgx2)


def test_lstm_step_bwd_vs_autograd():
    g = gen(11)
    B, H = 5, 6
    gx, w, b = rnd(g, B, 4 * H), rnd(g, 4 * H, H), rnd(g, 4 * H)
    hp, cp = rnd(g, B, H).requires_grad_(), rnd(g, B, H).requires_grad_()
    gxr = gx.clone().requires_grad_()
    live = live_vec(B)
    h, c, y, acts = rr.lstm_step_fwd(gxr, w, b, hp, cp, live)
    dy, dh, dc = rnd(g, B, H), rnd(g, B, H), rnd(g, B, H)
    dg_ref, dhp_ref, dcp_ref = grads((y, h, c), (dy, dh, dc), (gxr, hp, cp))
    # dh arrives as pass-through + dgates_next W_hh: split an arbitrary dh that way
    dgn = rnd(g, B, 4 * H)
    dg, dcp, dpass = rr.lstm_step_bwd(dy, dgn, w, dh - dgn @ w, dc, acts.detach(), cp.detach(), c.detach(), live)
    close("dgates", dg, dg_ref)
    close("dc_prev", dcp, dcp_ref)
    close("dh_prev", dpass + dg @ w, dhp_ref)


@pytest.mark.parametrize("shape", [(2, 9, 7, 5), (1, 1, 1, 3), (3, 2, 5, 4), (2, 4, 6, 3)])
def test_maxpool_vs_torch(shape):
    g = gen(sum(shape))
    x = rnd(g, *shape).requires_grad_()                    # tie-free
    y, idx = rr.maxpool2x2_fwd(x)
    y_ref = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1)
    close("pool y", y.detach(), y_ref.detach())
    dy = rnd(g, *y.shape)
    (dx_ref,) = torch.autograd.grad((y_ref * dy).sum(), x)
    (dx_auto,) = torch.autograd.grad((y * dy).sum(), x)
    dx = rr.maxpool2x2_bwd(dy, idx, shape)
    close("pool dx vs F.max_pool2d", dx, dx_ref)
    close("pool dx vs autograd of the restatement", dx, dx_auto)


def test_maxpool_first_maximum_wins():
    x = torch.tensor([[1.0, 1.0, 0.0], [1.0, 2.0, 0.0], [-1.0, -1.0, float("-inf")]]).reshape(1, 3, 3, 1)
    y, idx = rr.maxpool2x2_fwd(x)
    assert y.reshape(-1).tolist() == [2.0, 0.0, -1.0, float("-inf")]
    assert idx.reshape(-1).tolist() == [3, 0, 0, 0]
    x = torch.ones(1, 2, 2, 1)
    assert rr.maxpool2x2_fwd(x)[1].item() == 0
    dx = rr.maxpool2x2_bwd(torch.full((1, 1, 1, 1), 5.0), torch.tensor([[[[2]]]], dtype=torch.uint8), (1, 2, 2, 1))
    assert dx.reshape(-1).tolist() == [0.0, 0.0, 5.0, 0.0]


ATTLOC_CASES = [(2, 7, 8, 3, 5, 1, 6), (3, 9, 6, 10, 3, 1, 5), (2, 5, 4, 2, 11, 3, 3), (1, 1, 3, 1, 1, 1, 1), (2, 6, 5, 0, 0, 1, 4)]


@pytest.mark.parametrize("B,T,A,C,K,R,E", ATTLOC_CASES)
@pytest.mark.parametrize("scaling", [1.0, 2.0])
def test_attloc_bwd_vs_autograd(B, T, A, C, K, R, E, scaling):
    g = gen(B + T * 3 + A * 5 + C * 7 + K + R)
    lens = torch.randint(1, T + 1, (B,), generator=g).int()
    lens[0] = T
    pre, dec, gvec, gb, enc = (rnd(g, B, T, A).requires_grad_(), rnd(g, B, A).requires_grad_(), rnd(g, A).requires_grad_(),
                               rnd(g, 1).requires_grad_(), rnd(g, B, T, E).requires_grad_())
    if C:
        prev = torch.softmax(rnd(g, B, R, T), dim=2).requires_grad_()
        cw, wa = rnd(g, C, R, K).requires_grad_(), rnd(g, A, C).requires_grad_()
    else:
        prev = cw = wa = None
    e, th, conv, w, ctx = rr.attloc_fwd(prev, cw, wa, pre, dec, gvec, gb, lens, enc, scaling)
    mask = rr.frame_mask(lens, T)
    assert bool(torch.isinf(e[~mask]).all()) and bool((w[~mask] == 0).all())
    dctx, dw_ext = rnd(g, B, E), rnd(g, B, T)
    ins = [pre, dec, gvec, gb, enc] + ([prev, cw, wa] if C else [])
    ref = grads((ctx, w), (dctx, dw_ext), ins)
    d = lambda t: None if t is None else t.detach()
    de, deh, df, dgvec, dgb, ddec = rr.attloc_bwd_energy(dctx, dw_ext, d(w), d(enc), d(th), d(gvec), scaling)
    assert bool((de[~mask] == 0).all()) and bool((df[~mask] == 0).all())
    close("df", df, ref[0])
    close("d_dec_proj", ddec, ref[1])
    close("dgvec", dgvec, ref[2])
    assert abs(float(dgb) - float(ref[3])) <= REL * float(de.abs().sum())          # exactly 0 but for rounding
    close("d_enc_h", deh, ref[4])
    if C:
        out = rr.attloc_bwd_energy_conv(dctx, dw_ext, d(w), d(enc), d(th), d(gvec), scaling, d(conv), d(wa))
        close("dw_att", out[7], ref[7])
        d_prev, dcw = rr.attloc_bwd_conv(out[6], d(cw), d(prev))
        close("d_prev", d_prev, ref[5])
        close("dconv_w", dcw, ref[6])
        (dconv_ref,) = torch.autograd.grad((ctx * dctx).sum() + (w * dw_ext).sum(), conv, retain_graph=True)
        close("dconv", out[6], dconv_ref)
    # dw_ext None
    ref2 = grads((ctx,), (dctx,), ins)
    out2 = rr.attloc_bwd_energy(dctx, None, d(w), d(enc), d(th), d(gvec), scaling)
    close("df, dw_ext None", out2[2], ref2[0])
    assert rr.attloc_bwd_workspace(B, T, A, max(C, 1)) == B * ((T + 31) // 32) * A * (max(C, 1) + 2) * 4


def test_loc_conv_vs_conv1d():
    g = gen(3)
    for B, R, T, C, K in [(2, 1, 9, 3, 5), (2, 3, 4, 2, 11), (1, 1, 1, 1, 1)]:
        p, w = rnd(g, B, R, T), rnd(g, C, R, K)
        close("loc_conv", rr.loc_conv(p, w), F.conv1d(p, w, padding=(K - 1) // 2).transpose(1, 2))


@pytest.mark.parametrize("B,T,C,K", [(2, 9, 3, 5), (1, 1, 1, 1), (3, 4, 2, 11), (2, 70, 4, 3)])
def test_convmax_bwd_vs_autograd(B, T, C, K):
    g = gen(B + T + C + K)
    prev, cw = torch.softmax(rnd(g, B, T), dim=1).requires_grad_(), rnd(g, C, K).requires_grad_()
    cw.data[0] = -cw.data[0].abs()                         # a row that is nowhere positive: pooled 0, no gradient
    pooled, idx = rr.convmax_fwd(prev, cw)
    ref_p = torch.relu(F.conv1d(prev.unsqueeze(1), cw.unsqueeze(1), padding=(K - 1) // 2)).max(dim=2)
    close("pooled", pooled.detach(), ref_p.values.detach())
    assert bool((pooled[:, 0] == 0).all())
    assert torch.equal(idx.long()[pooled > 0], ref_p.indices[pooled > 0])
    dpool = rnd(g, B, C)
    dp_ref, dw_ref = grads((pooled,), (dpool,), (prev, cw))
    d_prev, dcw = rr.convmax_bwd(dpool, pooled.detach(), idx, prev.detach(), cw.detach())
    close("d_prev", d_prev, dp_ref)
    close("dconv_w", dcw, dw_ref)
    assert bool((dcw[0] == 0).all())


def test_convmax_ties_go_to_the_earliest_frame():
    prev = torch.tensor([[0.25, 0.5, 0.5, 0.25, 0.5]])
    pooled, idx = rr.convmax_fwd(prev, torch.tensor([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]))
    assert idx.tolist() == [[1, 0]] and pooled.tolist() == [[0.5, 0.0]]


@pytest.mark.parametrize("B,T,A,E", [(2, 9, 5, 4), (1, 1, 1, 1), (3, 4, 7, 6)])
def test_dot_attention_bwd_vs_autograd(B, T, A, E):
    g = gen(B * 7 + T + A + E)
    lens = torch.randint(1, T + 1, (B,), generator=g).int()
    k, q, v = rnd(g, B, T, A).requires_grad_(), rnd(g, B, A).requires_grad_(), rnd(g, B, T, E).requires_grad_()
    e = rr.att_dot_energy_fwd(k, q, lens)
    mask = rr.frame_mask(lens, T)
    assert bool(torch.isinf(e[~mask]).all())
    w, ctx = rr.att_ctx_fwd(e, v, 2.0)
    dctx, dw_ext = rnd(g, B, E), rnd(g, B, T)
    dk_ref, dq_ref, dv_ref = grads((ctx, w), (dctx, dw_ext), (k, q, v))
    de, d_v, dsum = rr.att_ctx_bwd(dctx, dw_ext, w.detach(), v.detach(), 2.0)
    dk, dq = rr.att_dot_energy_bwd(de, k.detach(), q.detach())
    close("d_v", d_v, dv_ref)
    close("dk", dk, dk_ref)
    close("dq", dq, dq_ref)
    assert abs(float(dsum)) <= REL * float(de.abs().sum()) + 1e-300
    # softmax + context alone, on finite energies
    e2 = rnd(g, B, T).requires_grad_()
    w2, ctx2 = rr.att_ctx_fwd(e2, v, 0.5)
    (de_ref,) = torch.autograd.grad((ctx2 * dctx).sum() + (w2 * dw_ext).sum(), e2)
    close("de", rr.att_ctx_bwd(dctx, dw_ext, w2.detach(), v.detach(), 0.5)[0], de_ref)
