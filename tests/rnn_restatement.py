"""Plain float64 statements of what the kernels of csrc/rnn.hip and csrc/lstm_seq.hip compute, written from the formulas in
their comments: LSTM / GRU cells with the `live` rule of packed sequences, the 2x2 ceil-mode max-pool, location-aware
attention (forward and the three backward stages), the conv + ReLU + arg-max front end of AttLocRec, dot-product energies,
softmax + context, one LSTM time step and a whole masked, optionally reversed LSTM sequence with its backward.

Everything takes and returns CPU tensors; inputs of any float type are computed on in float64.  `live` is a uint8 / bool
vector (None = every row live): a dead row carries its state through unchanged and its output row is +0.  Forward functions
are differentiable torch code, so tests/test_rnn_restatement.py can check every hand-written backward against autograd."""
import torch
import torch.nn.functional as F


def _d(t):
    return None if t is None else t.double()


def _live(live, B):
    if live is None:
        return torch.ones(B, 1, dtype=torch.bool)
    return live.reshape(B, 1) != 0


def _z(*shape):
    return torch.zeros(*shape, dtype=torch.float64)


# ---- LSTM cell (gate order i, f, g, o) --------------------------------------------------------------------------------
def lstm_cell_fwd(gates, c_prev, h_prev=None, live=None):
    """gates [B, 4H] pre-activations -> h, c, y, acts [B, 4H] (the four gate values)"""
    gates, c_prev, h_prev = _d(gates), _d(c_prev), _d(h_prev)
    B, H = c_prev.shape
    gi, gf, gg, go = gates.reshape(B, 4, H).unbind(1)
    i, f, g, o = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
    c = f * c_prev + i * g
    h = o * torch.tanh(c)
    y = h
    if live is not None:
        lv = _live(live, B)
        c, h, y = torch.where(lv, c, c_prev), torch.where(lv, h, h_prev), torch.where(lv, h, torch.zeros_like(h))
    return h, c, y, torch.cat([i, f, g, o], dim=1)


def lstm_cell_bwd(dy, dh, dc, acts, c_prev, c, live=None):
    """dy: gradient of y, dh / dc: gradients of h / c arriving from the next step (None = 0) -> dgates [B, 4H], dc_prev,
    dh_pass (the share that goes straight to h_prev: dh on a dead row, 0 on a live one)"""
    acts, c_prev, c = _d(acts), _d(c_prev), _d(c)
    B, H = c.shape
    dy, dh, dc = (_z(B, H) if t is None else _d(t) for t in (dy, dh, dc))
    i, f, g, o = acts.reshape(B, 4, H).unbind(1)
    dhv = dh + dy
    tc = torch.tanh(c)
    dct = dc + dhv * o * (1 - tc * tc)
    dg = torch.cat([dct * g * i * (1 - i), dct * c_prev * f * (1 - f), dct * i * (1 - g * g), dhv * tc * o * (1 - o)], dim=1)
    lv = _live(live, B)
    return (torch.where(lv, dg, torch.zeros_like(dg)), torch.where(lv, dct * f, dc), torch.where(lv, torch.zeros_like(dh), dh))


# ---- GRU cell (gate order r, z, n) ------------------------------------------------------------------------------------
def gru_cell_fwd(gx, gh, h_prev, live=None):
    """gx = x W_ih^T + b_ih, gh = h W_hh^T + b_hh, both [B, 3H] -> h, y, acts [B, 4H] = (r, z, n, gh_n)"""
    gx, gh, h_prev = _d(gx), _d(gh), _d(h_prev)
    B, H = h_prev.shape
    xr, xz, xn = gx.reshape(B, 3, H).unbind(1)
    hr, hz, hn = gh.reshape(B, 3, H).unbind(1)
    r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
    n = torch.tanh(xn + r * hn)
    h = (1 - z) * n + z * h_prev
    y = h
    if live is not None:
        lv = _live(live, B)
        h, y = torch.where(lv, h, h_prev), torch.where(lv, h, torch.zeros_like(h))
    return h, y, torch.cat([r, z, n, hn], dim=1)


def gru_cell_bwd(dy, dh, acts, h_prev, live=None):
    """-> dgx, dgh [B, 3H], dh_direct [B, H] (what reaches h_prev without W_hh: z * d, or all of dh on a dead row)"""
    acts, h_prev = _d(acts), _d(h_prev)
    B, H = h_prev.shape
    dy, dh = (_z(B, H) if t is None else _d(t) for t in (dy, dh))
    r, z, n, ghn = acts.reshape(B, 4, H).unbind(1)
    d = dh + dy
    dn = d * (1 - z) * (1 - n * n)
    dz = d * (h_prev - n) * z * (1 - z)
    dr = dn * ghn * r * (1 - r)
    dgx, dgh = torch.cat([dr, dz, dn], dim=1), torch.cat([dr, dz, dn * r], dim=1)
    lv = _live(live, B)
    zero = torch.zeros_like(dgx)
    return torch.where(lv, dgx, zero), torch.where(lv, dgh, zero), torch.where(lv, d * z, dh)


# ---- 2x2 / stride-2 max-pool, ceil mode, NHWC -------------------------------------------------------------------------
def _pool_windows(x):
    """x [B, H, W, C] -> values [4, B, Ho, Wo, C] in the order (0,0), (0,1), (1,0), (1,1) and which of them exist"""
    B, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(x, (0, 0, 0, 2 * Wo - W, 0, 2 * Ho - H))
    ok = F.pad(torch.ones(H, W, dtype=torch.bool), (0, 2 * Wo - W, 0, 2 * Ho - H))
    v = torch.stack([xp[:, a::2, b::2] for a in (0, 1) for b in (0, 1)])
    m = torch.stack([ok[a::2, b::2] for a in (0, 1) for b in (0, 1)]).reshape(4, 1, Ho, Wo, 1)
    return v, m


def maxpool2x2_fwd(x):
    """-> y [B, ceil(H/2), ceil(W/2), C] and idx (uint8, 0..3): the first maximum in window order wins; a window that is
    all -inf gives -inf and idx 0 (nothing is greater than the -inf the search starts from)"""
    x = _d(x)
    v, m = _pool_windows(x)
    best = torch.full_like(v[0], float("-inf"))
    idx = torch.zeros(v[0].shape, dtype=torch.uint8)
    for k in range(4):
        upd = m[k] & (v[k] > best)
        best = torch.where(upd, v[k], best)
        idx = torch.where(upd, torch.full_like(idx, k), idx)
    return best, idx


def maxpool2x2_bwd(dy, idx, shape):
    """dx[b, h, w, c] = dy of its window where idx names this position, else 0"""
    dy = _d(dy)
    B, H, W, C = shape
    up = lambda t: t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W]
    k = (torch.arange(H).reshape(1, H, 1, 1) % 2) * 2 + torch.arange(W).reshape(1, 1, W, 1) % 2
    return torch.where(up(idx.long()) == k, up(dy), torch.zeros((), dtype=torch.float64))


# ---- location-aware attention -----------------------------------------------------------------------------------------
def loc_conv(att_prev, conv_w):
    """conv[b, t, c] = sum_{r, k} conv_w[c, r, k] * att_prev[b, r, t + k - F], F = (K - 1) / 2, zero outside the sequence;
    att_prev [B, R, T] (or [B, T]: R = 1), conv_w [C, R, K] (or [C, K])"""
    att_prev, conv_w = _d(att_prev), _d(conv_w)
    B, T = att_prev.shape[0], att_prev.shape[-1]
    C, K = conv_w.shape[0], conv_w.shape[-1]
    p, w = att_prev.reshape(B, -1, T), conv_w.reshape(C, -1, K)
    Fh = (K - 1) // 2
    pp = F.pad(p, (Fh, Fh))
    out = _z(B, T, C)
    for k in range(K):
        out = out + torch.einsum("brt,cr->btc", pp[:, :, k:k + T], w[:, :, k])
    return out


def frame_mask(lens, T):
    return torch.arange(T).unsqueeze(0) < lens.reshape(-1, 1).long()


def att_ctx_fwd(e, v, scaling):
    """w = softmax(scaling * e) over the frames, ctx[b] = sum_t w[b, t] v[b, t]"""
    e, v = _d(e), _d(v)
    w = torch.softmax(scaling * e, dim=1)
    return w, torch.einsum("bt,bte->be", w, v)


def attloc_fwd(att_prev, conv_w, w_att, pre_enc, dec_proj, gvec, gb, lens, enc_h, scaling):
    """-> e, th, conv, w, ctx; conv_w None: additive attention (no location term, conv is None)"""
    pre_enc, dec_proj, gvec, gb = _d(pre_enc), _d(dec_proj), _d(gvec), _d(gb)
    B, T, A = pre_enc.shape
    f = pre_enc + dec_proj.unsqueeze(1)
    conv = None
    if conv_w is not None:
        conv = loc_conv(att_prev, conv_w)
        f = f + conv @ _d(w_att).t()
    th = torch.tanh(f)
    e = th @ gvec.reshape(A) + gb.reshape(())
    e = torch.where(frame_mask(lens, T), e, torch.full_like(e, float("-inf")))
    w, ctx = att_ctx_fwd(e, enc_h, scaling)
    return e, th, conv, w, ctx


def att_ctx_bwd(dctx, dw_ext, w, v, scaling):
    """backward of softmax + context -> de, d_v, dsum = sum of de (the gradient of a bias added to every energy)"""
    dctx, w, v = _d(dctx), _d(w), _d(v)
    dw = torch.einsum("bte,be->bt", v, dctx)
    if dw_ext is not None:
        dw = dw + _d(dw_ext)
    d_v = w.unsqueeze(2) * dctx.unsqueeze(1)
    s = (w * dw).sum(1, keepdim=True)
    de = scaling * w * (dw - s)
    return de, d_v, de.sum()


def attloc_bwd_energy(dctx, dw_ext, w, enc_h, th, gvec, scaling):
    """-> de, d_enc_h, df, dgvec, dgb, d_dec_proj"""
    th, gvec = _d(th), _d(gvec).reshape(-1)
    de, d_enc_h, dgb = att_ctx_bwd(dctx, dw_ext, w, enc_h, scaling)
    df = de.unsqueeze(2) * gvec * (1 - th * th)
    dgvec = torch.einsum("bt,bta->a", de, th)
    return de, d_enc_h, df, dgvec, dgb, df.sum(1)


def attloc_bwd_energy_conv(dctx, dw_ext, w, enc_h, th, gvec, scaling, conv, w_att):
    """the same plus dconv = df @ W_att and dw_att = sum_{b, t} df^T conv"""
    out = attloc_bwd_energy(dctx, dw_ext, w, enc_h, th, gvec, scaling)
    df = out[2]
    return out + (df @ _d(w_att), torch.einsum("bta,btc->ac", df, _d(conv)))


def attloc_bwd_workspace(B, T, A, C):
    """bytes: per (utterance, chunk of 32 frames) A * (C + 2) fp32 partial sums"""
    return B * (-(-T // 32)) * A * (C + 2) * 4


def attloc_bwd_conv(dconv, conv_w, att_prev):
    """d_prev[b, r, s] = sum_{c, k} dconv[b, s - k + F, c] conv_w[c, r, k];
    dconv_w[c, r, k] = sum_{b, t} dconv[b, t, c] att_prev[b, r, t + k - F]"""
    dconv, conv_w, att_prev = _d(dconv), _d(conv_w), _d(att_prev)
    B, T, C = dconv.shape
    K = conv_w.shape[-1]
    w, p = conv_w.reshape(C, -1, K), att_prev.reshape(B, -1, T)
    R = w.shape[1]
    Fh = (K - 1) // 2
    pp = F.pad(p, (Fh, Fh))
    dp = _z(B, R, T + 2 * Fh)
    dw = _z(C, R, K)
    for k in range(K):
        dp[:, :, k:k + T] += torch.einsum("btc,cr->brt", dconv, w[:, :, k])
        dw[:, :, k] = torch.einsum("btc,brt->cr", dconv, pp[:, :, k:k + T])
    return dp[:, :, Fh:Fh + T].reshape(att_prev.shape), dw.reshape(conv_w.shape)


# ---- AttLocRec front end: conv + ReLU + max over the frames -----------------------------------------------------------
def convmax_fwd(att_prev, conv_w):
    """att_prev [B, T], conv_w [C, K] -> pooled [B, C] = max_t relu(conv[b, t, c]), idx = the earliest frame of the largest
    conv value (whatever its sign)"""
    conv = loc_conv(att_prev, conv_w)                      # [B, T, C]
    T = conv.shape[1]
    best = conv.max(dim=1, keepdim=True).values
    frames = torch.arange(T).reshape(1, T, 1).expand_as(conv)
    idx = torch.where(conv == best, frames, torch.full_like(frames, T)).min(dim=1).values
    pooled = torch.clamp(conv.gather(1, idx.unsqueeze(1)).squeeze(1), min=0)
    return pooled, idx.int()


def convmax_bwd(dpool, pooled, idx, att_prev, conv_w):
    """only the arg-max frame carries gradient, and only where the ReLU was active (pooled > 0)"""
    dpool, pooled, att_prev, conv_w = _d(dpool), _d(pooled), _d(att_prev), _d(conv_w)
    B, T = att_prev.shape
    C, K = conv_w.shape[0], conv_w.shape[-1]
    w = conv_w.reshape(C, K)
    Fh = (K - 1) // 2
    g = torch.where(pooled > 0, dpool, torch.zeros_like(dpool))                   # [B, C]
    ts = idx.long().unsqueeze(2) + torch.arange(K).reshape(1, 1, K) - Fh            # [B, C, K]
    ok = (ts >= 0) & (ts < T)
    tsc = ts.clamp(0, T - 1)
    contrib = torch.where(ok, g.unsqueeze(2) * w.unsqueeze(0), _z(1))
    d_prev = _z(B, T).scatter_add_(1, tsc.reshape(B, C * K), contrib.reshape(B, C * K))
    pv = torch.gather(att_prev.unsqueeze(1).expand(B, C, T), 2, tsc)
    dconv_w = torch.where(ok, g.unsqueeze(2) * pv, _z(1)).sum(0)
    return d_prev, dconv_w.reshape(conv_w.shape)


# ---- dot-product attention energies -----------------------------------------------------------------------------------
def att_dot_energy_fwd(k, q, lens):
    """e[b, t] = sum_a k[b, t, a] q[b, a]; -inf for t >= lens[b]"""
    k, q = _d(k), _d(q)
    e = torch.einsum("bta,ba->bt", k, q)
    return torch.where(frame_mask(lens, k.shape[1]), e, torch.full_like(e, float("-inf")))


def att_dot_energy_bwd(de, k, q):
    de, k, q = _d(de), _d(k), _d(q)
    return de.unsqueeze(2) * q.unsqueeze(1), torch.einsum("bt,bta->ba", de, k)


# ---- LSTM steps and sequences -----------------------------------------------------------------------------------------
def lstm_step_fwd(gx, w_hh, b_hh, h_prev, c_prev, live=None):
    """gates = gx + b_hh + h_prev W_hh^T (w_hh [4H, H]), then the cell"""
    gates = _d(gx) + _d(h_prev) @ _d(w_hh).t()
    if b_hh is not None:
        gates = gates + _d(b_hh)
    return lstm_cell_fwd(gates, c_prev, h_prev, live)


def lstm_step_bwd(dy, dgates_next, w_hh, dh_pass_in, dc, acts, c_prev, c, live=None):
    """dh = dh_pass_in + dgates_next W_hh (either may be None), then the cell backward"""
    B, H = c.shape
    dh = _z(B, H) if dh_pass_in is None else _d(dh_pass_in)
    if dgates_next is not None:
        dh = dh + _d(dgates_next) @ _d(w_hh)
    return lstm_cell_bwd(dy, dh, dc, acts, c_prev, c, live)


def lstm_seq_fwd(gx, w_hh, b_hh, live=None, reverse=False):
    """gx [T, B, 4H], live [T, B] or None; the state starts at zero and walks the frames backwards if reverse.
    -> y, h, c [T, B, H] (the state after each frame; the final state is that of the last frame walked), acts [T, B, 4H]"""
    T, B, H4 = gx.shape
    H = H4 // 4
    h, c = _z(B, H), _z(B, H)
    ys, hs, cs, As = [None] * T, [None] * T, [None] * T, [None] * T
    for s in range(T):
        t = T - 1 - s if reverse else s
        h, c, ys[t], As[t] = lstm_step_fwd(gx[t], w_hh, b_hh, h, c, None if live is None else live[t])
        hs[t], cs[t] = h, c
    return torch.stack(ys), torch.stack(hs), torch.stack(cs), torch.stack(As)


def lstm_seq_bwd(dy, w_hh, acts, c, live=None, reverse=False):
    """dy [T, B, H] or None, acts / c as lstm_seq_fwd returns them (reverse = the FORWARD direction); no gradient arrives
    at the final state.  -> dgates [T, B, 4H], the gradient of every step's gate pre-activations (= of gx)"""
    T, B, H = c.shape
    dgs = [None] * T
    dg, dc, dpass = None, None, None
    for s in range(T):
        t = s if reverse else T - 1 - s
        pt = t + 1 if reverse else t - 1
        c_prev = c[pt] if 0 <= pt < T else _z(B, H)
        dg, dc, dpass = lstm_step_bwd(None if dy is None else dy[t], dg, w_hh, dpass, dc, acts[t], c_prev, c[t],
                                      None if live is None else live[t])
        dgs[t] = dg
    return torch.stack(dgs)
