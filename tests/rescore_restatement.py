"""Pure-torch float64 restatement of second-pass n-best rescoring (csrc/rescore.hip, include/espnet_amd.h): the pack of the
first pass's n-best into teacher-forcing operands, the merge of the row-statistics tile partials, the per-scorer terms, the
combined score f and the ranking with its stable tie rule.  Shared by the CPU and the GPU tests; it runs no project code."""
import math

import numpy as np
import torch

EPS32 = 2.0 ** -24


def make_nbest(hyps, T):
    """hyps[b][n] = (s1, tokens) or None (absent) -> int32 [B, N, 2 + T] as eamd_ctc_prefix_beam writes it"""
    B, N = len(hyps), len(hyps[0])
    out = np.zeros((B, N, 2 + T), dtype=np.int32)
    for b in range(B):
        assert len(hyps[b]) == N
        for n, h in enumerate(hyps[b]):
            if h is None:
                out[b, n, 1] = -1
                continue
            s1, toks = h
            assert len(toks) <= T
            out[b, n, 0] = np.float32(s1).view(np.int32)
            out[b, n, 1] = len(toks)
            out[b, n, 2:2 + len(toks)] = toks
    return torch.from_numpy(out)


def pack(nbest, U, sos, eos):
    """-> (ys_in [B*N, U] int64, col [B*N*U] int32, ulen [B*N] int32), vectorised"""
    B, N, W = nbest.shape
    rows = nbest.reshape(B * N, W).long()
    L = rows[:, 1]
    here = L >= 0
    Lc = L.clamp(min=0, max=U - 1)
    pos = torch.arange(U).view(1, U)
    toks = torch.zeros(B * N, U + 1, dtype=torch.int64)
    k = min(U, W - 2)
    toks[:, :k] = rows[:, 2:2 + k]
    nxt = torch.where(pos < Lc.view(-1, 1), toks[:, :U], torch.where(pos == Lc.view(-1, 1), torch.tensor(eos), torch.tensor(-1)))
    nxt = torch.where(here.view(-1, 1), nxt, torch.tensor(-1))
    prev = torch.full((B * N, U), eos, dtype=torch.int64)
    prev[:, 0] = sos
    if U > 1:
        shifted = toks[:, :U - 1]
        prev[:, 1:] = torch.where((pos[:, 1:] - 1 < Lc.view(-1, 1)) & here.view(-1, 1), shifted, torch.tensor(eos))
    ulen = torch.where(here, Lc + 1, torch.zeros_like(Lc))
    return prev, nxt.reshape(-1).to(torch.int32), ulen.to(torch.int32)


def tile_partials(logits, tile):
    """what eamd_gemm's row-statistics epilogue leaves for logits [rows, V]: part [rows, ceil(V / tile), 2] = per column tile
    (max, sum exp(v - max)), in the dtype of logits"""
    rows, V = logits.shape
    tn = (V + tile - 1) // tile
    part = logits.new_zeros(rows, tn, 2)
    for j in range(tn):
        blk = logits[:, j * tile:(j + 1) * tile]
        m = blk.max(dim=1).values
        part[:, j, 0] = m
        part[:, j, 1] = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(blk - m.view(-1, 1)).sum(1))
    return part


def merge_lse(part):
    """part [rows, tiles, 2] -> the rows' log-sum-exp, float64"""
    part = part.double()
    mx, sm = part[..., 0], part[..., 1]
    m = mx.max(dim=1).values
    w = torch.where(torch.isinf(mx) & (mx < 0), torch.zeros_like(mx), torch.exp(mx - m.view(-1, 1)))
    return m + torch.log((sm * w).sum(1))


def scorer_terms(part, zcol, ulen, U):
    """-> (term [B*N] float64 = sum_{i < ulen} (zcol - lse), magnitude [B*N] = sum_{i < ulen} (|zcol| + |max| + |log sum| + 1):
    what the a-priori error bound of the fp32 kernel multiplies (see term_bound)"""
    R = ulen.numel()
    lse = merge_lse(part.reshape(R * U, -1, 2)).view(R, U)
    z = zcol.double().view(R, U)
    live = torch.arange(U).view(1, U) < ulen.view(R, 1)
    lp = torch.where(live, z - lse, torch.zeros_like(z))
    m = part.double().reshape(R * U, -1, 2)[..., 0].max(dim=1).values.view(R, U)
    mag = z.abs() + m.abs() + (lse - m).abs() + 1.0
    mag = torch.where(live & torch.isfinite(mag), mag, torch.zeros_like(mag))
    return lp.sum(1), mag.sum(1)


def term_bound(mag, U, tiles_n):
    """A-priori bound on |fp32 term - float64 term|, the rule of the project's float64 kernel tests: (n_terms + 8) * 2^-24 times
    the sum of the magnitudes added, n_terms = U + tiles_n.  Per position the kernel adds zcol, the row maximum and log(sum),
    and the sum's relative error (tiles_n roundings and as many exp calls) becomes an ABSOLUTE error of its logarithm, which
    is why every position also counts a magnitude of 1."""
    return (U + tiles_n + 8) * EPS32 * mag


def combine(s1, terms, weights, w0):
    """f = w0 * s1 + sum_s weights[s] * terms[s] in float64 (a NaN, 0 * -inf, stays a NaN)"""
    f = w0 * s1.double()
    for w, t in zip(weights, terms):
        f = f + w * t
    return f


def rank(f, here):
    """f, here [B, N] -> order [B, N]: f descending (NaN as -inf), equal f to the lower index, absent hypotheses last in their
    own order"""
    B, N = f.shape
    order = torch.zeros(B, N, dtype=torch.int64)
    for b in range(B):
        key = [(-math.inf if (v != v) else v) for v in f[b].tolist()]
        pres = sorted([n for n in range(N) if here[b, n]], key=lambda n: (-key[n], n))
        order[b] = torch.tensor(pres + [n for n in range(N) if not here[b, n]])
    return order


def rescore(nbest, U, scorers, w0):
    """nbest int32 [B, N, 2 + T]; scorers = [(part, zcol, weight)] over the B*N*U rows of pack() ->
    dict(f [B, N] float64 and terms [B, N, 1 + S] float64 in the NEW order, order [B, N], nbest_out rows re-ordered (word 0
    untouched), mags [S][B, N] in the new order)"""
    B, N, W = nbest.shape
    here = nbest[:, :, 1] >= 0
    s1 = torch.from_numpy(nbest[:, :, 0].contiguous().numpy().view(np.float32).astype(np.float64))
    ulen = torch.where(here, nbest[:, :, 1].clamp(max=U - 1) + 1, torch.zeros_like(nbest[:, :, 1])).reshape(-1)
    ts, mags = [], []
    for part, zcol, _ in scorers:
        t, mag = scorer_terms(part, zcol, ulen, U)
        ts.append(t.view(B, N))
        mags.append(mag.view(B, N))
    f = combine(s1, ts, [w for _, _, w in scorers], w0)
    order = rank(f, here)
    g = lambda x: torch.gather(x, 1, order)      # noqa: E731
    terms = torch.stack([g(s1)] + [g(t) for t in ts], dim=2)
    out = torch.gather(nbest, 1, order.view(B, N, 1).expand(B, N, W))
    return dict(f=g(f), terms=terms, order=order, nbest_out=out, mags=[g(m) for m in mags], here=g(here))


def f_bound(res, weights, w0, U, tiles):
    """bound on |fp32 f - float64 f| in the new order: every term's bound times its weight, plus the roundings of the (at most
    three) products and (at most two) sums, 4 * 2^-24 of the magnitudes combined"""
    t = res["terms"]
    b = 4 * EPS32 * abs(w0) * t[..., 0].abs()
    for s, w in enumerate(weights):
        ts = torch.where(torch.isfinite(t[..., 1 + s]), t[..., 1 + s].abs(), torch.zeros_like(t[..., 1 + s]))
        b = b + abs(w) * term_bound(res["mags"][s], U, tiles[s]) + 4 * EPS32 * abs(w) * ts
    return b


def scored_hypotheses(yseqs, scores, eos, maxlen):
    """The hypotheses of a reference n-best whose score is that of an ENDED hypothesis, as [(yseq, score)].  In its last step
    (i == maxlen - 1, maxlen = the encoder frames when maxlenratio = 0) the reference's BeamSearch appends <eos> to every running
    hypothesis without scoring it (espnet/nets/beam_search.py:437-443), after which they count as ended:
      - one that had just chosen <eos> as its maxlen-th token ends in <eos> <eos>: the score is that of the sequence WITHOUT the
        second <eos>, which is what is returned for it;
      - any other of maxlen tokens never had an <eos> scored and carries a CTC PREFIX score, not a sequence log-likelihood: no
        sum over a complete hypothesis recomposes it, and it is left out."""
    out = []
    for y, s in zip(yseqs, scores):
        if len(y) >= 3 and y[-2] == eos:
            out.append((list(y[:-1]), s))
        elif len(y) - 2 < maxlen:
            out.append((list(y), s))
    return out


def ctc_loglik(logp, y, blank=0):
    """log p_ctc(y) for one utterance, float64 forward recursion over logp [T, V] (blank = 0)"""
    logp = logp.double()
    ext = [blank]
    for t in y:
        ext += [int(t), blank]
    S = len(ext)
    idx = torch.tensor(ext)
    skip = torch.tensor([s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] for s in range(S)])
    ninf = torch.full((1,), -math.inf, dtype=torch.float64)
    alpha = torch.full((S,), -math.inf, dtype=torch.float64)
    alpha[0] = logp[0, blank]
    if S > 1:
        alpha[1] = logp[0, ext[1]]
    for t in range(1, logp.shape[0]):
        a1 = torch.cat([ninf, alpha[:-1]])
        a2 = torch.where(skip, torch.cat([ninf, ninf, alpha[:-2]]), ninf.expand(S))
        alpha = torch.logsumexp(torch.stack([alpha, a1, a2]), 0) + logp[t, idx]
    return float(torch.logsumexp(alpha[-2:], 0)) if S > 1 else float(alpha[0])
