"""Support for the batched nsc transducer search tests (not collected: no test_ prefix): the N-step constrained search of
espnet_amd/nets/beam_search_transducer.py (nsc_batch; reference: espnet/nets/beam_search_transducer.py:466-663 without an LM)
restated in numpy float64 and Python lists:

  nsc_step64     one call (frame t, n-step v) of all utterances on the arrays eamd_rnnt_nsc_step reads and writes
                 (csrc/rnnt_nsc.hip);
  nsc_batch64    the whole search in the order nsc_batch runs it - prediction network and joint network of
                 tests/rnnt_greedy_restatement.py on n * W rows per call ((1 + prefix_alpha) n * W on a frame's first), the pair
                 terms of the prefix rescoring by the pair list the previous frame's last call wrote, nsc_step64 for the
                 bookkeeping, the n-best sort at the end - which also reports the smallest float64 gap of every ordering decision
                 that is used and counts prefix terms by depth, hypotheses removed by substract, V lists shorter than W and
                 duplicate sequences in kept.

Hypotheses live in N + 2 blocks of R = n * W rows (N = nstep): block 0 and block N + 1 are the parities of kept, block v
(1 <= v <= N) is the V of n-step v - 1 = the hyps of n-step v; block row = block * R + b * W + w.  With N == 1 block 1 is never
written: V goes straight into the next kept.  A label sequence holds at most ycap = 1 + T N entries.  The lin_dec outputs are stacked
[N + 2][1 + alpha][R]: level 0 = the row's own d, level a = d of its labels without the last a; hrow(block row, level) is a row of
that stack.

tests/test_nsc_restatement.py pins both to a plain per-utterance statement of the algorithm."""
import math

import numpy as np

from alsd_restatement import nbest
from rnnt_greedy_restatement import act64, pred_step64


def new_state(n, W, T, N):
    """the blocks before frame 0: slot 0 of every utterance's kept (parity 0 = block 0) holds [blank] with score 0"""
    st = dict(score=np.zeros((N + 2, n, W)), ulen=np.zeros((N + 2, n, W), np.int32), count=np.zeros((N + 2, n), np.int32),
              yseq=np.zeros((N + 2, n, W, 1 + T * N), np.int32))
    st["count"][0] = 1
    return st


def new_s(n, W, N):
    return dict(score=np.zeros((n, W * N)), src=np.zeros((n, W * N), np.int32), nS=np.zeros(n, np.int32))


def new_pairs(n, W, alpha):
    """the pair list before frame 0: [blank] has no prefix"""
    pairs = np.zeros((max(1, n * W * alpha), 2), np.int32)
    pairs[:, 0] = -1
    return pairs


def kept_block(N, p):
    return N + 1 if p else 0


def _key(s):
    return -math.inf if s != s else s


def _gaps(stats, srt, W):
    if stats is not None:
        for a, c in zip(srt[:W], srt[1:W + 1]):
            stats["sort_gap"] = min(stats.get("sort_gap", math.inf), _key(a[0]) - _key(c[0]))


def _bump(stats, name, by=1):
    if stats is not None and by:
        stats[name] = stats.get(name, 0) + by


def nsc_step64(rec, pair_lp, hlens, st, S, pairs, V, T, N, alpha, t, v, p, stats=None):
    """rec [n * W, 1 + 2k] as eamd_transducer_expand_rows writes it for the rows of hyps' block, pair_lp [n * W * alpha] of the
    frame's first pass, hlens [n] or None, st / S / pairs as new_state / new_s / new_pairs
    -> (blocks, S, par [n * W], tok, live, hidx [1 + alpha, n * W], pairs) after the call; the inputs are not modified, and what the
    kernel does not write keeps the value it had.  stats (dict, optional) accumulates: sort_gap = the smallest difference of
    adjacent scores of the sorted extensions that substract leaves and of sorted S + V, both down to position W + 1; prefix1 /
    prefix2 / prefix3 = rescoring terms by depth; substracted; short_v = V lists shorter than W; dup_kept = entries of a new kept
    whose labels an earlier entry holds."""
    _blocks, n, W = st["score"].shape
    k = min(W, V - 1)
    R, LV = n * W, 1 + alpha
    ycap = 1 + T * N
    rec = np.asarray(rec).reshape(R, 1 + 2 * k)
    pair_lp = np.asarray(pair_lp).reshape(-1)
    st = {key: x.copy() for key, x in st.items()}
    S = {key: x.copy() for key, x in S.items()}
    pairs = np.array(pairs, np.int32).reshape(-1, 2)
    flat_ulen, flat_yseq = st["ulen"].reshape(-1), st["yseq"].reshape(-1, ycap)      # views: block rows
    par = np.zeros(R, np.int32)
    tok = np.zeros(R, np.int64)
    live = np.zeros(R, np.uint8)
    hidx = np.zeros((LV, R), np.int32)
    hrow = lambda br, lvl: ((br // R) * LV + lvl) * R + br % R      # noqa: E731
    kp, ko = kept_block(N, p), kept_block(N, 1 - p)
    last = N == 1 or v == N
    assert 0 <= v <= (0 if N == 1 else N)
    cin = kp if v == 0 else v
    cout = ko if last else v + 1
    for b in range(n):
        Tb = T if hlens is None else max(0, min(int(hlens[b]), T))
        own = cin * R + b * W
        if t >= Tb:
            for w in range(W):
                par[b * W + w] = kp * R + b * W + w
                hidx[:, b * W + w] = [hrow(kp * R + b * W + w, a) for a in range(LV)]
            if last:
                nb = int(st["count"][kp, b])
                st["count"][ko, b] = nb
                for w in range(nb):
                    u = int(st["ulen"][kp, b, w])
                    st["score"][ko, b, w], st["ulen"][ko, b, w] = st["score"][kp, b, w], u
                    st["yseq"][ko, b, w, :u + 1] = st["yseq"][kp, b, w, :u + 1]
            continue
        # [score, labels, block row, token or None]
        hyps = [[float(st["score"][cin, b, w]), [int(x) for x in st["yseq"][cin, b, w, :int(st["ulen"][cin, b, w]) + 1]], own + w,
                 None] for w in range(int(st["count"][cin, b]))]
        if v < N:
            if v == 0:
                hyps = sorted(hyps, key=lambda x: len(x[1]), reverse=True)
                was = [x[0] for x in hyps]
                for j in range(len(hyps) - 1):
                    yj = hyps[j][1]
                    for i in range(j + 1, len(hyps)):
                        yi = hyps[i][1]
                        delta = len(yj) - len(yi)
                        if delta >= 1 and yj[:len(yi)] == yi and delta <= alpha:
                            curr = was[i]
                            for a in range(delta, 0, -1):
                                curr += float(pair_lp[(hyps[j][2] - own + b * W) * alpha + a - 1])
                            hyps[j][0] = float(np.logaddexp(hyps[j][0], curr))
                            _bump(stats, "prefix%d" % delta)
            lst = [] if v == 0 else [[float(S["score"][b, e]), None, int(S["src"][b, e]), None] for e in range(int(S["nS"][b]))]
            ext = []
            for x in hyps:
                r = x[2] - own + b * W
                for j in range(1, k + 1):
                    tk = int(rec[r, k + j])
                    ext.append([x[0] + float(rec[r, j]), x[1] + [tk], x[2], tk])
                lst.append([x[0] + float(rec[r, 0]), x[1], x[2], None])
            assert len(lst) <= W * N
            S["nS"][b] = len(lst)
            for e, a in enumerate(lst):
                S["score"][b, e], S["src"][b, e] = a[0], a[2]
            seqs = [x[1] for x in hyps]
            left = [x for x in ext if x[1] not in seqs]           # substract
            _bump(stats, "substracted", len(ext) - len(left))
            srt = sorted(left, key=lambda x: _key(x[0]), reverse=True)
            _gaps(stats, srt, W)
            new = srt[:W]
            _bump(stats, "short_v", int(len(new) < W))
        else:
            lst = [[float(S["score"][b, e]), None, int(S["src"][b, e]), None] for e in range(int(S["nS"][b]))]
            new = [[x[0] + float(rec[x[2] - own + b * W, 0]), x[1], x[2], None] for x in hyps]
        if last:
            for a in lst:
                if a[1] is None:
                    a[1] = [int(x) for x in flat_yseq[a[2], :int(flat_ulen[a[2]]) + 1]]
            srt = sorted(lst + new, key=lambda x: _key(x[0]), reverse=True)
            _gaps(stats, srt, W)
            new = srt[:W]
            _bump(stats, "dup_kept", sum(x[1] in [y[1] for y in new[:m]] for m, x in enumerate(new)))
        st["count"][cout, b] = len(new)
        for m in range(W):
            r = b * W + m
            if m >= len(new):
                par[r] = own + m
                hidx[:, r] = [hrow(own + m, a) for a in range(LV)]
                if last:
                    for a in range(1, LV):
                        pairs[r * alpha + a - 1] = (-1, 0)
                continue
            s, y, src, tk = new[m]
            assert len(y) <= ycap, "a frame appends at most N labels"
            st["score"][cout, b, m], st["ulen"][cout, b, m] = s, len(y) - 1
            st["yseq"][cout, b, m, :len(y)] = y
            par[r] = src
            tok[r] = 0 if tk is None else tk
            live[r] = 0 if tk is None else 1
            hidx[0, r] = hrow(src, 0)
            for a in range(1, LV):
                hidx[a, r] = hrow(src, a if tk is None else a - 1)
                if last:
                    pairs[r * alpha + a - 1] = (a * R + r, y[len(y) - a]) if a <= len(y) - 1 else (-1, 0)
    return st, S, par, tok, live, hidx, pairs


def _logp(logits):
    mx = logits.max(1, keepdims=True)
    return logits - mx - np.log(np.exp(logits - mx).sum(1, keepdims=True))


def _expand(logp, k):
    """expand_rows64 of tests/alsd_restatement.py on log-probabilities"""
    order = np.argsort(-logp[:, 1:], axis=1, kind="stable")
    top = np.take_along_axis(logp[:, 1:], order, 1)
    gap = top[:, k - 1] - top[:, k] if top.shape[1] > k else np.full(len(logp), np.inf)
    return np.concatenate([logp[:, :1], top[:, :k], (order[:, :k] + 1).astype(np.float64)], 1), gap


def nsc_batch64(w, hs_pad, hlens, beam, nstep, prefix_alpha, score_norm=True, act="tanh", blank=0):
    """hs_pad [B, T, D_enc] encoder states -> dict(nbest: per utterance [(score, labels)] as BeamSearchTransducer returns them (the
    final kept sorted), min_gap over every ordering decision that is used (the top-k boundary of every live row of hyps on the calls
    v < N, the sorted extensions and sorted S + V down to position W + 1 - after prefix rescoring -, the final sort), prefix =
    [terms of depth 1, 2, 3], substracted, short_v, dup_kept, labels: those of the best hypotheses)"""
    hs_pad = np.asarray(hs_pad, np.float64)
    n, T, _ = hs_pad.shape
    N, alpha = int(nstep), int(prefix_alpha)
    V = w["lin_out_w"].shape[0]
    W = min(beam, V)
    k = min(W, V - 1)
    hl = np.full(n, T, np.int64) if hlens is None else np.clip(np.asarray(hlens, np.int64), 0, T)
    enc = (hs_pad @ w["lin_enc_w"].T + w["lin_enc_b"]).reshape(n * T, -1)
    J = enc.shape[1]
    L, H = len(w["layers"]), w["layers"][0][1].shape[1]
    R, LV = n * W, 1 + alpha
    h, c = np.zeros((L, (N + 2) * R, H)), np.zeros((L, (N + 2) * R, H))
    hs = np.zeros((N + 2, LV, R, J))
    h[:, :R], c[:, :R] = pred_step64(w, np.full(R, blank), (h[:, :R], c[:, :R]), np.ones(R, bool), blank)
    hs[0, 0] = h[-1][:R] @ w["lin_dec_w"].T
    st, S, pairs = new_state(n, W, T, N), new_s(n, W, N), new_pairs(n, W, alpha)
    pair_lp = np.zeros(len(pairs))
    stats = {}
    topk_gap = math.inf
    p = 0
    for t in range(int(hl.max()) if n else 0):
        frame = np.repeat(np.arange(n) * T + np.clip(np.minimum(t, hl - 1), 0, None), W)
        kp, ko = kept_block(N, p), kept_block(N, 1 - p)
        for v in range(1 if N == 1 else N + 1):
            last = N == 1 or v == N
            cin = kp if v == 0 else v
            if v == 0 and alpha:
                logp = _logp(act64(enc[np.tile(frame, LV)] + hs[kp].reshape(LV * R, J), act) @ w["lin_out_w"].T + w["lin_out_b"])
                for j, (row, tk) in enumerate(pairs):
                    if 0 <= row < LV * R:
                        pair_lp[j] = logp[row, tk]
                logp = logp[:R]
            else:
                logp = _logp(act64(enc[frame] + hs[cin, 0], act) @ w["lin_out_w"].T + w["lin_out_b"])
            rec, gap = _expand(logp, k)
            if v < N:
                used = ((np.arange(W)[None, :] < st["count"][cin][:, None]) & (t < hl)[:, None]).reshape(-1)
                if used.any():
                    topk_gap = min(topk_gap, float(gap[used].min()))
            st, S, par, tok, live, hidx, pairs = nsc_step64(rec, pair_lp, hl, st, S, pairs, V, T, N, alpha, t, v, p, stats)
            cout = ko if last else v + 1
            hs_rows = hs.reshape(-1, J).copy()
            hn, cn = h[:, par], c[:, par]
            if N == 1 or not last:
                hn, cn = pred_step64(w, tok, (hn, cn), live.astype(bool), blank)
                hs[cout, 0] = hn[-1] @ w["lin_dec_w"].T
            else:
                hs[cout, 0] = hs_rows[hidx[0]]
            for a in range(1, LV):
                hs[cout, a] = hs_rows[hidx[a]]
            h[:, cout * R:(cout + 1) * R], c[:, cout * R:(cout + 1) * R] = hn, cn
        p = 1 - p
    res, final_gap, labels = [], math.inf, 0
    blk = kept_block(N, p)
    for b in range(n):
        hyps = [(float(st["score"][blk, b, m]), [int(x) for x in st["yseq"][blk, b, m, :st["ulen"][blk, b, m] + 1]])
                for m in range(int(st["count"][blk, b]))]
        srt, g = nbest(hyps, score_norm)
        final_gap = min(final_gap, g)
        labels += len(srt[0][1]) - 1
        res.append(srt)
    return dict(nbest=res, min_gap=min(topk_gap, stats.get("sort_gap", math.inf), final_gap),
                prefix=[stats.get("prefix%d" % a, 0) for a in (1, 2, 3)], substracted=stats.get("substracted", 0),
                short_v=stats.get("short_v", 0), dup_kept=stats.get("dup_kept", 0), labels=labels)
