"""Support for the batched tsd transducer search tests (not collected: no test_ prefix): the time-synchronous search of
espnet_amd/nets/beam_search_transducer.py (tsd_batch; reference: espnet/nets/beam_search_transducer.py:239-347 without an LM)
restated in numpy float64 and Python lists:

  tsd_step64     one pass (frame t, symbol expansion v) of all utterances on the arrays eamd_rnnt_tsd_step reads and writes
                 (csrc/rnnt_tsd.hip);
  tsd_batch64    the whole search in the order tsd_batch runs it - prediction network and joint network of
                 tests/rnnt_greedy_restatement.py on n * W rows per pass, expand_rows64 of tests/alsd_restatement.py, tsd_step64 for
                 the bookkeeping, the n-best sort at the end - which also reports the smallest float64 gap of every ordering
                 decision that is used and counts merges, truncated A entries and emitted labels.

Hypotheses live in M + 1 blocks of n * W rows (M = max_sym_exp): block 0 and block M are the parities of B, block v (1 <= v < M) is
the C of pass v; block row = block * n * W + b * W + w.  A label sequence holds at most ycap = 1 + T (M - 1) entries: B comes from A,
A's entries are slots of the C of passes 0 .. M - 1, and the C of pass v is v labels longer than a hypothesis of the frame's B, so a
frame appends at most M - 1 labels (the expansion of pass M - 1 is never used).  tsd_step64 asserts the bound.

tests/test_tsd_restatement.py pins both to a plain per-utterance statement of the algorithm."""
import math

import numpy as np

from alsd_restatement import expand_rows64, nbest
from rnnt_greedy_restatement import act64, pred_step64


def new_state(n, W, T, M):
    """the blocks before frame 0: slot 0 of every utterance's B (parity 0 = block 0) holds [blank] with score 0"""
    st = dict(score=np.zeros((M + 1, n, W)), ulen=np.zeros((M + 1, n, W), np.int32), count=np.zeros((M + 1, n), np.int32),
              yseq=np.zeros((M + 1, n, W, 1 + T * (M - 1)), np.int32))
    st["count"][0] = 1
    return st


def new_a(n, W, M):
    return dict(score=np.zeros((n, W * M)), src=np.zeros((n, W * M), np.int32), nA=np.zeros(n, np.int32))


def b_block(M, p):
    return M if p else 0


def _key(s):
    return -math.inf if s != s else s


def _gaps(stats, name, srt, W):
    if stats is not None:
        for a, c in zip(srt[:W], srt[1:W + 1]):
            stats[name] = min(stats.get(name, math.inf), _key(a[0]) - _key(c[0]))


def tsd_step64(rec, hlens, st, A, V, T, M, t, v, p, stats=None):
    """rec [n * W, 1 + 2k] as eamd_transducer_expand_rows writes it for the rows of C, hlens [n] or None, st / A as new_state / new_a
    -> (blocks, A, par [n * W], tok, live) after the pass; st and A are not modified, and what the kernel does not write keeps the
    value it had.  stats (dict, optional) accumulates: sort_gap = the smallest difference of adjacent scores of sorted D and of
    sorted A down to position W + 1, merges, truncated (A entries dropped at a frame end)."""
    _blocks, n, W = st["score"].shape
    k = min(W, V - 1)
    R = n * W
    ycap = 1 + T * (M - 1)
    rec = np.asarray(rec).reshape(R, 1 + 2 * k)
    st = {key: x.copy() for key, x in st.items()}
    A = {key: x.copy() for key, x in A.items()}
    flat_ulen, flat_yseq = st["ulen"].reshape(-1), st["yseq"].reshape(-1, ycap)      # views: block rows
    par = np.zeros(R, np.int32)
    tok = np.zeros(R, np.int64)
    live = np.zeros(R, np.uint8)
    cin = b_block(M, p) if v == 0 else v
    cout = v + 1 if v < M - 1 else b_block(M, 1 - p)
    for b in range(n):
        Tb = T if hlens is None else max(0, min(int(hlens[b]), T))
        own = cin * R + b * W
        if t >= Tb:
            bp = b_block(M, p)
            par[b * W:(b + 1) * W] = bp * R + b * W + np.arange(W)
            if v == M - 1:
                nb = int(st["count"][bp, b])
                st["count"][cout, b] = nb
                for w in range(nb):
                    u = int(st["ulen"][bp, b, w])
                    st["score"][cout, b, w], st["ulen"][cout, b, w] = st["score"][bp, b, w], u
                    st["yseq"][cout, b, w, :u + 1] = st["yseq"][bp, b, w, :u + 1]
            continue
        # [score, labels, block row]
        C = [[float(st["score"][cin, b, w]), [int(x) for x in st["yseq"][cin, b, w, :int(st["ulen"][cin, b, w]) + 1]], own + w]
             for w in range(int(st["count"][cin, b]))]
        nA = 0 if v == 0 else int(A["nA"][b])
        lst = [[float(A["score"][b, e]), [int(x) for x in flat_yseq[A["src"][b, e], :int(flat_ulen[A["src"][b, e]]) + 1]],
                int(A["src"][b, e])] for e in range(nA)]
        seq_A = [a[1] for a in lst]                       # the reference's snapshot, taken before the loop
        for w, c in enumerate(C):
            s = c[0] + float(rec[b * W + w, 0])
            if c[1] not in seq_A:
                lst.append([s, c[1], c[2]])
            else:
                a = lst[seq_A.index(c[1])]
                a[0] = float(np.logaddexp(a[0], s))
                if stats is not None:
                    stats["merges"] = stats.get("merges", 0) + 1
        assert len(lst) <= W * M
        A["nA"][b] = len(lst)
        for e, a in enumerate(lst):
            A["score"][b, e], A["src"][b, e] = a[0], a[2]
        if v < M - 1:
            D = []
            for w, c in enumerate(C):
                for j in range(1, k + 1):
                    tk = int(rec[b * W + w, k + j])
                    D.append([c[0] + float(rec[b * W + w, j]), c[1] + [tk], c[2], tk])
            srt = sorted(D, key=lambda x: _key(x[0]), reverse=True)
            _gaps(stats, "sort_gap", srt, W)
            new = srt[:W]
        else:
            srt = sorted(lst, key=lambda x: _key(x[0]), reverse=True)
            _gaps(stats, "sort_gap", srt, W)
            if stats is not None:
                stats["truncated"] = stats.get("truncated", 0) + max(0, len(srt) - W)
            new = [a + [None] for a in srt[:W]]
        st["count"][cout, b] = len(new)
        for m in range(W):
            r = b * W + m
            if m >= len(new):
                par[r] = own + m
                continue
            s, y, src, tk = new[m]
            assert len(y) <= ycap, "a frame appends at most M - 1 labels"
            st["score"][cout, b, m], st["ulen"][cout, b, m] = s, len(y) - 1
            st["yseq"][cout, b, m, :len(y)] = y
            par[r] = src
            tok[r] = 0 if tk is None else tk
            live[r] = 0 if tk is None else 1
    return st, A, par, tok, live


def tsd_batch64(w, hs_pad, hlens, beam, max_sym_exp, score_norm=True, act="tanh", blank=0):
    """hs_pad [B, T, D_enc] encoder states -> dict(nbest: per utterance [(score, labels)] as BeamSearchTransducer returns them (the
    final B sorted), min_gap over every ordering decision that is used (the top-k boundary of every live row of C on the passes
    v < M - 1, sorted D and sorted A down to position W + 1, the final sort), merges, truncated, labels: those of the best
    hypotheses)"""
    hs_pad = np.asarray(hs_pad, np.float64)
    n, T, _ = hs_pad.shape
    M = int(max_sym_exp)
    V = w["lin_out_w"].shape[0]
    W = min(beam, V)
    k = min(W, V - 1)
    hl = np.full(n, T, np.int64) if hlens is None else np.clip(np.asarray(hlens, np.int64), 0, T)
    enc = (hs_pad @ w["lin_enc_w"].T + w["lin_enc_b"]).reshape(n * T, -1)
    L, H = len(w["layers"]), w["layers"][0][1].shape[1]
    R = n * W
    h, c = np.zeros((L, (M + 1) * R, H)), np.zeros((L, (M + 1) * R, H))
    h[:, :R], c[:, :R] = pred_step64(w, np.full(R, blank), (h[:, :R], c[:, :R]), np.ones(R, bool), blank)
    st, A = new_state(n, W, T, M), new_a(n, W, M)
    stats = {}
    topk_gap = math.inf
    p = 0
    for t in range(int(hl.max())):
        frame = np.repeat(np.arange(n) * T + np.clip(np.minimum(t, hl - 1), 0, None), W)
        for v in range(M):
            cin = b_block(M, p) if v == 0 else v
            cout = v + 1 if v < M - 1 else b_block(M, 1 - p)
            d = h[-1][cin * R:(cin + 1) * R] @ w["lin_dec_w"].T
            logits = act64(enc[frame] + d, act) @ w["lin_out_w"].T + w["lin_out_b"]
            rec, gap = expand_rows64(logits, k)
            if v < M - 1:
                used = ((np.arange(W)[None, :] < st["count"][cin][:, None]) & (t < hl)[:, None]).reshape(-1)
                if used.any():
                    topk_gap = min(topk_gap, float(gap[used].min()))
            st, A, par, tok, live = tsd_step64(rec, hl, st, A, V, T, M, t, v, p, stats)
            hn, cn = h[:, par], c[:, par]
            if v < M - 1:
                hn, cn = pred_step64(w, tok, (hn, cn), live.astype(bool), blank)
            h[:, cout * R:(cout + 1) * R], c[:, cout * R:(cout + 1) * R] = hn, cn
        p = 1 - p
    res, final_gap, labels = [], math.inf, 0
    blk = b_block(M, p)
    for b in range(n):
        hyps = [(float(st["score"][blk, b, m]), [int(x) for x in st["yseq"][blk, b, m, :st["ulen"][blk, b, m] + 1]])
                for m in range(int(st["count"][blk, b]))]
        srt, g = nbest(hyps, score_norm)
        final_gap = min(final_gap, g)
        labels += len(srt[0][1]) - 1
        res.append(srt)
    return dict(nbest=res, min_gap=min(topk_gap, stats.get("sort_gap", math.inf), final_gap), merges=stats.get("merges", 0),
                truncated=stats.get("truncated", 0), labels=labels)
