"""Support for the batched default transducer search tests (not collected: no test_ prefix): the default (Graves A / B) beam
search of espnet_amd/nets/beam_search_transducer.py (default_batch; reference: espnet/nets/beam_search_transducer.py:163-237 without
an LM) restated in numpy float64 and Python lists:

  plain_default     the reference's loop on one utterance, A and B as unpruned Python lists, the joint rows from a callback;
  default_step64    one step (finish the pending pop, end the frame, select the next pop) of all utterances on the arrays
                    eamd_rnnt_default_step reads and writes (csrc/rnnt_default.hip);
  default_batch64   the whole search in the order default_batch runs it - prediction network and joint network of
                    tests/rnnt_greedy_restatement.py on n rows, the state pool with its two frame-parity regions, default_step64
                    for the bookkeeping, the n-best sort at the end - which also reports the smallest float64 gap of every ordering
                    decision it took, the pops of every frame and the duplicates that stay (there is no recombination).

tests/test_default_restatement.py pins default_step64 and default_batch64 to plain_default."""
import math

import numpy as np

from alsd_restatement import expand_rows64
from rnnt_greedy_restatement import act64, pred_step64

C_T, C_POPS, C_NA, C_NB, C_NLOG, C_SEQ, C_CUR, C_MAXPOPS = range(8)      # columns of ctr
_A, _B = ("a_score", "a_seq", "a_row", "a_log", "a_tok"), ("b_score", "b_row", "b_log")
STATE = _A + _B + ("cur", "ctr", "log", "flags")
OUT = ("par", "tok", "dst", "live", "frame", "alive")


def _key(s):
    return -math.inf if s != s else s


def plain_default(row_fn, T, W, k, score_norm=True):
    """row_fn(t, labels) -> (blank logp, [(logp, token)] * k in top-k order).  -> (n-best [(score, labels)], pops per frame)"""
    B = [(0.0, [0])]
    pops = []
    for t in range(T):
        A, B = B, []
        count = 0
        while True:
            j = max(range(len(A)), key=lambda i: A[i][0])          # the first maximum in list order
            s, y = A.pop(j)
            blank_lp, ext = row_fn(t, y)
            for lp, tok in ext[:k]:
                A.append((s + float(lp), y + [int(tok)]))
            B.append((s + float(blank_lp), y))
            count += 1
            bound = max(a[0] for a in A)
            ahead = sorted((c for c in B if c[0] > bound), key=lambda c: c[0])
            if len(ahead) >= W:
                B = ahead
                break
        pops.append(count)
    key = (lambda x: x[0] / len(x[1])) if score_norm else (lambda x: x[0])
    return sorted(B, key=key, reverse=True), pops


def new_state(n, P, log_cap, hlens, T):
    """the state before the first step and what the first step's launches read: A = [(0.0, [blank])] has been popped already - record
    0, its state in row 0 of the odd region -; an utterance without frames is done with B = [(0.0, [blank])]"""
    hl = np.full(n, T, np.int64) if hlens is None else np.clip(np.asarray(hlens, np.int64), 0, T)
    run = hl > 0
    st = {key: np.zeros((n, P), np.float64 if key.endswith("score") else np.int32) for key in _A + _B}
    st.update(cur=np.zeros(n), ctr=np.zeros((n, 8), np.int32), log=np.zeros((n, log_cap, 2), np.int32), flags=np.zeros((2, n), np.int32))
    st["flags"][0] = ~run
    st["ctr"][:, C_POPS] = run
    st["ctr"][:, C_NB] = ~run
    st["ctr"][:, C_NLOG] = 1
    st["log"][:, 0, 0] = -1
    rows = np.arange(n)
    out = dict(par=(rows * 2 * P + P).astype(np.int32), tok=np.zeros(n, np.int64), dst=(rows * 2 * P).astype(np.int32),
               live=np.zeros(n, np.uint8), frame=(rows * T).astype(np.int32), alive=run.astype(np.uint8))
    return st, out


def labels_of(log_b, rec, blank=0):
    """the labels of record `rec` of one utterance's log [log_cap, 2]"""
    out = []
    while rec > 0:
        if log_b[rec, 1]:
            out.append(int(log_b[rec, 1]))
        rec = int(log_b[rec, 0])
    return [blank] + out[::-1]


def final_b(st, b):
    """[(score, labels)] of B, in its order"""
    return [(float(st["b_score"][b, j]), labels_of(st["log"][b], int(st["b_log"][b, j]))) for j in range(int(st["ctr"][b, C_NB]))]


def nbest(hyps, score_norm):
    """[(score, labels)] -> sorted as the reference sorts the last B; smallest adjacent key difference"""
    key = (lambda x: x[0] / len(x[1])) if score_norm else (lambda x: x[0])
    srt = sorted(hyps, key=key, reverse=True)
    gap = min((key(a) - key(c) for a, c in zip(srt, srt[1:])), default=math.inf)
    return srt, gap


def default_step64(rec, hlens, st, W, V, T, stats=None):
    """rec [n, 1 + 2k] as eamd_transducer_expand_rows writes it for the pending pops, hlens [n] or None, st as new_state
    -> (state after the step, dict(par, tok, dst, live, frame, alive)); st is not modified.
    stats (dict, optional) accumulates: gap = the smallest distance of an ordering decision (A[0] against A[1] when A[0] is popped,
    every score of B against bound, adjacent scores of ahead), pops = per utterance the pops of every finished frame, long_ahead =
    frames that end with more than W entries, cut = entries of A dropped by the cut at P."""
    n, P = st["a_score"].shape
    k = min(W, V - 1)
    log_cap = st["log"].shape[1]
    rec = np.asarray(rec).reshape(n, 1 + 2 * k)
    st = {key: v.copy() for key, v in st.items()}
    ctr, flags = st["ctr"], st["flags"]
    out = dict(par=np.zeros(n, np.int32), tok=np.zeros(n, np.int64), dst=np.zeros(n, np.int32), live=np.zeros(n, np.uint8),
               frame=np.zeros(n, np.int32), alive=np.zeros(n, np.uint8))

    def gap(v):
        if stats is not None and v == v:
            stats["gap"] = min(stats.get("gap", math.inf), abs(v))

    for b in range(n):
        Tb = T if hlens is None else min(max(int(hlens[b]), 0), T)
        base = b * 2 * P
        out["par"][b], out["dst"][b], out["frame"][b] = base, base, b * T
        if flags[0, b] or flags[1, b]:
            continue
        t, pops, nA, nB, nlog, seqc, cur = (int(ctr[b, c]) for c in (C_T, C_POPS, C_NA, C_NB, C_NLOG, C_SEQ, C_CUR))
        cur_row = (t & 1) * P + pops - 1
        s = float(st["cur"][b])
        A = [tuple(st[key][b, x].item() for key in _A) for x in range(nA)]
        B = [tuple(st[key][b, x].item() for key in _B) for x in range(nB)]
        # finish the pop
        for j in range(k):
            A.append((s + float(rec[b, 1 + j]), seqc + j, cur_row, cur, int(rec[b, 1 + k + j])))
        B.append((s + float(rec[b, 0]), cur_row, cur))
        for key, v in zip(_B, B[-1]):
            st[key][b, nB] = v
        nB += 1
        A.sort(key=lambda e: (-_key(e[0]), e[1]))
        bound = _key(A[0][0])
        ahead = [x for x in range(nB) if _key(B[x][0]) > bound]
        for x in range(nB):
            gap(_key(B[x][0]) - bound)
        turn = len(ahead) >= W
        t1 = t + 1 if turn else t
        if turn:
            order = sorted(ahead, key=lambda x: _key(B[x][0]))             # stable, ascending
            for x, y in zip(order, order[1:]):
                gap(_key(B[y][0]) - _key(B[x][0]))
            if stats is not None:
                stats.setdefault("pops", {}).setdefault(b, []).append(pops)
                stats["long_ahead"] = stats.get("long_ahead", 0) + (len(ahead) > W)
            ctr[b, C_MAXPOPS] = max(int(ctr[b, C_MAXPOPS]), pops)
            if t1 >= Tb:                                                   # after the last frame: B = ahead, done
                for rank, x in enumerate(order):
                    for key, v in zip(_B, B[x]):
                        st[key][b, rank] = v
                ctr[b, C_T], ctr[b, C_POPS], ctr[b, C_NA], ctr[b, C_NB], ctr[b, C_SEQ] = t1, 0, 0, len(order), len(order)
                flags[0, b] = 1
                continue
            A = sorted(((B[x][0], rank, B[x][1], B[x][2], 0) for rank, x in enumerate(order)), key=lambda e: (-_key(e[0]), e[1]))
            pops0, nB, seqn = 0, 0, len(order)
        else:
            if stats is not None:
                stats["cut"] = stats.get("cut", 0) + max(0, len(A) - P)
            A = A[:P]
            pops0, seqn = pops, seqc + k
        pop = pops0 < P and nlog < log_cap
        if pop:
            if len(A) > 1:
                gap(_key(A[0][0]) - _key(A[1][0]))
            (p_score, _seq, p_row, p_log, p_tok), A = A[0], A[1:]
        for x, e in enumerate(A):
            for key, v in zip(_A, e):
                st[key][b, x] = v
        ctr[b, C_T], ctr[b, C_NA], ctr[b, C_NB], ctr[b, C_SEQ] = t1, len(A), nB, seqn
        if pop:
            ctr[b, C_POPS], ctr[b, C_NLOG], ctr[b, C_CUR] = pops0 + 1, nlog + 1, nlog
            st["log"][b, nlog] = (p_log, p_tok)
            st["cur"][b] = p_score
            out["par"][b], out["tok"][b], out["dst"][b] = base + p_row, p_tok, base + (t1 & 1) * P + pops0
            out["live"][b], out["frame"][b], out["alive"][b] = p_tok != 0, b * T + t1, 1
        else:
            ctr[b, C_POPS] = pops0
            flags[1, b] = 1
    return st, out


def default_batch64(w, hs_pad, hlens, beam, P=256, score_norm=True, max_steps=None, act="tanh", blank=0):
    """hs_pad [B, T, D_enc] encoder states -> dict(nbest: per utterance [(score, labels)] as BeamSearchTransducer returns them, None
    for an utterance that overflowed or was cut off at max_steps; min_gap over every ordering decision (top-k boundary of every
    pending row, default_step64's gaps, the final sort); pops: per utterance the pops of every frame; total: per utterance the pops
    selected; overflow: per utterance; dups: equal label sequences that stayed side by side in a frame's final B; long_ahead; cut)"""
    hs_pad = np.asarray(hs_pad, np.float64)
    n, T, _ = hs_pad.shape
    V = w["lin_out_w"].shape[0]
    W = min(beam, V)
    k = min(W, V - 1)
    hl = np.full(n, T, np.int64) if hlens is None else np.clip(np.asarray(hlens, np.int64), 0, T)
    enc = (hs_pad @ w["lin_enc_w"].T + w["lin_enc_b"]).reshape(n * T, -1)
    L, H = len(w["layers"]), w["layers"][0][1].shape[1]
    if max_steps is None:
        max_steps = 64 * W * int(hl.max())
    st, out = new_state(n, P, max_steps + 1, hl, T)
    pool = [np.zeros((L, n * 2 * P, H)), np.zeros((L, n * 2 * P, H))]
    first = pred_step64(w, np.full(n, blank), (np.zeros((L, n, H)), np.zeros((L, n, H))), np.ones(n, bool), blank)
    pool[0][:, out["par"]], pool[1][:, out["par"]] = first
    stats = {}
    topk_gap, dups, steps = math.inf, 0, 0
    while steps < max_steps and not (st["flags"][0] | st["flags"][1]).all():
        state = pred_step64(w, out["tok"], (pool[0][:, out["par"]], pool[1][:, out["par"]]), out["live"].astype(bool), blank)
        on = out["alive"].astype(bool)
        pool[0][:, out["dst"][on]], pool[1][:, out["dst"][on]] = state[0][:, on], state[1][:, on]
        d = state[0][-1] @ w["lin_dec_w"].T
        logits = act64(enc[out["frame"]] + d, act) @ w["lin_out_w"].T + w["lin_out_b"]
        rec, gap = expand_rows64(logits, k)
        if on.any():
            topk_gap = min(topk_gap, float(gap[on].min()))
        before = st["ctr"][:, C_T].copy()
        st, out = default_step64(rec, hl, st, W, V, T, stats)
        steps += 1
        for b in np.nonzero(st["ctr"][:, C_T] != before)[0]:             # a frame ended: what it hands on, duplicates included
            if st["flags"][0, b]:
                seqs = [tuple(y) for _s, y in final_b(st, b)]
            else:
                recs = [int(st["a_log"][b, x]) for x in range(int(st["ctr"][b, C_NA]))] + [int(st["log"][b, st["ctr"][b, C_CUR], 0])]
                seqs = [tuple(labels_of(st["log"][b], r)) for r in recs]
            dups += len(seqs) - len(set(seqs))
    res, final_gap = [], math.inf
    for b in range(n):
        if st["flags"][1, b] or not st["flags"][0, b]:
            res.append(None)
            continue
        srt, g = nbest(final_b(st, b), score_norm)
        final_gap = min(final_gap, g)
        res.append(srt)
    return dict(nbest=res, min_gap=min(topk_gap, stats.get("gap", math.inf), final_gap),
                pops=[stats.get("pops", {}).get(b, []) for b in range(n)], total=[int(v) for v in st["ctr"][:, C_NLOG] * (hl > 0)],
                overflow=[bool(st["flags"][1, b] or not st["flags"][0, b]) for b in range(n)], dups=dups,
                long_ahead=stats.get("long_ahead", 0), cut=stats.get("cut", 0), steps=steps)
