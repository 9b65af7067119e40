"""Support for the tests of RNN LM shallow fusion in the batched alsd / tsd transducer searches (not collected: no test_ prefix).

With an LM the reference's extension score is `s = score + lp; s += lm_weight * torch.tensor(q, dtype=float32)`: from the first label
on a score is a float32 0-d tensor and every later sum, and np.logaddexp of a merge, runs in float32; only [blank] (u == 0 labels)
and its chain of blank continuations stay Python doubles.  The device loops store scores as doubles that hold float32 values
(csrc/rnnt_search.h: rs_add / rs_ext / rs_merge).  Restated here with np.float32 arithmetic:

  lm_add / lm_ext / lm_merge   the scalar rule;
  alsd_lm_step, tsd_lm_step    one step / pass of all utterances on the arrays eamd_rnnt_alsd_step_lm / eamd_rnnt_tsd_step_lm read and
                               write, the record [n * W, 1 + 3k] as eamd_transducer_expand_rows writes it with an LM; they also say
                               which scores a merge touched (the GPU test holds the others to bit equality);
  alsd_lm_batch, tsd_lm_batch  the whole searches in the order alsd_batch / tsd_batch run them with an LM - prediction network, LM
                               (the same cell stack: pred_step64 of tests/rnnt_greedy_restatement.py) and joint network in float64
                               on n * W rows, the record rounded to float32 as the kernel reads it, the n-best sort with its
                               float32 division - with the smallest gap of every ordering decision.

tests/test_rnnt_lm_restatement.py pins the scalar rule to torch's arithmetic bit for bit and the searches to a per-utterance loop
over hypothesis objects."""
import math

import numpy as np

from alsd_restatement import expand_rows64, new_finals, new_state
from rnnt_greedy_restatement import act64, pred_step64
from tsd_restatement import b_block, new_a
from tsd_restatement import new_state as tsd_new_state

f32 = np.float32


# ---- the scalar rule ------------------------------------------------------------------------------------------------------------
def lm_add(S, u, lp):
    """parent score S (a double; with u > 0 labels it holds a float32 value) + a joint log-probability lp (float32)"""
    if u == 0:
        return float(S) + float(f32(lp))
    return float(f32(S) + f32(lp))


def lm_ext(S, u, lp, q, w):
    """an extension: lm_add, then + (float)w * q with the product rounded to float32 before the sum"""
    m = f32(w) * f32(q)                          # one float32 multiply
    return float(f32(lm_add(S, u, lp)) + m)


def lm_merge(a, b, u):
    """the score of two equal label sequences of u labels: numpy's float32 logaddexp, the double one for [blank]"""
    if u == 0:
        return float(np.logaddexp(float(a), float(b)))
    return float(np.logaddexp(f32(a), f32(b)))


def lm_key(score, length, score_norm):
    """the n-best sort's key: score / len(yseq) divides in float32 for a hypothesis with labels"""
    if not score_norm:
        return score
    return score / length if length <= 1 else float(f32(score) / f32(length))


def _key(s):
    return -math.inf if s != s else s


def _gaps(stats, srt, W):
    if stats is not None:
        for a, c in zip(srt[:W], srt[1:W + 1]):
            stats["sort_gap"] = min(stats.get("sort_gap", math.inf), _key(a[0]) - _key(c[0]))


def _count(stats, name, by=1):
    if stats is not None:
        stats[name] = stats.get(name, 0) + by


# ---- alsd: one step -------------------------------------------------------------------------------------------------------------
def alsd_lm_step(rec, hlens, st, fin, V, T, u_max, i, w, stats=None):
    """rec [n * W, 1 + 3k] float32 (blank, k log-probabilities, k tokens, k raw LM log-probabilities), hlens [n] or None, st / fin as
    alsd_restatement.new_state / new_finals, w = lm_weight -> (state of the other parity, finals, par [n * W], tok, live, frame,
    active [n, W], merged = dict(score [n, W], fin [n, fcap]): the scores a recombination produced); st and fin are not modified"""
    n, W = st["score"].shape
    k = min(W, V - 1)
    rec = np.asarray(rec, f32).reshape(n * W, 1 + 3 * k)
    out = dict(score=np.zeros((n, W)), ulen=np.zeros((n, W), np.int32), nhyp=np.zeros(n, np.int32), yseq=np.zeros_like(st["yseq"]))
    fin = {key: v.copy() for key, v in fin.items()}
    merged = dict(score=np.zeros((n, W), bool), fin=np.zeros(fin["score"].shape, bool))
    par = np.arange(n * W, dtype=np.int32)
    tok = np.zeros(n * W, np.int64)
    live = np.zeros(n * W, np.uint8)
    frame = np.zeros(n * W, np.int32)
    active = np.zeros((n, W), bool)
    for b in range(n):
        Tb = T if hlens is None else min(int(hlens[b]), T)
        umb = min(u_max, Tb - 1)
        nh = int(st["nhyp"][b])
        # [score, labels, parent slot, appended token or None, grown by a merge]
        B = [[float(st["score"][b, s]), [int(v) for v in st["yseq"][b, s, :int(st["ulen"][b, s]) + 1]], s, None, False]
             for s in range(nh)]
        act = [] if i >= Tb + umb else [s for s in range(nh) if i - (len(B[s][1]) - 1) + 1 <= Tb - 1]
        active[b, act] = True
        if act:
            A, final = [], []
            for s in act:
                S, y = B[s][0], B[s][1]
                u, r = len(y) - 1, b * W + s
                nb = [lm_add(S, u, rec[r, 0]), y, s, None, False]
                A.append(nb)
                if i - u + 1 == Tb - 1:
                    final.append(nb)
                for j in range(1, k + 1):
                    t = int(rec[r, k + j])
                    A.append([lm_ext(S, u, rec[r, j], rec[r, 2 * k + j], w), y + [t], s, t, False])
            srt = sorted(A, key=lambda x: _key(x[0]), reverse=True)
            _count(stats, "dropped", nh - len(act))
            _gaps(stats, srt, W)
            B = srt[:W]
            seen = []
            for h in B:
                for f in seen:
                    if f[1] == h[1]:
                        f[0] = lm_merge(f[0], h[0], len(h[1]) - 1)
                        f[4] = True
                        _count(stats, "merges")
                        _count(stats, "merges32", int(len(h[1]) > 1))
                        break
                else:
                    seen.append(h)
            for h in final:                       # the objects of A: a selected first occurrence carries its recombined score
                q = int(fin["nfin"][b])
                fin["score"][b, q] = h[0]
                fin["len"][b, q] = len(h[1])
                fin["yseq"][b, q, :len(h[1])] = h[1]
                merged["fin"][b, q] = h[4]
                fin["nfin"][b] = q + 1
        out["nhyp"][b] = len(B)
        for m, h in enumerate(B):
            r = b * W + m
            out["score"][b, m] = h[0]
            out["ulen"][b, m] = len(h[1]) - 1
            out["yseq"][b, m, :len(h[1])] = h[1]
            merged["score"][b, m] = h[4]
            if act:
                par[r] = b * W + h[2]
                tok[r] = 0 if h[3] is None else h[3]
                live[r] = 0 if h[3] is None else 1
        for m in range(W):
            u = int(out["ulen"][b, m])
            frame[b * W + m] = b * T + min(max(i + 1 - u + 1, 0), max(Tb - 1, 0))
    return out, fin, par, tok, live, frame, active, merged


# ---- tsd: one pass --------------------------------------------------------------------------------------------------------------
def tsd_lm_step(rec, hlens, st, A, V, T, M, t, v, p, w, stats=None):
    """rec [n * W, 1 + 3k] float32 of the rows of C, hlens [n] or None, st / A as tsd_restatement.new_state / new_a, w = lm_weight
    -> (blocks, A, par [n * W], tok, live, merged = dict(a [n, W M], score [n, W]): the entries of A a merge of this pass grew, the
    slots of the block this pass wrote that hold such a score); st and A are not modified, and what the kernel does not write keeps
    the value it had"""
    _blocks, n, W = st["score"].shape
    k = min(W, V - 1)
    R = n * W
    ycap = 1 + T * (M - 1)
    rec = np.asarray(rec, f32).reshape(R, 1 + 3 * k)
    st = {key: x.copy() for key, x in st.items()}
    A = {key: x.copy() for key, x in A.items()}
    merged = dict(a=np.zeros(A["score"].shape, bool), score=np.zeros((n, W), bool))
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
                for s in range(nb):
                    u = int(st["ulen"][bp, b, s])
                    st["score"][cout, b, s], st["ulen"][cout, b, s] = st["score"][bp, b, s], u
                    st["yseq"][cout, b, s, :u + 1] = st["yseq"][bp, b, s, :u + 1]
            continue
        # [score, labels, block row, grown by a merge of this pass]
        C = [[float(st["score"][cin, b, s]), [int(x) for x in st["yseq"][cin, b, s, :int(st["ulen"][cin, b, s]) + 1]], own + s]
             for s in range(int(st["count"][cin, b]))]
        nA = 0 if v == 0 else int(A["nA"][b])
        lst = [[float(A["score"][b, e]), [int(x) for x in flat_yseq[A["src"][b, e], :int(flat_ulen[A["src"][b, e]]) + 1]],
                int(A["src"][b, e]), False] for e in range(nA)]
        seq_A = [a[1] for a in lst]                       # the reference's snapshot, taken before the loop
        for s, c in enumerate(C):
            u = len(c[1]) - 1
            sc = lm_add(c[0], u, rec[b * W + s, 0])
            if c[1] not in seq_A:
                lst.append([sc, c[1], c[2], False])
            else:
                a = lst[seq_A.index(c[1])]
                a[0] = lm_merge(a[0], sc, u)
                a[3] = True
                _count(stats, "merges")
                _count(stats, "merges32", int(u > 0))
        assert len(lst) <= W * M
        A["nA"][b] = len(lst)
        for e, a in enumerate(lst):
            A["score"][b, e], A["src"][b, e] = a[0], a[2]
            merged["a"][b, e] = a[3]
        if v < M - 1:
            D = []
            for s, c in enumerate(C):
                for j in range(1, k + 1):
                    tk = int(rec[b * W + s, k + j])
                    D.append([lm_ext(c[0], len(c[1]) - 1, rec[b * W + s, j], rec[b * W + s, 2 * k + j], w), c[1] + [tk], c[2], False,
                              tk])
            srt = sorted(D, key=lambda x: _key(x[0]), reverse=True)
            _gaps(stats, srt, W)
            new = srt[:W]
        else:
            srt = sorted(lst, key=lambda x: _key(x[0]), reverse=True)
            _gaps(stats, srt, W)
            _count(stats, "truncated", max(0, len(srt) - W))
            new = [a + [None] for a in srt[:W]]
        st["count"][cout, b] = len(new)
        for m in range(W):
            r = b * W + m
            if m >= len(new):
                par[r] = own + m
                continue
            s, y, src, grown, tk = new[m]
            assert len(y) <= ycap, "a frame appends at most M - 1 labels"
            st["score"][cout, b, m], st["ulen"][cout, b, m] = s, len(y) - 1
            st["yseq"][cout, b, m, :len(y)] = y
            merged["score"][b, m] = grown
            par[r] = src
            tok[r] = 0 if tk is None else tk
            live[r] = 0 if tk is None else 1
    return st, A, par, tok, live, merged


# ---- the whole searches ---------------------------------------------------------------------------------------------------------
def lm_weights_from_state_dict(sd, prefix="lm."):
    """{name: array} of a ClassifierWithState(RNNLM) state dict -> the cell stack in pred_step64's form, plus the output layer"""
    g = lambda k: np.asarray(sd[prefix + k], np.float64)      # noqa: E731
    layers = []
    while prefix + "predictor.rnn.%d.weight_ih" % len(layers) in sd:
        i = len(layers)
        layers.append(tuple(g("predictor.rnn.%d.%s" % (i, k)) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
    gates = layers[0][0].shape[0] // layers[0][1].shape[1]
    return dict(embed=g("predictor.embed.weight"), layers=layers, dtype="lstm" if gates == 4 else "gru",
                lo_w=g("predictor.lo.weight"), lo_b=g("predictor.lo.bias"))


def seeded_lm(seed, typ, L, H, V, sharp=1.5):
    """float32 weights of a ClassifierWithState(RNNLM) as a state dict of numpy arrays (prefix "lm."), scaled so that its
    log-probabilities spread over a few units: the LM term then changes selections"""
    r = np.random.default_rng(seed)
    G = 4 if typ == "lstm" else 3
    f = lambda *s, scale=1.0: (r.standard_normal(s) * scale).astype(np.float32)      # noqa: E731
    sd = {"lm.predictor.embed.weight": f(V, H)}
    for l in range(L):
        sd["lm.predictor.rnn.%d.weight_ih" % l] = f(G * H, H, scale=1.0 / np.sqrt(H))
        sd["lm.predictor.rnn.%d.weight_hh" % l] = f(G * H, H, scale=1.0 / np.sqrt(H))
        sd["lm.predictor.rnn.%d.bias_ih" % l] = f(G * H, scale=0.1)
        sd["lm.predictor.rnn.%d.bias_hh" % l] = f(G * H, scale=0.1)
    sd["lm.predictor.lo.weight"] = f(V, H, scale=sharp / np.sqrt(H) * 4.0)
    sd["lm.predictor.lo.bias"] = f(V, scale=0.5)
    return sd


def log_softmax64(z):
    mx = z.max(1, keepdims=True)
    return z - mx - np.log(np.exp(z - mx).sum(1, keepdims=True))


def lm_rows64(lmw, h_top):
    """the LM's log-probabilities of the next token from the top layer's h [R, H]"""
    return log_softmax64(h_top @ lmw["lo_w"].T + lmw["lo_b"])


def expand_rows_lm(logits, k, lm_logp):
    """float64 logits [n, V], LM log-probabilities [n, V] -> (rec [n, 1 + 3k] float32 as the kernel writes it, top-k gap [n] in
    float64)"""
    rec, gap = expand_rows64(logits, k)
    toks = rec[:, 1 + k:].astype(np.int64)
    return np.concatenate([rec, np.take_along_axis(lm_logp, toks, 1)], 1).astype(f32), gap


def nbest_lm(hyps, score_norm):
    """[(score, labels)] -> sorted as the per-utterance search sorts them; smallest adjacent key difference"""
    key = lambda x: lm_key(x[0], len(x[1]), score_norm)      # noqa: E731
    srt = sorted(hyps, key=key, reverse=True)
    gap = min((key(a) - key(c) for a, c in zip(srt, srt[1:])), default=math.inf)
    return srt, gap


def _zero_state(net, R):
    L, H = len(net["layers"]), net["layers"][0][1].shape[1]
    return np.zeros((L, R, H)), np.zeros((L, R, H))


def alsd_lm_batch(w, lmw, hs_pad, hlens, beam, u_max, lm_weight, score_norm=True, act="tanh", blank=0):
    """hs_pad [B, T, D_enc] encoder states -> dict(nbest: per utterance [(score, labels)] as alsd_batch returns them with an LM,
    min_gap over every ordering decision (top-k boundary of every active row in float64, sorted A down to position W + 1, the final
    sort's keys), merges, merges32 (those in float32), finals, dropped, no_final)"""
    hs_pad = np.asarray(hs_pad, np.float64)
    n, T, _ = hs_pad.shape
    V = w["lin_out_w"].shape[0]
    W = min(beam, V)
    k = min(W, V - 1)
    hl = np.full(n, T, np.int64) if hlens is None else np.minimum(np.asarray(hlens, np.int64), T)
    enc = (hs_pad @ w["lin_enc_w"].T + w["lin_enc_b"]).reshape(n * T, -1)
    R = n * W
    every = np.ones(R, bool)
    state = pred_step64(w, np.full(R, blank), _zero_state(w, R), every, blank)
    lstate = pred_step64(lmw, np.full(R, blank), _zero_state(lmw, R), every, blank)
    st, fin = new_state(n, W, T, u_max), new_finals(n, W, u_max)
    frame = np.repeat(np.arange(n) * T + np.clip(hl - 1, 0, 1), W)
    stats = {}
    topk_gap = math.inf
    steps = int(max(int(t) + min(u_max, int(t) - 1) for t in hl))
    for i in range(steps):
        d = state[0][-1] @ w["lin_dec_w"].T
        logits = act64(enc[frame] + d, act) @ w["lin_out_w"].T + w["lin_out_b"]
        rec, gap = expand_rows_lm(logits, k, lm_rows64(lmw, lstate[0][-1]))
        st, fin, par, tok, live, frame, active, _m = alsd_lm_step(rec, hl, st, fin, V, T, u_max, i, lm_weight, stats)
        if active.any():
            topk_gap = min(topk_gap, float(gap[active.reshape(-1)].min()))
        on = live.astype(bool)
        state = pred_step64(w, tok, (state[0][:, par], state[1][:, par]), on, blank)
        lstate = pred_step64(lmw, tok, (lstate[0][:, par], lstate[1][:, par]), on, blank)
    res, final_gap, no_final = [], math.inf, 0
    for b in range(n):
        q = int(fin["nfin"][b])
        if q:
            srt, g = nbest_lm([(float(fin["score"][b, j]), [int(v) for v in fin["yseq"][b, j, :fin["len"][b, j]]]) for j in range(q)],
                              score_norm)
            final_gap = min(final_gap, g)
            res.append(srt)
        else:
            no_final += 1
            res.append([(float(st["score"][b, m]), [int(v) for v in st["yseq"][b, m, :st["ulen"][b, m] + 1]])
                        for m in range(int(st["nhyp"][b]))])
    return dict(nbest=res, min_gap=min(topk_gap, stats.get("sort_gap", math.inf), final_gap), merges=stats.get("merges", 0),
                merges32=stats.get("merges32", 0), finals=int(fin["nfin"].sum()), dropped=stats.get("dropped", 0), no_final=no_final)


def tsd_lm_batch(w, lmw, hs_pad, hlens, beam, max_sym_exp, lm_weight, score_norm=True, act="tanh", blank=0):
    """hs_pad [B, T, D_enc] encoder states -> dict(nbest: per utterance [(score, labels)] as tsd_batch returns them with an LM (the
    final B sorted), min_gap over every ordering decision that is used (the top-k boundary of every live row of C on the passes
    v < M - 1, sorted D and sorted A down to position W + 1, the final sort's keys), merges, merges32, truncated, labels)"""
    hs_pad = np.asarray(hs_pad, np.float64)
    n, T, _ = hs_pad.shape
    M = int(max_sym_exp)
    V = w["lin_out_w"].shape[0]
    W = min(beam, V)
    k = min(W, V - 1)
    hl = np.full(n, T, np.int64) if hlens is None else np.clip(np.asarray(hlens, np.int64), 0, T)
    enc = (hs_pad @ w["lin_enc_w"].T + w["lin_enc_b"]).reshape(n * T, -1)
    R = n * W
    every = np.ones(R, bool)
    nets = []                                              # per network: weights, h and c of the M + 1 blocks
    for net in (w, lmw):
        z = _zero_state(net, (M + 1) * R)
        h, c = z[0].copy(), z[1].copy()
        h[:, :R], c[:, :R] = pred_step64(net, np.full(R, blank), (h[:, :R], c[:, :R]), every, blank)
        nets.append((net, h, c))
    st, A = tsd_new_state(n, W, T, M), new_a(n, W, M)
    stats = {}
    topk_gap = math.inf
    p = 0
    for t in range(int(hl.max())):
        frame = np.repeat(np.arange(n) * T + np.clip(np.minimum(t, hl - 1), 0, None), W)
        for v in range(M):
            cin = b_block(M, p) if v == 0 else v
            cout = v + 1 if v < M - 1 else b_block(M, 1 - p)
            d = nets[0][1][-1][cin * R:(cin + 1) * R] @ w["lin_dec_w"].T
            logits = act64(enc[frame] + d, act) @ w["lin_out_w"].T + w["lin_out_b"]
            rec, gap = expand_rows_lm(logits, k, lm_rows64(lmw, nets[1][1][-1][cin * R:(cin + 1) * R]))
            if v < M - 1:
                used = ((np.arange(W)[None, :] < st["count"][cin][:, None]) & (t < hl)[:, None]).reshape(-1)
                if used.any():
                    topk_gap = min(topk_gap, float(gap[used].min()))
            st, A, par, tok, live, _m = tsd_lm_step(rec, hl, st, A, V, T, M, t, v, p, lm_weight, stats)
            for net, h, c in nets:
                hn, cn = h[:, par], c[:, par]
                if v < M - 1:
                    hn, cn = pred_step64(net, tok, (hn, cn), live.astype(bool), blank)
                h[:, cout * R:(cout + 1) * R], c[:, cout * R:(cout + 1) * R] = hn, cn
        p = 1 - p
    res, final_gap, labels = [], math.inf, 0
    blk = b_block(M, p)
    for b in range(n):
        hyps = [(float(st["score"][blk, b, m]), [int(x) for x in st["yseq"][blk, b, m, :st["ulen"][blk, b, m] + 1]])
                for m in range(int(st["count"][blk, b]))]
        srt, g = nbest_lm(hyps, score_norm)
        final_gap = min(final_gap, g)
        labels += len(srt[0][1]) - 1
        res.append(srt)
    return dict(nbest=res, min_gap=min(topk_gap, stats.get("sort_gap", math.inf), final_gap), merges=stats.get("merges", 0),
                merges32=stats.get("merges32", 0), truncated=stats.get("truncated", 0), labels=labels)
