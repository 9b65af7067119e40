"""tests/nsc_restatement.py (the float64 restatement the GPU tests of the batched nsc transducer search compare against) pinned to a
plain per-utterance statement of N-step constrained decoding without an LM, in the shape of BeamSearchTransducer._nsc: Python
hypothesis objects, the length sort, the in-place prefix rescoring, sorted(), list membership for substract, the last V's blank
term when nstep != 1.  The fixtures' encoder output needs the GPU model, so the pin to the reference's recorded n-best lists
(dec_nsc3_*, dec_nsc3n2_*, dec_nsc2n3_* of tests/golden/transducer_rnn.npz / transducer_gru.npz) happens in
tests/test_gpu_rnnt_nsc.py; here seeded small models are decoded both ways.  Also checked here, on the CPU: single calls against
arrays written out by hand, that every case of the GPU test finds a seed that meets its precondition and that the cases together
meet every prefix depth, substract and a short V, and that the new entry point refuses bad arguments on the host."""
import ctypes

import numpy as np
import pytest

from nsc_restatement import new_pairs, new_s, new_state, nsc_batch64, nsc_step64
from rnnt_greedy_restatement import act64, pred_step64, seeded_weights, weights_from_state_dict


class _H:
    def __init__(self, score, yseq):
        self.score, self.yseq = score, yseq


def _pred_out(w, yseq, cache):
    """prediction-network output after consuming yseq (leading blank included), from the zero state"""
    key = tuple(yseq)
    if key not in cache:
        L, H = len(w["layers"]), w["layers"][0][1].shape[1]
        st = (np.zeros((L, 1, H)), np.zeros((L, 1, H)))
        for t in yseq:
            st = pred_step64(w, np.array([t]), st, np.ones(1, bool))
        cache[key] = st[0][-1][0]
    return cache[key]


def plain_nsc(w, h, beam_size, nstep, prefix_alpha, score_norm=True, act="tanh"):
    """N-step constrained decoding of one utterance's encoder states h [T, D_enc] with Python lists"""
    V = w["lin_out_w"].shape[0]
    beam = min(beam_size, V)
    k = min(beam, V - 1)
    enc = np.asarray(h, np.float64) @ w["lin_enc_w"].T + w["lin_enc_b"]
    cache = {}

    def logp_of(t, yseqs):
        y = np.stack([_pred_out(w, s, cache) for s in yseqs])
        logits = act64(enc[t][None, :] + y @ w["lin_dec_w"].T, act) @ w["lin_out_w"].T + w["lin_out_b"]
        mx = logits.max(1, keepdims=True)
        return logits - mx - np.log(np.exp(logits - mx).sum(1, keepdims=True))

    kept = [_H(0.0, [0])]
    for t in range(enc.shape[0]):
        hyps = sorted(kept, key=lambda x: len(x.yseq), reverse=True)
        for j in range(len(hyps) - 1):
            for i in range(j + 1, len(hyps)):
                yj, yi = hyps[j].yseq, hyps[i].yseq
                if len(yi) < len(yj) and yj[:len(yi)] == yi and len(yj) - len(yi) <= prefix_alpha:
                    curr = hyps[i].score + float(logp_of(t, [yi])[0, yj[len(yi)]])
                    for m in range(len(yi), len(yj) - 1):
                        curr += float(logp_of(t, [yj[:m + 1]])[0, yj[m + 1]])
                    hyps[j].score = float(np.logaddexp(hyps[j].score, curr))
        S, Vl = [], []
        for n in range(nstep):
            if n > 0 and not hyps:
                break
            logp = logp_of(t, [x.yseq for x in hyps])
            order = np.argsort(-logp[:, 1:], axis=1, kind="stable")[:, :k] + 1
            Vl = []
            for i, x in enumerate(hyps):
                for tok in order[i]:
                    Vl.append(_H(x.score + float(logp[i, tok]), x.yseq + [int(tok)]))
                nb = _H(x.score + float(logp[i, 0]), x.yseq[:])
                S.append(nb)
                Vl.append(nb)
            Vl = sorted(Vl, key=lambda x: x.score, reverse=True)
            seqs = [x.yseq for x in hyps]
            Vl = [x for x in Vl if x.yseq not in seqs][:beam]
            if n < nstep - 1:
                hyps = Vl[:]
            elif nstep != 1 and Vl:
                logp = logp_of(t, [x.yseq for x in Vl])
                for i, x in enumerate(Vl):
                    x.score += float(logp[i, 0])
        kept = sorted(S + Vl, key=lambda x: x.score, reverse=True)[:beam]
    if score_norm:
        kept = sorted(kept, key=lambda x: x.score / len(x.yseq), reverse=True)
    else:
        kept = sorted(kept, key=lambda x: x.score, reverse=True)
    return [(x.score, x.yseq) for x in kept]


def _case(seed, dtype, L, H, J, V, n, T):
    sd = seeded_weights(seed, dtype, L, H, 6, J, V, 8, {2: 0.0, 6: 2.0}.get(V, 4.0))
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((n, T, 8)).astype(np.float32)
    hlens = r.integers(3, T + 1, n)
    hlens[0], hlens[-1] = T, 1
    if n > 2:
        hlens[1] = 2
    if n > 3:
        hlens[2] = 0
    return weights_from_state_dict(sd), hs, hlens


@pytest.mark.parametrize("dtype,L,H,J,V", [("lstm", 1, 12, 7, 6), ("gru", 2, 12, 7, 6), ("lstm", 2, 16, 20, 40), ("gru", 1, 12, 7, 2)])
@pytest.mark.parametrize("beam,N,alpha,score_norm", [(2, 3, 3, False), (3, 2, 1, True), (8, 1, 2, True), (4, 4, 2, True),
                                                     (3, 1, 0, True), (5, 2, 0, False)])
def test_batched_restatement_equals_the_plain_statement(dtype, L, H, J, V, beam, N, alpha, score_norm):
    """nsc_batch64 (n * W rows per call in lock-step, blocks, history rows, the device-side pair list, nsc_step64) against the plain
    statement on every utterance alone; an utterance without frames returns [blank] with score 0"""
    w, hs, hlens = _case(3 + beam, dtype, L, H, J, V, 5, 7)
    got = nsc_batch64(w, hs, hlens, beam, N, alpha, score_norm)
    for b in range(len(hlens)):
        want = plain_nsc(w, hs[b, :hlens[b]], beam, N, alpha, score_norm)
        assert [y for _s, y in got["nbest"][b]] == [y for _s, y in want], (b, got["nbest"][b], want)
        for (s, _y), (s_ref, _y2) in zip(got["nbest"][b], want):
            assert abs(s - s_ref) <= 1e-10 * max(1.0, abs(s_ref)), (b, s, s_ref)
    assert got["nbest"][2] == [(0.0, [0])] and hlens[2] == 0
    assert got["min_gap"] > 0
    if alpha == 0:
        assert got["prefix"] == [0, 0, 0]
    if V > 2:
        assert got["substracted"] > 0


def test_whole_batch_lengths_none():
    w, hs, _ = _case(11, "lstm", 1, 12, 7, 6, 2, 5)
    got = nsc_batch64(w, hs, None, 3, 2, 1)
    for b in range(2):
        want = plain_nsc(w, hs[b], 3, 2, 1)
        assert [y for _s, y in got["nbest"][b]] == [y for _s, y in want]


def _la(*v):
    out = v[0]
    for x in v[1:]:
        out = float(np.logaddexp(out, x))
    return out


def test_one_call_restatement_on_hand_made_calls():
    """one utterance, W = 3, V = 5, N = 2, alpha = 2, frame 1, kept in parity 1 (block 3): every array written out"""
    n, W, V, T, N, alpha, t = 1, 3, 5, 3, 2, 2, 1
    st, S, pairs = new_state(n, W, T, N), new_s(n, W, N), new_pairs(n, W, alpha)
    assert st["yseq"].shape == (4, 1, 3, 7) and pairs.shape == (6, 2)
    st["count"][3, 0] = 3
    st["score"][3, 0] = [-1.0, -2.0, -3.0]
    st["ulen"][3, 0] = [0, 2, 1]
    st["yseq"][3, 0, 1, :3] = [0, 1, 2]
    st["yseq"][3, 0, 2, :2] = [0, 1]
    S["nS"][0], S["src"][0], S["score"][0] = 5, 4, 9.0         # left over from frame 0: call 0 starts from an empty S
    pair_lp = np.array([9, 9, -0.5, -0.25, -0.125, 9], np.float32)      # slot 1: depth 1, depth 2; slot 2: depth 1
    rec = np.array([[-0.5, -1.0, -1.5, -2.0, 1, 3, 4], [-0.25, -0.5, -4.0, -5.0, 3, 1, 2], [-0.75, -0.0625, -0.1875, -6.0, 2, 4, 1]],
                   np.float32)
    stats = {}
    s1, S1, par, tok, live, hidx, p1 = nsc_step64(rec, pair_lp, None, st, S, pairs, V, T, N, alpha, t, 0, 1, stats)
    # hyps = [0, 1, 2], [0, 1], [0]: the first gains [0, 1] (depth 1) and then [0] (depth 2: -0.25, then -0.5), the second gains [0]
    # (depth 1), each from the scores as they were
    s_a = _la(-2.0, -3.0 + -0.5, (-1.0 + -0.25) + -0.5)
    s_b = _la(-3.0, -1.0 + -0.125)
    assert stats["prefix1"] == 2 and stats["prefix2"] == 1 and "prefix3" not in stats
    assert S1["nS"].tolist() == [3] and S1["src"][0].tolist() == [10, 11, 9, 4, 4, 4]
    assert S1["score"][0].tolist() == [s_a - 0.25, s_b - 0.75, -1.5, 9.0, 9.0, 9.0]
    # substract: [0] + 1 = [0, 1] and [0, 1] + 2 = [0, 1, 2] are members of hyps
    assert stats["substracted"] == 2
    ext = sorted([(s_a - 0.5, 10, 3), (s_a - 4.0, 10, 1), (s_a - 5.0, 10, 2), (s_b - 0.1875, 11, 4), (s_b - 6.0, 11, 1), (-2.5, 9, 3),
                  (-3.0, 9, 4)], key=lambda x: x[0], reverse=True)[:3]
    assert s1["score"][1, 0].tolist() == [e[0] for e in ext] and par.tolist() == [e[1] for e in ext]
    assert tok.tolist() == [e[2] for e in ext] and live.tolist() == [1, 1, 1] and s1["count"][:, 0].tolist() == [1, 3, 0, 3]
    assert np.array_equal(p1, pairs) and np.array_equal(s1["score"][3], st["score"][3])
    # hrow(block row 9 + s, level) = (3 * 3 + level) * 3 + s: a row that appended takes its parent's d as hist[1], its hist[1] as hist[2]
    assert hidx[:, 0].tolist() == [(9 + 0) * 3 + par[0] - 9, (9 + 0) * 3 + par[0] - 9, (9 + 1) * 3 + par[0] - 9]
    # the finishing call: block 2 holds V of n-step 1; S + V sorted, the pair list of frame 2 written
    s1["count"][2, 0] = 1
    s1["score"][2, 0, 0], s1["ulen"][2, 0, 0] = -0.5, 2
    s1["yseq"][2, 0, 0, :3] = [0, 3, 4]
    rec = np.full((3, 7), -1.0, np.float32)
    s2, S2, par, tok, live, hidx, p2 = nsc_step64(rec, pair_lp, None, s1, S1, pairs, V, T, N, alpha, t, 2, 1, stats)
    want = sorted([(s_a - 0.25, 10), (s_b - 0.75, 11), (-1.5, 9), (-1.5, 6)], key=lambda x: x[0], reverse=True)[:3]
    assert s2["count"][0, 0] == 3 and s2["score"][0, 0].tolist() == [e[0] for e in want] and par.tolist() == [e[1] for e in want]
    assert tok.tolist() == [0, 0, 0] and live.tolist() == [0, 0, 0]
    for m, (_s, src) in enumerate(want):
        y = {10: [0, 1, 2], 11: [0, 1], 9: [0], 6: [0, 3, 4]}[src]
        assert s2["yseq"][0, 0, m, :len(y)].tolist() == y and s2["ulen"][0, 0, m] == len(y) - 1
        assert hidx[:, m].tolist() == [((src // 3) * 3 + a) * 3 + src % 3 for a in range(3)]
        for a in (1, 2):
            assert p2[m * 2 + a - 1].tolist() == ([a * 3 + m, y[len(y) - a]] if a <= len(y) - 1 else [-1, 0])


def test_one_call_restatement_idles_past_the_end():
    """two utterances, hlens 1 and 3, frame 1, N = 1: the first one's kept is carried into the other parity, its rows point at
    themselves in kept's block"""
    n, W, V, T, N, alpha = 2, 2, 4, 3, 1, 1
    st, S, pairs = new_state(n, W, T, N), new_s(n, W, N), new_pairs(n, W, alpha)
    st["count"][2] = [2, 1]                                   # parity 1 = block 2 is read
    st["score"][2] = [[-1.0, -2.0], [-0.5, 0.0]]
    st["ulen"][2, 0] = [1, 0]
    st["yseq"][2, 0, 0, :2] = [0, 3]
    st["score"][0], st["count"][0], st["yseq"][0] = 7.0, -3, -3     # what frame 0 left in the other parity
    rec = np.array([[-3, -1, -1, 1, 2]] * 4, np.float32)
    s1, S1, par, tok, live, hidx, p1 = nsc_step64(rec, np.zeros(4, np.float32), np.array([1, 3]), st, S, pairs, V, T, N, alpha, 1, 0, 1)
    assert par.tolist() == [8, 9, 10, 10] and tok.tolist() == [0, 0, 1, 2] and live.tolist() == [0, 0, 1, 1]
    assert s1["count"][0].tolist() == [2, 2] and s1["score"][0, 0].tolist() == [-1.0, -2.0] and s1["ulen"][0, 0].tolist() == [1, 0]
    assert s1["yseq"][0, 0].tolist() == [[0, 3, -3, -3], [0, -3, -3, -3]] and s1["yseq"][0, 1].tolist() == [[0, 1, -3, -3], [0, 2, -3, -3]]
    assert S1["nS"].tolist() == [0, 1] and p1.tolist() == [[-1, 0], [-1, 0], [4 + 2, 1], [4 + 3, 2]]
    assert hidx.tolist() == [[16, 17, 18, 18], [20, 21, 18, 18]]


def test_every_gpu_search_case_finds_a_seed():
    """the deterministic seed search of tests/test_gpu_rnnt_nsc.py, run with the restatement alone; together the cases meet prefix
    terms of depth 1 and 2, substract and a V shorter than W"""
    import test_gpu_rnnt_nsc as g
    assert len(g.SEARCH_CASES) == 48
    shapes = {c[3:] for c in g.SEARCH_CASES}
    assert shapes >= {(7, 6, 20, 1, 1, 3), (7, 6, 3, 2, 2, 2), (52, 257, 3, 2, 1, 8), (52, 257, 2, 3, 3, 16), (52, 257, 8, 1, 2, 4)}
    for col, vals in enumerate([("lstm", "gru"), (1, 2), (12, 64)]):
        assert {c[col] for c in g.SEARCH_CASES} == set(vals), col
    tot = dict(p1=0, p2=0, substracted=0, short_v=0, dup_kept=0, labels=0)
    for case in g.SEARCH_CASES:
        seed = g.search_seed(*case)
        ref = g.search_reference(*case, seed)
        assert ref["min_gap"] >= g.GAP
        tot["p1"] += ref["prefix"][0]
        tot["p2"] += ref["prefix"][1]
        for key in ("substracted", "short_v", "dup_kept", "labels"):
            tot[key] += ref[key]
    print("[coverage] nsc search cases:", tot)
    assert tot["p1"] > 0 and tot["p2"] > 0 and tot["substracted"] > 0 and tot["short_v"] > 0 and tot["labels"] > 0, tot


def test_the_entry_point_refuses_bad_arguments_on_the_host():
    """NULL operands, one array for two operands, a call beyond the frame's: EAMD_EINVAL; 17 slots, nstep 5, prefix_alpha 4, more
    slots than tokens: EAMD_EUNSUPPORTED - all before any launch, so without a GPU"""
    from espnet_amd import _lib
    L = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, _lib.EAMD_EUNSUPPORTED            # include/espnet_amd.h
    bufs = [(ctypes.c_double * 64)() for _ in range(14)]     # never read: every call below is refused on the host
    ptrs = [ctypes.addressof(x) for x in bufs]

    def call(p, n=1, W=2, V=6, T=3, N=2, alpha=1, t=0, v=0, par=0):
        return L.eamd_rnnt_nsc_step(*p, n, W, V, T, N, alpha, t, v, par, None)

    ok = ptrs[:2] + [None] + ptrs[2:]                         # hlens may be NULL
    assert len(ok) == 15
    for i in [0, 1] + list(range(3, 15)):
        assert call(ok[:i] + [None] + ok[i + 1:]) == EINVAL, i
    assert call([None] * 15) == EINVAL
    assert call(ok[:4] + [ok[8]] + ok[5:]) == EINVAL           # ulen and s_src in one array
    assert call(ok[:13] + [ok[14], ok[14]]) == EINVAL          # hidx and pairs in one array
    assert call([ok[0], ok[0]] + ok[2:]) == EINVAL             # rec and pair_lp in one array
    for kw in (dict(n=0), dict(V=1), dict(T=0), dict(v=3), dict(N=1, v=1), dict(t=-1), dict(par=2), dict(W=0)):
        assert call(ok, **kw) == EINVAL, kw
    for kw in (dict(W=17, V=40), dict(N=5), dict(W=7, V=6), dict(N=0), dict(alpha=4), dict(alpha=-1)):
        assert call(ok, **kw) == EUNSUPPORTED, kw
