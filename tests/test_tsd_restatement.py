"""tests/tsd_restatement.py (the float64 restatement the GPU tests of the batched tsd transducer search compare against) pinned to
a plain per-utterance statement of time-synchronous decoding without an LM, in the shape of BeamSearchTransducer._tsd: Python
hypothesis objects, the snapshot seq_A, sorted(), every one of the max_sym_exp passes expanding.  The fixtures' encoder output needs
the GPU model, so the pin to the reference's recorded n-best lists (dec_tsd3_*, dec_tsd2_* of tests/golden/transducer_rnn.npz /
transducer_gru.npz) happens in tests/test_gpu_rnnt_tsd.py; here seeded small models are decoded both ways.  Also checked here, on the
CPU: single passes against arrays written out by hand, that every case of the GPU test finds a seed that meets its precondition,
and that the new entry point refuses bad arguments on the host."""
import ctypes

import numpy as np
import pytest

from rnnt_greedy_restatement import act64, pred_step64, seeded_weights, weights_from_state_dict
from tsd_restatement import new_a, new_state, tsd_batch64, tsd_step64


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


def plain_tsd(w, h, beam_size, max_sym_exp, score_norm=True, act="tanh"):
    """time-synchronous decoding of one utterance's encoder states h [T, D_enc] with Python lists"""
    V = w["lin_out_w"].shape[0]
    beam = min(beam_size, V)
    k = min(beam, V - 1)
    enc = np.asarray(h, np.float64) @ w["lin_enc_w"].T + w["lin_enc_b"]
    cache = {}
    B = [_H(0.0, [0])]
    for t in range(enc.shape[0]):
        A = []
        C = B
        for _v in range(max_sym_exp):
            y = np.stack([_pred_out(w, c.yseq, cache) for c in C])
            logits = act64(enc[t][None, :] + y @ w["lin_dec_w"].T, act) @ w["lin_out_w"].T + w["lin_out_b"]
            mx = logits.max(1, keepdims=True)
            logp = logits - mx - np.log(np.exp(logits - mx).sum(1, keepdims=True))
            order = np.argsort(-logp[:, 1:], axis=1, kind="stable")[:, :k] + 1
            seq_A = [a.yseq for a in A]
            for i, c in enumerate(C):
                if c.yseq not in seq_A:
                    A.append(_H(c.score + float(logp[i, 0]), c.yseq[:]))
                else:
                    a = A[seq_A.index(c.yseq)]
                    a.score = float(np.logaddexp(a.score, c.score + float(logp[i, 0])))
            D = []
            for i, c in enumerate(C):
                for tok in order[i]:
                    D.append(_H(c.score + float(logp[i, tok]), c.yseq + [int(tok)]))
            C = sorted(D, key=lambda x: x.score, reverse=True)[:beam]
        B = sorted(A, key=lambda x: x.score, reverse=True)[:beam]
    if score_norm:
        B = sorted(B, key=lambda x: x.score / len(x.yseq), reverse=True)
    else:
        B = sorted(B, key=lambda x: x.score, reverse=True)
    return [(x.score, x.yseq) for x in B]


def _case(seed, dtype, L, H, J, V, n, T):
    sd = seeded_weights(seed, dtype, L, H, 6, J, V, 8, {2: 0.0, 6: 2.0}.get(V, 4.0))
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((n, T, 8)).astype(np.float32)
    hlens = r.integers(3, T + 1, n)
    hlens[0], hlens[-1] = T, 1
    if n > 2:
        hlens[1] = 2
    return weights_from_state_dict(sd), hs, hlens


@pytest.mark.parametrize("dtype,L,H,J,V", [("lstm", 1, 12, 7, 6), ("gru", 2, 12, 7, 6), ("lstm", 2, 16, 20, 40), ("gru", 1, 12, 7, 2)])
@pytest.mark.parametrize("beam,M,score_norm", [(2, 3, False), (3, 2, True), (8, 1, True), (4, 4, True)])
def test_batched_restatement_equals_the_plain_statement(dtype, L, H, J, V, beam, M, score_norm):
    """tsd_batch64 (n * W rows per pass in lock-step, blocks, tsd_step64) against the plain statement on every utterance alone"""
    w, hs, hlens = _case(3 + beam, dtype, L, H, J, V, 5, 7)
    got = tsd_batch64(w, hs, hlens, beam, M, score_norm)
    for b in range(len(hlens)):
        want = plain_tsd(w, hs[b, :hlens[b]], beam, M, score_norm)
        assert [y for _s, y in got["nbest"][b]] == [y for _s, y in want], (b, got["nbest"][b], want)
        for (s, _y), (s_ref, _y2) in zip(got["nbest"][b], want):
            assert abs(s - s_ref) <= 1e-10 * max(1.0, abs(s_ref)), (b, s, s_ref)
    assert got["min_gap"] > 0
    if M > 1 and V > 2:
        assert got["merges"] > 0 and got["truncated"] > 0
    if M == 1:                                              # no expansion is ever used: only [blank] survives
        assert got["labels"] == 0 and all(nb == [(nb[0][0], [0])] for nb in got["nbest"])


def test_whole_batch_lengths_none():
    w, hs, _ = _case(11, "lstm", 1, 12, 7, 6, 2, 5)
    got = tsd_batch64(w, hs, None, 3, 2)
    for b in range(2):
        want = plain_tsd(w, hs[b], 3, 2)
        assert [y for _s, y in got["nbest"][b]] == [y for _s, y in want]


def _la(*v):
    out = v[0]
    for x in v[1:]:
        out = float(np.logaddexp(out, x))
    return out


def test_one_pass_restatement_on_hand_made_passes():
    """frame 1 of one utterance, W = 2, M = 2 (blocks: 0 = B read, 1 = C of pass 1, 2 = B written), every array written out"""
    n, W, V, T, M, t = 1, 2, 4, 3, 2, 1
    st, A = new_state(n, W, T, M), new_a(n, W, M)
    assert st["yseq"].shape == (3, 1, 2, 4)
    st["count"][0, 0] = 2
    st["score"][0, 0] = [-1.0, -2.0]
    st["ulen"][0, 0] = [1, 0]
    st["yseq"][0, 0, 0, :2] = [0, 2]
    A["nA"][0], A["src"][0], A["score"][0] = 3, 5, 9.0       # left over from frame 0: pass 0 starts from an empty A
    rec = np.array([[-0.5, -0.25, -4.0, 3, 1], [-0.25, -0.75, -3.0, 2, 1]], np.float32)
    s1, A1, par, tok, live = tsd_step64(rec, None, st, A, V, T, M, t, 0, 0)
    assert A1["nA"].tolist() == [2] and A1["score"][0].tolist() == [-1.5, -2.25, 9.0, 9.0] and A1["src"][0].tolist() == [0, 1, 5, 5]
    # D = [0, 2, 3]: -1.25, [0, 2, 1]: -5, [0, 2]: -2.75, [0, 1]: -5
    assert s1["count"][:, 0].tolist() == [2, 2, 0]
    assert s1["score"][1, 0].tolist() == [-1.25, -2.75] and s1["ulen"][1, 0].tolist() == [2, 1]
    assert s1["yseq"][1, 0].tolist() == [[0, 2, 3, 0], [0, 2, 0, 0]]
    assert par.tolist() == [0, 1] and tok.tolist() == [3, 2] and live.tolist() == [1, 1]
    assert np.array_equal(s1["score"][0], st["score"][0]) and np.array_equal(s1["yseq"][0], st["yseq"][0])
    # the frame's end: [0, 2, 3] is new, [0, 2] of C joins A's first entry; three entries, two kept
    rec = np.array([[-0.125, -9, -9, 1, 2], [-0.25, -9, -9, 1, 2]], np.float32)
    stats = {}
    s2, A2, par, tok, live = tsd_step64(rec, None, s1, A1, V, T, M, t, 1, 0, stats)
    grown = _la(-1.5, -3.0)
    assert A2["nA"].tolist() == [3] and A2["score"][0].tolist() == [grown, -2.25, -1.375, 9.0] and A2["src"][0].tolist() == [0, 1, 2, 5]
    assert stats["merges"] == 1 and stats["truncated"] == 1
    assert s2["count"][:, 0].tolist() == [2, 2, 2]
    assert s2["score"][2, 0].tolist() == [grown, -1.375] and s2["ulen"][2, 0].tolist() == [1, 2]
    assert s2["yseq"][2, 0].tolist() == [[0, 2, 0, 0], [0, 2, 3, 0]]
    assert par.tolist() == [0, 2] and tok.tolist() == [0, 0] and live.tolist() == [0, 0]
    # equal scores keep the list's order; fewer candidates than slots: V = 2, one hypothesis, one extension
    st = new_state(1, 2, 3, 2)
    rec = np.array([[-1.0, -1.0, 1], [0, 0, 1]], np.float32)
    s1, A1, par, tok, live = tsd_step64(rec, None, st, new_a(1, 2, 2), 2, 3, 2, 0, 0, 0)
    assert s1["count"][:, 0].tolist() == [1, 1, 0] and s1["yseq"][1, 0, 0].tolist() == [0, 1, 0, 0]
    assert par.tolist() == [0, 1] and tok.tolist() == [1, 0] and live.tolist() == [1, 0]


def test_one_pass_restatement_idles_past_the_end():
    """two utterances, hlens 1 and 3, frame 1: the first one's B is carried into the other parity on the last pass only, its rows
    point at themselves in B's block"""
    n, W, V, T, M = 2, 2, 4, 3, 2
    st, A = new_state(n, W, T, M), new_a(n, W, M)
    st["count"][2] = [2, 1]                                   # parity 1 = block 2 is read
    st["score"][2] = [[-1.0, -2.0], [-0.5, 0.0]]
    st["ulen"][2, 0] = [1, 0]
    st["yseq"][2, 0, 0, :2] = [0, 3]
    st["score"][0], st["count"][0], st["yseq"][0] = 7.0, -3, -3     # what frame 0 left in the other parity
    rec = np.full((4, 5), -1.0, np.float32)
    rec[:, 3:] = [1, 2]
    hl = np.array([1, 3])
    s1, A1, par, tok, live = tsd_step64(rec, hl, st, A, V, T, M, 1, 0, 1)
    assert par.tolist() == [8, 9, 10, 10] and live.tolist() == [0, 0, 1, 1] and A1["nA"].tolist() == [0, 1]
    assert s1["count"][1].tolist() == [0, 2] and s1["count"][0].tolist() == [-3, -3]
    s2, A2, par, tok, live = tsd_step64(rec, hl, s1, A1, V, T, M, 1, 1, 1)
    assert par[:2].tolist() == [8, 9] and live.tolist() == [0, 0, 0, 0]
    assert s2["count"][0].tolist() == [2, 2] and s2["score"][0, 0].tolist() == [-1.0, -2.0] and s2["ulen"][0, 0].tolist() == [1, 0]
    assert s2["yseq"][0, 0].tolist() == [[0, 3, -3, -3], [0, -3, -3, -3]]


def test_every_gpu_search_case_finds_a_seed():
    """the deterministic seed search of tests/test_gpu_rnnt_tsd.py, run with the restatement alone"""
    import test_gpu_rnnt_tsd as g
    assert len(g.SEARCH_CASES) == 40
    for col, vals in enumerate([("lstm", "gru"), (1, 2), (12, 64), (7, 52), (6, 257), (3, 8, 20), (2, 3, 4), (2, 3, 4, 8, 16)]):
        assert {c[col] for c in g.SEARCH_CASES} == set(vals), col
    labels = 0
    for case in g.SEARCH_CASES:
        seed = g.search_seed(*case)
        ref = g.search_reference(*case, seed)
        assert ref["min_gap"] >= g.GAP
        assert ref["merges"] > 0 and ref["truncated"] > 0, case
        labels += ref["labels"]
    assert labels > 0


def test_the_entry_point_refuses_bad_arguments_on_the_host():
    """NULL operands, one array for two operands, a pass beyond max_sym_exp: EAMD_EINVAL; 17 slots, max_sym_exp 5, more slots than
    tokens: EAMD_EUNSUPPORTED - all before any launch, so without a GPU"""
    from espnet_amd import _lib
    L = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, _lib.EAMD_EUNSUPPORTED            # include/espnet_amd.h
    bufs = [(ctypes.c_double * 64)() for _ in range(11)]     # never read: every call below is refused on the host
    ptrs = [ctypes.addressof(x) for x in bufs]

    def call(p, n=1, W=2, V=6, T=3, M=2, t=0, v=0, par=0):
        return L.eamd_rnnt_tsd_step(*p, n, W, V, T, M, t, v, par, None)

    ok = [ptrs[0], None] + ptrs[1:]                           # hlens may be NULL
    for i in [0] + list(range(2, 12)):
        assert call(ok[:i] + [None] + ok[i + 1:]) == EINVAL, i
    assert call([None] * 12) == EINVAL
    assert call(ok[:3] + [ok[7]] + ok[4:]) == EINVAL           # ulen and a_src in one array
    for kw in (dict(n=0), dict(V=1), dict(T=0), dict(v=2), dict(t=-1), dict(par=2), dict(W=0)):
        assert call(ok, **kw) == EINVAL, kw
    for kw in (dict(W=17, V=40), dict(M=5), dict(W=7, V=6), dict(M=0)):
        assert call(ok, **kw) == EUNSUPPORTED, kw
