"""tests/default_restatement.py (the float64 restatement the GPU tests of the batched default transducer search compare against)
pinned to plain_default, a plain per-utterance statement of the reference's loop (espnet/nets/beam_search_transducer.py:163-237
without an LM): A and B as Python lists, A never pruned, max() for the first maximum, sorted() for ahead.  default_step64 is driven
with joint rows on a score grid of 1 / 4 (ties everywhere); default_batch64 decodes seeded small models.  The fixtures' encoder output
needs the GPU model, so the pin to the reference's recorded n-best lists happens in tests/test_gpu_rnnt_default.py.  Also checked
here, on the CPU: every search case of the GPU test finds a seed that meets its preconditions."""
import numpy as np
import pytest

from default_restatement import C_CUR, C_T, default_batch64, default_step64, final_b, labels_of, nbest, new_state, plain_default
from rnnt_greedy_restatement import act64, pred_step64, seeded_weights, weights_from_state_dict


def grid_rows(seed, V, k, blank_lo, blank_hi):
    """joint rows on a grid of 1 / 4, a function of (utterance, frame, labels) alone: blank in -[blank_lo, blank_hi) / 4, the k
    extensions in -[2, 14) / 4 in descending order with distinct tokens"""
    def row(b, t, y):
        r = np.random.default_rng([seed, b, t] + [int(v) for v in y])
        ext = -np.sort(r.integers(2, 14, k)) / 4.0
        toks = r.permutation(np.arange(1, V))[:k]
        return -float(r.integers(blank_lo, blank_hi)) / 4.0, list(zip(ext.tolist(), toks.tolist()))
    return row


def drive_steps(row, hlens, W, V, T, P, log_cap, stats):
    """the whole search of n utterances through default_step64, the pending pops' rows from row(b, t, labels)"""
    n, k = len(hlens), min(W, V - 1)
    st, out = new_state(n, P, log_cap, hlens, T)
    steps = 0
    while not (st["flags"][0] | st["flags"][1]).all():
        rec = np.zeros((n, 1 + 2 * k))
        for b in np.nonzero(out["alive"])[0]:
            t, cur = int(st["ctr"][b, C_T]), int(st["ctr"][b, C_CUR])
            assert out["frame"][b] == b * T + t and out["live"][b] == (st["log"][b, cur, 1] != 0)
            blank_lp, ext = row(b, t, labels_of(st["log"][b], cur))
            rec[b] = [blank_lp] + [lp for lp, _t in ext] + [tk for _lp, tk in ext]
        st, out = default_step64(rec, hlens, st, W, V, T, stats)
        steps += 1
    return st, steps


@pytest.mark.parametrize("W,V,blank", [(1, 2, (0, 3)), (2, 2, (0, 3)), (3, 3, (0, 3)), (2, 6, (0, 3)), (4, 6, (2, 9)), (8, 40, (0, 4)),
                                       (16, 40, (0, 3)), (3, 6, (6, 14))])
def test_step_restatement_equals_the_plain_loop_on_a_score_grid(W, V, blank):
    """scores on a grid of 1 / 4: ties between carried entries and children, in B against bound and within ahead.  W == V (k < W),
    weak blanks (frames of many pops), and A cut at P = the most pops a frame takes (the cut must change nothing)"""
    T, k = 5, min(W, V - 1)
    hlens = [T, 0, 1, 2, 4]
    row = grid_rows(7 * W + V, V, k, *blank)
    plain = [plain_default(lambda t, y, b=b: row(b, t, y), hlens[b], W, k, score_norm=bool(b & 1)) for b in range(len(hlens))]
    most = max(max(p[1], default=0) for p in plain)
    for P in (256, max(W, most)):
        stats = {}
        st, steps = drive_steps(row, hlens, W, V, T, P, 1 + sum(sum(p[1]) for p in plain), stats)
        assert not st["flags"][1].any() and st["flags"][0].all()
        assert steps == max(sum(p[1]) for p in plain)                        # one pop per step: the slowest utterance decides
        for b, (want, pops) in enumerate(plain):
            got, _gap = nbest(final_b(st, b), bool(b & 1))
            assert got == want, (P, b, got, want)
            assert stats.get("pops", {}).get(b, []) == pops
        assert stats["gap"] == 0.0 or V < 6                                  # ties were met
        if blank[0] >= 6:
            assert most > 4 * W and (stats["cut"] > 0) == (P < 256), (most, stats)
    # one pop too few: the utterance with the longest frame overflows, the others are what they were
    if most > W:
        st, _ = drive_steps(row, hlens, W, V, T, most - 1, 4096, {})
        slow = [b for b, p in enumerate(plain) if max(p[1], default=0) == most]
        assert [b for b in range(len(hlens)) if st["flags"][1, b]] == slow
        for b in set(range(len(hlens))) - set(slow):
            assert nbest(final_b(st, b), bool(b & 1))[0] == plain[b][0]


def test_step_restatement_meets_long_ahead_lists():
    tot = 0
    for W, V in ((2, 6), (3, 6), (4, 40)):
        stats = {}
        drive_steps(grid_rows(W, V, min(W, V - 1), 0, 2), [6, 6, 6], W, V, 6, 256, 4096, stats)
        tot += stats["long_ahead"]
    assert tot > 0


def test_one_step_restatement_on_a_hand_made_step():
    """frame 1 of a beam-2 search: the pending pop's best child ties with a carried entry - the carried one, earlier in list order,
    is popped -; then a step that ends the frame with ahead longer than W"""
    n, W, V, T, P = 1, 2, 6, 3, 8
    st, _ = new_state(n, P, 16, [T], T)
    st["ctr"][0, :7] = [1, 1, 1, 0, 3, 2, 2]                  # t, pops, nA, nB, nlog, seq, cur
    st["log"][0, 1], st["log"][0, 2] = (0, 0), (0, 4)
    st["cur"][0] = -0.5
    st["a_score"][0, 0], st["a_seq"][0, 0], st["a_row"][0, 0], st["a_log"][0, 0] = -1.0, 1, 1, 1
    rec = np.array([[-9.0, -0.5, -2.0, 3, 5]])
    s1, out = default_step64(rec, None, st, W, V, T)
    assert (out["par"][0], out["tok"][0], out["dst"][0], out["live"][0], out["frame"][0], out["alive"][0]) == (1, 0, P + 1, 0, 1, 1)
    assert s1["ctr"][0, :7].tolist() == [1, 2, 2, 1, 4, 4, 3] and s1["log"][0, 3].tolist() == [1, 0] and s1["cur"][0] == -1.0
    assert s1["a_score"][0, :2].tolist() == [-1.0, -2.5] and s1["a_tok"][0, :2].tolist() == [3, 5] and s1["a_row"][0, :2].tolist() == [P, P]
    assert s1["b_score"][0, 0] == -9.5 and s1["b_row"][0, 0] == P and s1["b_log"][0, 0] == 2
    st, _ = new_state(n, P, 16, [T], T)
    st["ctr"][0, :7] = [0, 4, 0, 3, 4, 8, 3]
    st["b_score"][0, :3], st["b_log"][0, :3], st["b_row"][0, :3] = [-1.0, -1.25, -1.125], [0, 1, 2], [0, 1, 2]
    st["cur"][0] = -0.875
    stats = {}
    s1, out = default_step64(np.array([[-0.0625, -5.0, -6.0, 1, 2]]), None, st, W, V, T, stats)
    assert stats["long_ahead"] == 1 and stats["pops"] == {0: [4]}
    assert s1["ctr"][0, :7].tolist() == [1, 1, 3, 0, 5, 4, 4] and s1["cur"][0] == -0.9375 and s1["log"][0, 4].tolist() == [3, 0]
    assert s1["a_score"][0, :3].tolist() == [-1.0, -1.125, -1.25] and s1["a_seq"][0, :3].tolist() == [2, 1, 0]
    assert (out["par"][0], out["dst"][0], out["frame"][0], out["live"][0]) == (3, P, 1, 0)


# ---- the whole search on seeded models ------------------------------------------------------------------------------------------
def _pred_out(w, yseq, cache):
    key = tuple(yseq)
    if key not in cache:
        L, H = len(w["layers"]), w["layers"][0][1].shape[1]
        st = (np.zeros((L, 1, H)), np.zeros((L, 1, H)))
        for t in yseq:
            st = pred_step64(w, np.array([t]), st, np.ones(1, bool))
        cache[key] = st[0][-1][0]
    return cache[key]


def reference_default(w, h, beam_size, score_norm=True, act="tanh"):
    """plain_default on one utterance's encoder states h [T, D_enc], the joint rows from the model"""
    V = w["lin_out_w"].shape[0]
    beam = min(beam_size, V)
    k = min(beam, V - 1)
    enc = np.asarray(h, np.float64) @ w["lin_enc_w"].T + w["lin_enc_b"]
    cache = {}

    def row(t, y):
        logits = act64(enc[t] + _pred_out(w, y, cache) @ w["lin_dec_w"].T, act) @ w["lin_out_w"].T + w["lin_out_b"]
        logp = logits - logits.max() - np.log(np.exp(logits - logits.max()).sum())
        order = np.argsort(-logp[1:], kind="stable")[:k] + 1
        return float(logp[0]), [(float(logp[j]), int(j)) for j in order]
    return plain_default(row, h.shape[0], beam, k, score_norm)


def _case(seed, dtype, L, H, J, V, n, T):
    sd = seeded_weights(seed, dtype, L, H, 6, J, V, 8, {3: 2.0, 6: 4.0}.get(V, 6.0))
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((n, T, 8)).astype(np.float32)
    hlens = r.integers(3, T + 1, n)
    hlens[0], hlens[-1] = T, 1
    if n > 2:
        hlens[1] = 2
    return weights_from_state_dict(sd), hs, hlens


@pytest.mark.parametrize("dtype,L,H,J,V", [("lstm", 1, 12, 7, 6), ("gru", 2, 12, 7, 6), ("lstm", 2, 16, 20, 40), ("gru", 1, 12, 7, 3)])
@pytest.mark.parametrize("beam,score_norm", [(2, False), (3, True), (8, True)])
def test_batched_restatement_equals_the_plain_loop(dtype, L, H, J, V, beam, score_norm):
    """default_batch64 (n rows in lock-step in pops, the state pool, default_step64) against the plain loop on every utterance alone,
    with A at 256 entries and cut at the most pops a frame takes; duplicates stay"""
    w, hs, hlens = _case(3 + beam, dtype, L, H, J, V, 5, 7)
    plain = [reference_default(w, hs[b, :hlens[b]], beam, score_norm) for b in range(len(hlens))]
    most = max(max(p[1]) for p in plain)
    assert most <= 256
    for P in (256, max(min(beam, V), most)):
        got = default_batch64(w, hs, hlens, beam, P, score_norm)
        assert not any(got["overflow"]) and got["min_gap"] > 0
        for b, (want, pops) in enumerate(plain):
            assert [y for _s, y in got["nbest"][b]] == [y for _s, y in want], (b, got["nbest"][b], want)
            for (s, _y), (s_ref, _y2) in zip(got["nbest"][b], want):
                assert abs(s - s_ref) <= 1e-10 * max(1.0, abs(s_ref)), (b, s, s_ref)
            assert got["pops"][b] == pops and got["total"][b] == sum(pops)
        assert got["steps"] == max(sum(p[1]) for p in plain)


def test_duplicates_stay():
    """no recombination: the first seeded model whose n-best list holds one label sequence twice - the plain loop returns the same
    list, with both entries and their own scores"""
    for seed in range(32):
        w, hs, hlens = _case(seed, "lstm", 1, 12, 7, 6, 3, 7)
        got = default_batch64(w, hs, hlens, 8)
        seqs = [tuple(y) for _s, y in got["nbest"][0]]
        if len(set(seqs)) < len(seqs):
            break
    assert len(set(seqs)) < len(seqs) and got["dups"] > 0
    want, _pops = reference_default(w, hs[0, :hlens[0]], 8)
    assert [y for _s, y in want] == [list(y) for y in seqs]
    assert np.allclose([s for s, _y in want], [s for s, _y in got["nbest"][0]], rtol=1e-10, atol=0)
    assert len({s for s, _y in want}) == len(want)


def test_batched_restatement_cut_off_by_the_step_limit():
    """max_steps = W max(T_b), the least a search takes: the utterances that need more are reported as overflowed, the others are
    what they are without a limit"""
    for seed in range(32):
        w, hs, hlens = _case(seed, "lstm", 1, 12, 7, 6, 3, 6)
        full = default_batch64(w, hs, hlens, 3)
        slow = [b for b in range(3) if full["total"][b] > 3 * int(max(hlens))]
        if slow:
            break
    got = default_batch64(w, hs, hlens, 3, max_steps=3 * int(max(hlens)))
    assert slow and [b for b in range(3) if got["overflow"][b]] == slow and all(got["nbest"][b] is None for b in slow)
    assert all(got["nbest"][b] == full["nbest"][b] for b in range(3) if b not in slow)


def test_every_gpu_search_case_finds_a_seed():
    """the deterministic seed search of tests/test_gpu_rnnt_default.py, run with the restatement alone"""
    import test_gpu_rnnt_default as g
    for col, vals in enumerate([("lstm", "gru"), (1, 2), (12, 64), (7, 52), (6, 257), (2, 3, 20), (2, 3, 4, 8, 16)]):
        assert {c[col] for c in g.SEARCH_CASES} == set(vals), col
    dups = long_ahead = 0
    for case in g.SEARCH_CASES:
        seed = g.search_seed(*case)
        ref = g.search_reference(*case, seed)
        assert g.precondition(case, ref)
        dups += ref["dups"]
        long_ahead += ref["long_ahead"]
    assert dups > 0 and long_ahead > 0, (dups, long_ahead)
