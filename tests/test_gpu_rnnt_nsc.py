"""Batched N-step constrained transducer beam search on the GPU: eamd_rnnt_nsc_step (csrc/rnnt_nsc.hip) and
BeamSearchTransducer.nsc_batch / E2E.recognize_batch against
  * tests/nsc_restatement.py - float64, pinned to a plain per-utterance statement by tests/test_nsc_restatement.py,
  * the per-utterance nsc search of the same package, and
  * the nsc n-best lists the reference recorded in tests/golden/transducer_rnn.npz / transducer_gru.npz.
Kernel: par, tok, live, hidx, the pair list, lengths, labels, counts, s_src and nS exact - whole arrays, so what the kernel must not
write shows as well; scores within 1e-12 relative (float64 sums and the roundings of logaddexp, the bound of
tests/test_gpu_rnnt_tsd.py for the same arithmetic).  Search: same n-best length, same sequences in the same order, scores within
1e-4 relative (the bound of tests/test_gpu_transducer_search.py).  Equal sequences are meaningful where float32 cannot flip an
ordering decision, so every float64 decision gap that is used (top-k boundary of a live row of hyps on a call v < N, adjacent scores
of the sorted extensions and of sorted S + V down to position W + 1 - after prefix rescoring -, adjacent keys of the final sort)
must be >= 1e-4; this precondition is ASSERTED, and each case takes the first seed of its own sequence that meets it on the CPU
(tests/test_nsc_restatement.py checks that every case finds one and that the cases together meet prefix terms of depth 1 and 2,
substract and a V shorter than W; the choice never looks at a GPU result)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from nsc_restatement import kept_block, new_pairs, new_s, new_state, nsc_batch64, nsc_step64
from rnnt_greedy_restatement import seeded_weights, weights_from_state_dict

DEV = "cuda"
GAP = 1e-4


@pytest.fixture(autouse=True)
def _fp32():
    import espnet_amd
    espnet_amd.set_precision("fp32")
    yield
    espnet_amd.set_precision("fp32")


# ---- 1. the step kernel vs the one-call restatement ---------------------------------------------------------------------------
_ST, _SK = ("score", "ulen", "count", "yseq"), ("score", "src", "nS")


def _run_step(rec, pair_lp, hlens, st, S, pairs, V, T, N, alpha, t, v, p):
    """eamd_rnnt_nsc_step on numpy operands -> (blocks, S, par, tok, live, hidx, pairs) as numpy; par / tok / live / hidx start as
    sentinels"""
    from espnet_amd import ops
    _blocks, n, W = st["score"].shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    s, a = tuple(up(st[key]) for key in _ST), tuple(up(S[key]) for key in _SK)
    par = torch.full((n * W,), -3, dtype=torch.int32, device=DEV)
    tok = torch.full((n * W,), -3, dtype=torch.int64, device=DEV)
    live = torch.full((n * W,), 9, dtype=torch.uint8, device=DEV)
    hidx = torch.full((1 + max(alpha, 0), n * W), -3, dtype=torch.int32, device=DEV)
    pr = up(np.asarray(pairs, np.int32))
    hl = None if hlens is None else torch.from_numpy(np.asarray(hlens, np.int32)).to(DEV)
    ops.rnnt_nsc_step(up(np.asarray(rec, np.float32)), up(np.asarray(pair_lp, np.float32)), hl, s, a, par, tok, live, hidx, pr,
                      V, T, N, alpha, t, v, p)
    torch.cuda.synchronize()
    return (dict(zip(_ST, (x.cpu().numpy() for x in s))), dict(zip(_SK, (x.cpu().numpy() for x in a))), par.cpu().numpy(),
            tok.cpu().numpy(), live.cpu().numpy(), hidx.cpu().numpy(), pr.cpu().numpy())


def _close(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):                    # inf - inf
        return bool(np.all((got == want) | (np.abs(got - want) <= 1e-12 * np.maximum(np.abs(got), np.abs(want)))
                           | (np.isnan(got) & np.isnan(want))))


def _check_step(rec, pair_lp, hlens, st, S, pairs, V, T, N, alpha, t, v, p, stats=None):
    rec, pair_lp = np.asarray(rec, np.float32), np.asarray(pair_lp, np.float32)
    want = nsc_step64(rec, pair_lp, hlens, st, S, pairs, V, T, N, alpha, t, v, p, stats)
    got = _run_step(rec, pair_lp, hlens, st, S, pairs, V, T, N, alpha, t, v, p)
    (ws, wS, wpar, wtok, wlive, whidx, wpairs), (gs, gS, gpar, gtok, glive, ghidx, gpairs) = want, got
    what = (st["score"].shape[1:], V, N, alpha, t, v, p)
    assert gpar.tolist() == wpar.tolist() and gtok.tolist() == wtok.tolist() and glive.tolist() == wlive.tolist(), what
    assert ghidx.tolist() == whidx.tolist() and gpairs.tolist() == wpairs.tolist(), what
    for key in ("ulen", "count", "yseq"):
        assert np.array_equal(gs[key], ws[key]), (what, key)
    assert np.array_equal(gS["src"], wS["src"]) and np.array_equal(gS["nS"], wS["nS"]), what
    assert _close(gs["score"], ws["score"]) and _close(gS["score"], wS["score"]), (what, gs["score"], ws["score"])
    return want


def _sentinels(n, W, T, N, alpha):
    """blocks, S and a pair list that hold nothing yet: what a call does not write must still be there afterwards"""
    st, S, pairs = new_state(n, W, T, N), new_s(n, W, N), new_pairs(n, W, alpha)
    st["score"][:], st["ulen"][:], st["count"][:], st["yseq"][:] = 7.0, -3, -3, -3
    S["score"][:], S["src"][:], S["nS"][:] = 7.0, -3, -3
    pairs[:] = -5
    return st, S, pairs


def _kept(n, W, T, N, alpha, p, hyps):
    """hyps: per utterance [(score, labels)] -> sentinel blocks with kept's parity p filled"""
    st, S, pairs = _sentinels(n, W, T, N, alpha)
    blk = kept_block(N, p)
    for b, hb in enumerate(hyps):
        st["count"][blk, b] = len(hb)
        for w, (s, y) in enumerate(hb):
            st["score"][blk, b, w], st["ulen"][blk, b, w] = s, len(y) - 1
            st["yseq"][blk, b, w, :len(y)] = y
    return st, S, pairs


def _rec(k, rows, n_rows):
    """rows: {row: (blank logp, [(logp, token)] * k)}; other rows: -20 everywhere, tokens 1 .. k"""
    rec = np.full((n_rows, 1 + 2 * k), -20.0, np.float32)
    rec[:, 1 + k:] = np.arange(1, k + 1)
    for r_, (bl, ext) in rows.items():
        rec[r_, 0] = bl
        rec[r_, 1:1 + k] = [lp for lp, _t in ext]
        rec[r_, 1 + k:] = [t for _lp, t in ext]
    return rec


def _random_kept(r, st, n, W, V, T, N, t, p, ties):
    """a kept as frame t can meet it in parity p: 1 .. W sequences of at most t N labels in 1 .. V - 1; where the length allows a slot
    is the previous slot's labels plus one or two (prefix terms of depth 1 and 2, and extensions that substract removes) or the
    previous slot's labels again (the reference does not merge); with `ties` scores on a grid of 1 / 4"""
    blk = kept_block(N, p)
    val = (lambda: -float(r.integers(1, 12)) / 4.0) if ties else (lambda: -float(r.random()) * 4.0 - 0.01)
    for b in range(n):
        seqs = []
        for _try in range(W):
            y = [0] + [int(x) for x in r.integers(1, V, int(r.integers(0, t * N + 1)))]
            u = r.random()
            if seqs and u < 0.6:
                y = seqs[-1] + [int(x) for x in r.integers(1, V, 1 if u < 0.35 else 2)]
                y = y if len(y) - 1 <= t * N else seqs[-1][:]
            elif seqs and u < 0.7:
                y = seqs[-1][:]
            seqs.append(y)
        seqs = [seqs[i] for i in r.permutation(len(seqs))]
        seqs = seqs[:max(1, int(r.integers(1, W + 1)))] if r.random() < 0.5 else seqs
        st["count"][blk, b] = len(seqs)
        for w, y in enumerate(seqs):
            st["score"][blk, b, w], st["ulen"][blk, b, w] = val(), len(y) - 1
            st["yseq"][blk, b, w, :len(y)] = y


def _random_rec(r, st, n, W, V, cin, ties):
    """k distinct tokens per row; a row whose labels plus one token are another slot's labels proposes that token first"""
    k = min(W, V - 1)
    rec = np.zeros((n * W, 1 + 2 * k), np.float32)
    for row in range(n * W):
        rec[row, :1 + k] = -r.integers(1, 12, 1 + k) / 4.0 if ties else -r.random(1 + k) * 4.0 - 0.01
        rec[row, 1:1 + k] = -np.sort(-rec[row, 1:1 + k])
        toks = r.permutation(np.arange(1, V))[:k]
        b, w = divmod(row, W)
        for o in range(max(0, int(st["count"][cin, b]))):
            if st["ulen"][cin, b, o] == st["ulen"][cin, b, w] + 1 and w < st["count"][cin, b]:
                nxt = int(st["yseq"][cin, b, o, st["ulen"][cin, b, o]])
                if 1 <= nxt < V:
                    toks[toks == nxt] = toks[0]
                    toks[0] = nxt
        rec[row, 1 + k:] = toks
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("n,W,V", [(n, W, V) for n in (1, 5) for W in (1, 3, 16) for V in (6, 40) if W <= V])
def test_nsc_step_vs_restatement(n, W, V):
    """N = 1 .. 4, every call of random frames: a random kept in a random parity, the calls before v run by the restatement (so that
    S and the V blocks are what call v can meet), ragged hlens with finished utterances beside live ones and hlens NULL, with and
    without score ties, prefix_alpha 0 .. 3; blocks, S, the pair list and the per-row outputs start as sentinels"""
    T = 5
    r = np.random.default_rng(1000 * n + 10 * W + V)
    stats = {}
    for N in (1, 2, 3, 4):
        for trial in range(4):
            t, p, ties, alpha = int(r.integers(0, T)), int(r.integers(0, 2)), bool(trial & 1), (trial + N) % 4
            hlens = None if trial == 0 else r.choice([0, 1, 2, T - 1, T], n).astype(np.int32)
            if trial == 1 and n == 5:
                hlens = np.array([t, t + 1, T, 0, T + 3], np.int32)     # finished, on its last frame, live, empty, beyond T
            st, S, pairs = _sentinels(n, W, T, N, alpha)
            _random_kept(r, st, n, W, V, T, N, t, p, ties)
            pair_lp = (-r.integers(1, 12, len(pairs)) / 4.0 if ties else -r.random(len(pairs)) * 4.0 - 0.01).astype(np.float32)
            for v in range(1 if N == 1 else N + 1):
                cin = kept_block(N, p) if v == 0 else v
                st, S, _par, _tok, _live, _hidx, pairs = _check_step(_random_rec(r, st, n, W, V, cin, ties), pair_lp, hlens, st, S,
                                                                     pairs, V, T, N, alpha, t, v, p, stats)
    print("[parity] nsc step n=%d W=%d V=%d: prefix terms %s, %d substracted, %d short V, %d duplicates in kept over 52 calls"
          % (n, W, V, [stats.get("prefix%d" % a, 0) for a in (1, 2, 3)], stats.get("substracted", 0), stats.get("short_v", 0),
             stats.get("dup_kept", 0)))


@pytest.mark.gpu
def test_nsc_step_prefix_rescoring():
    """[0, a, b], [0, a], [0] in both orders of kept: prefix_alpha 1 (two terms of depth 1), 2 (slot [0, a, b] gains two contributions
    in ascending i, each from the un-updated scores), 3 (as 2) and 0 (nothing changes)"""
    la = lambda *v: float(functools.reduce(np.logaddexp, v))      # noqa: E731
    n, W, V, T, N, t = 1, 3, 6, 4, 1, 2
    hy = [(-1.0, [0, 1, 2]), (-2.0, [0, 1]), (-3.0, [0])]
    rec = _rec(3, {0: (-0.5, [(-9.0, 3), (-9.5, 4), (-10.0, 5)]), 1: (-0.5, [(-9.0, 3), (-9.5, 4), (-10.0, 5)]),
                   2: (-0.5, [(-9.0, 3), (-9.5, 4), (-10.0, 5)])}, 3)
    for alpha in (1, 2, 3, 0):
        for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
            st, S, pairs = _kept(n, W, T, N, alpha, 0, [[hy[i] for i in order]])
            pl = np.full((3, max(alpha, 1)), 9.0, np.float32)       # (slot, depth - 1); unused entries would show
            if alpha:
                pl[order.index(0), :min(alpha, 2)] = [-0.5, -0.25][:min(alpha, 2)]
                pl[order.index(1), 0] = -0.125
            stats = {}
            _st, S1, *_ = _check_step(rec, pl.reshape(-1)[:max(1, 3 * alpha)], None, st, S, pairs, V, T, N, alpha, t, 0, 0, stats)
            a = la(-1.0, -2.0 + -0.5, (-3.0 + -0.25) + -0.5) if alpha >= 2 else la(-1.0, -2.0 + -0.5) if alpha else -1.0
            b = la(-2.0, -3.0 + -0.125) if alpha else -2.0
            assert S1["score"][0, :3].tolist() == [a - 0.5, b - 0.5, -3.5] and S1["nS"].tolist() == [3]
            assert S1["src"][0, :3].tolist() == [order.index(0), order.index(1), order.index(2)]
            assert [stats.get("prefix%d" % d, 0) for d in (1, 2, 3)] == [[0, 0, 0], [2, 0, 0], [2, 1, 0], [2, 1, 0]][alpha]


@pytest.mark.gpu
def test_nsc_step_crafted_cases():
    # hypotheses of equal length keep kept's order, at equal scores everywhere: S before V, hyps' order, the record's order decide
    n, W, V, T = 1, 3, 6, 4
    st, S, pairs = _kept(n, W, T, 1, 1, 1, [[(-1.0, [0, 3]), (-1.0, [0, 1]), (-1.0, [0, 2])]])
    same = {r_: (-1.0, [(-1.0, 5), (-1.0, 4), (-1.0, 1)]) for r_ in range(3)}
    s1, S1, par, tok, live, _h, p1 = _check_step(_rec(3, same, 3), np.zeros(3), None, st, S, pairs, V, T, 1, 1, 1, 0, 1)
    assert S1["src"][0].tolist() == [6, 7, 8] and par.tolist() == [6, 7, 8] and live.tolist() == [0, 0, 0]
    st, S, pairs = _kept(n, W, T, 1, 1, 1, [[(-1.0, [0, 3]), (-1.0, [0, 1]), (-1.0, [0, 2, 2])]])
    same = {r_: (-3.0, [(-1.0, 5), (-1.0, 4), (-1.0, 1)]) for r_ in range(3)}
    s1, S1, par, tok, live, _h, p1 = _check_step(_rec(3, same, 3), np.zeros(3), None, st, S, pairs, V, T, 1, 1, 1, 0, 1)
    assert S1["src"][0].tolist() == [8, 6, 7] and par.tolist() == [8, 8, 8] and tok.tolist() == [5, 4, 1] and live.tolist() == [1, 1, 1]
    assert p1.tolist() == [[3, 5], [4, 4], [5, 1]] and s1["yseq"][0, 0, 2, :4].tolist() == [0, 2, 2, 1]
    # two equal sequences in kept: not prefixes of each other; [0] + 1 equals either and is removed, both gain [0]'s term
    stats = {}
    st, S, pairs = _kept(n, W, T, 2, 2, 0, [[(-1.0, [0, 1]), (-1.5, [0, 1]), (-2.0, [0])]])
    rec = _rec(3, {0: (-0.5, [(-0.25, 2), (-3.0, 3), (-4.0, 4)]), 1: (-0.5, [(-0.25, 2), (-3.0, 3), (-4.0, 4)]),
                   2: (-0.5, [(-0.125, 1), (-3.0, 3), (-4.0, 4)])}, 3)
    s1, S1, par, tok, live, *_ = _check_step(rec, -np.ones(6), None, st, S, pairs, V, T, 2, 2, 1, 0, 0, stats)
    assert stats == dict(prefix1=2, substracted=1, sort_gap=stats["sort_gap"]) and par.tolist() == [0, 1, 0] and tok.tolist() == [2, 2, 3]
    # substract leaves fewer than W: V = 2, [0] + 1 is a member of hyps, so V holds [0, 1, 1] alone; then nstep 2's finishing call
    stats = {}
    st, S, pairs = _kept(n, 2, T, 2, 1, 0, [[(-1.0, [0]), (-2.0, [0, 1])]])
    s1, S1, par, tok, live, *_ = _check_step(_rec(1, {0: (-0.5, [(-0.5, 1)]), 1: (-0.5, [(-0.25, 1)])}, 2), -np.ones(2), None, st, S, pairs,
                                             2, T, 2, 1, 1, 0, 0, stats)
    assert stats["substracted"] == 1 and stats["short_v"] == 1 and s1["count"][1, 0] == 1 and par.tolist() == [1, 1]
    assert live.tolist() == [1, 0] and s1["yseq"][1, 0, 0, :4].tolist() == [0, 1, 1, -3] and s1["score"][1, 0, 1] == 7.0
    # NaN sorts as -inf, +inf first: count < W, the third row points at itself and its block row is untouched
    st, S, pairs = _kept(n, W, T, 1, 0, 0, [[(-1.0, [0, 1]), (float("nan"), [0, 2])]])
    rec = _rec(3, {0: (float("inf"), [(-1.0, 3), (float("nan"), 4), (-2.0, 5)]), 1: (-1.0, [(-1.0, 3), (-1.0, 4), (-1.0, 5)])}, 3)
    s1, S1, par, tok, live, *_ = _check_step(rec, np.zeros(1), None, st, S, pairs, V, T, 1, 0, 1, 0, 0)
    assert par.tolist() == [0, 0, 0] and tok.tolist() == [0, 3, 5] and s1["count"][2, 0] == 3
    st, S, pairs = _kept(n, W, T, 1, 0, 0, [[(-1.0, [0])]])
    s1, S1, par, tok, live, *_ = _check_step(_rec(2, {0: (-9.0, [(-0.5, 2), (-0.5, 1)])}, 3), np.zeros(1), None, st, S, pairs, 3, T, 1,
                                             0, 0, 0, 0)
    assert s1["count"][2, 0] == 3 and par.tolist() == [0, 0, 0] and tok.tolist() == [2, 1, 0] and live.tolist() == [1, 1, 0]
    st, S, pairs = _kept(n, W, T, 2, 0, 0, [[(-1.0, [0])]])
    s1, S1, par, tok, live, *_ = _check_step(_rec(2, {0: (-9.0, [(-0.5, 2), (-0.5, 1)])}, 3), np.zeros(1), None, st, S, pairs, 3, T, 2,
                                             0, 0, 0, 0)
    assert s1["count"][1, 0] == 2 and par.tolist() == [0, 0, 2] and live.tolist() == [1, 1, 0]
    assert s1["score"][1, 0, 2] == 7.0 and s1["ulen"][1, 0, 2] == -3


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 4])
def test_nsc_step_frames_of_every_nstep(N):
    """two frames call by call: nstep 1 selects kept directly, without a blank term on V; nstep 2 and 4 add rec[r][0] to the last V in
    the finishing call"""
    n, W, V, T, alpha = 2, 3, 6, 3, 1
    r = np.random.default_rng(N)
    st, S, pairs = _sentinels(n, W, T, N, alpha)
    fresh = new_state(n, W, T, N)
    for key in _ST:
        st[key][0] = fresh[key][0]
    pairs[:] = new_pairs(n, W, alpha)
    p = 0
    for t in range(2):
        calls = 1 if N == 1 else N + 1
        recs = []
        for v in range(calls):
            rec = np.zeros((n * W, 7), np.float32)
            rec[:, :4] = -np.sort(r.random((n * W, 4)) * 3.0 + 0.01)
            rec[:, 0] = -r.random(n * W) - (8.0 if v == 0 else 0.01)      # the frame's first blank continuations lose
            rec[:, 4:] = np.stack([r.permutation(np.arange(1, V))[:3] for _ in range(n * W)])
            recs.append(rec)
        before = st
        out = None
        for v in range(calls):
            out = _check_step(recs[v], np.full(n * W, -0.5), None, st, S, pairs, V, T, N, alpha, t, v, p)
            if v == calls - 1 and N > 1:
                vb = st["score"][N, :, :] + recs[v][:, 0].reshape(n, W)
                best = np.where(np.arange(W)[None, :] < st["count"][N][:, None], vb, -np.inf).max(1)
                assert np.all(out[0]["score"][kept_block(N, 1 - p)].max(1) >= best - 1e-12)
            st, S, pairs = out[0], out[1], out[6]
        ko = kept_block(N, 1 - p)
        assert st["count"][ko].tolist() == [3, 3]
        if N == 1:
            assert out[4].reshape(n, W).sum() >= n            # the extensions beat the blank continuations: tokens appended
            b0 = kept_block(N, p) * n * W
            w0 = int(out[2][0]) - b0
            assert st["score"][ko, 0, 0] == before["score"][kept_block(N, p), 0, w0] + float(recs[0][w0, 1])
        p = 1 - p


@pytest.mark.gpu
def test_nsc_step_ragged_lengths():
    """one batch with hlens 0, 1, T and beyond T, at t below, at and past each length, both parities, nstep 1 and 3: a finished
    utterance is carried on the frame's last call and nothing else of it is written"""
    n, W, V, T, alpha = 4, 2, 5, 3, 2
    hlens = np.array([0, 1, T, T + 4], np.int32)
    r = np.random.default_rng(7)
    for N in (1, 3):
        for t in range(T + 1):
            for p in (0, 1):
                hy = [(-1.0, [0, 1]), (-2.0, [0])]
                st, S, pairs = _kept(n, W, T, N, alpha, p, [hy] * n)
                kp, ko = kept_block(N, p), kept_block(N, 1 - p)
                for v in range(1 if N == 1 else N + 1):
                    rec = _rec(2, {r_: (-float(r.integers(1, 9)) / 4, [(-0.25, 2), (-0.75, 1)]) for r_ in range(n * W)}, n * W)
                    st1, S1, par, tok, live, hidx, pairs1 = _check_step(rec, -np.ones(n * W * alpha), hlens, st, S, pairs, V, T, N,
                                                                        alpha, t, v, p)
                    last = N == 1 or v == N
                    for b in range(n):
                        idle = t >= min(int(hlens[b]), T)
                        rows = slice(b * W, (b + 1) * W)
                        if idle:
                            assert par[rows].tolist() == [kp * n * W + b * W, kp * n * W + b * W + 1] and not live[rows].any()
                            assert S1["nS"][b] == -3 and np.all(pairs1[b * W * alpha:(b + 1) * W * alpha] == -5)
                            assert (st1["count"][ko, b] == 2) == last and all(st1["count"][q, b] == -3 for q in range(1, N + 1))
                            if last:
                                assert st1["score"][ko, b].tolist() == [-1.0, -2.0] and st1["ulen"][ko, b].tolist() == [1, 0]
                        else:
                            assert S1["nS"][b] > 0 and (st1["count"][ko, b] > 0) == last
                    st, S, pairs = st1, S1, pairs1


@pytest.mark.gpu
def test_nsc_step_never_writes_past_a_full_label_row():
    """a kept whose label rows are full (ulen = ycap - 1: no search reaches it, a frame appends at most N labels): the extension keeps
    the parent's labels, its length stays ycap - 1, and the rows behind it keep their sentinels"""
    n, W, V, T, N, alpha = 1, 2, 4, 2, 1, 1
    ycap = 1 + T * N
    st, S, pairs = _kept(n, W, T, N, alpha, 0, [[(-1.0, [0, 1, 2]), (-1.5, [0, 2, 3])]])
    rec = _rec(2, {0: (-9.0, [(-0.5, 3), (-0.75, 1)]), 1: (-9.0, [(-2.0, 1), (-3.0, 2)])}, 2)
    s1, S1, par, tok, live, hidx, p1 = _run_step(rec, np.zeros(2, np.float32), None, st, S, pairs, V, T, N, alpha, 1, 0, 0)
    assert s1["count"][2, 0] == 2 and par.tolist() == [0, 0] and tok.tolist() == [3, 1] and live.tolist() == [1, 1]
    assert s1["ulen"][2, 0].tolist() == [ycap - 1, ycap - 1] and s1["yseq"][2, 0].tolist() == [[0, 1, 2], [0, 1, 2]]
    assert np.all(s1["yseq"][1] == -3) and np.array_equal(s1["yseq"][0], st["yseq"][0])
    assert S1["nS"].tolist() == [2] and S1["src"][0].tolist() == [0, 1]


@pytest.mark.gpu
def test_nsc_step_limits():
    """more than 16 slots, nstep 5, prefix_alpha 4, more slots than tokens: refused, nothing launched, outputs untouched"""
    from espnet_amd import _lib
    T, n = 4, 1
    for W, V, N, alpha in ((17, 40, 2, 1), (4, 40, 5, 1), (4, 40, 2, 4), (7, 6, 2, 1)):
        st, S, pairs = _sentinels(n, W, T, N, alpha)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
        from espnet_amd import ops
        s, a = tuple(up(st[key]) for key in _ST), tuple(up(S[key]) for key in _SK)
        outs = [torch.full((n * W,), -3, dtype=torch.int32, device=DEV), torch.full((n * W,), -3, dtype=torch.int64, device=DEV),
                torch.full((n * W,), 9, dtype=torch.uint8, device=DEV), torch.full((1 + alpha, n * W), -3, dtype=torch.int32, device=DEV),
                up(pairs)]
        with pytest.raises(_lib.EamdError):
            ops.rnnt_nsc_step(torch.zeros(n * W, 1 + 2 * min(W, V - 1), device=DEV), torch.zeros(len(pairs), device=DEV), None, s, a,
                              *outs, V, T, N, alpha, 0, 0, 0)
        torch.cuda.synchronize()
        for x, key in zip(s, _ST):
            assert np.array_equal(x.cpu().numpy(), st[key]), (W, V, N, alpha, key)
        for x, key in zip(a, _SK):
            assert np.array_equal(x.cpu().numpy(), S[key]), (W, V, N, alpha, key)
        assert all(bool((o == c).all()) for o, c in zip(outs[:4], (-3, -3, 9, -3))) and bool((outs[4] == -5).all())


# ---- 2. search vs float64 ----------------------------------------------------------------------------------------------------
T_S, E_S, D_S = 12, 6, 8
# (J, V, B, nstep, prefix_alpha, beam); the last shape has more slots than non-blank tokens (k < W: V lists shorter than W)
SEARCH_CASES = [(d, l, h) + shape for d, l, h in itertools.product(("lstm", "gru"), (1, 2), (12, 64))
                for shape in ((7, 6, 20, 1, 1, 3), (7, 6, 3, 2, 2, 2), (52, 257, 3, 2, 1, 8), (52, 257, 2, 3, 3, 16), (52, 257, 8, 1, 2, 4),
                              (7, 6, 3, 2, 1, 8))]


def search_case(dtype, L, H, J, V, B, N, alpha, beam, seed):
    sd = seeded_weights(seed, dtype, L, H, E_S, J, V, D_S, {6: 2.0}.get(V, 4.0))
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((B, T_S, D_S)).astype(np.float32)
    hlens = r.integers(T_S // 2, T_S + 1, B)
    hlens[0], hlens[1] = T_S, 1
    if B > 2:
        hlens[2] = 2
    return sd, hs, hlens


@functools.lru_cache(maxsize=None)
def search_reference(dtype, L, H, J, V, B, N, alpha, beam, seed):
    sd, hs, hlens = search_case(dtype, L, H, J, V, B, N, alpha, beam, seed)
    return nsc_batch64(weights_from_state_dict(sd), hs, hlens, beam, N, alpha)


@functools.lru_cache(maxsize=None)
def search_seed(dtype, L, H, J, V, B, N, alpha, beam):
    base = 31 * H + 7 * J + V + 1000 * L + 100000 * (dtype == "gru") + 17 * B + 3 * N + 1009 * beam + 53 * alpha
    for i in range(256):
        if search_reference(dtype, L, H, J, V, B, N, alpha, beam, base + 104729 * i)["min_gap"] >= GAP:
            return base + 104729 * i
    raise AssertionError("no seed meets the preconditions")


def _decoder(sd, dtype, L, H, E, J, V, D_enc, act="tanh"):
    from espnet_amd.nets.transducer.rnn_decoder import DecoderRNNT
    dec = DecoderRNNT(D_enc, V, dtype, L, H, 0, E, J, act)
    dec.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in sd.items()})
    return dec.to(DEV).eval()


def _same_nbest(got, want, what):
    """got: [Hypothesis], want: [(score, labels)]"""
    assert len(got) == len(want), (what, len(got), len(want))
    worst = 0.0
    for j, (h, (s, y)) in enumerate(zip(got, want)):
        assert list(h.yseq) == [int(v) for v in y], (what, j, h.yseq, y)
        err = abs(h.score - float(s)) / max(1.0, abs(float(s)))
        worst = max(worst, err)
        assert err <= 1e-4, (what, j, h.score, s)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,L,H,J,V,B,N,alpha,beam", SEARCH_CASES)
def test_nsc_batch_vs_float64(dtype, L, H, J, V, B, N, alpha, beam):
    """nsc_batch on a seeded DecoderRNNT with ragged lengths (T, 1 and 2 among them) against the whole-search restatement: the same
    n-best lists in the same order, scores within 1e-4 relative; gap precondition asserted"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    case = (dtype, L, H, J, V, B, N, alpha, beam)
    seed = search_seed(*case)
    ref = search_reference(*case, seed)
    assert ref["min_gap"] >= GAP, ("precondition: float64 decision gap", ref["min_gap"])
    sd, hs, hlens = search_case(*case, seed)
    bs = BeamSearchTransducer(decoder=_decoder(sd, dtype, L, H, E_S, J, V, D_S), beam_size=beam, search_type="nsc", nstep=N,
                              prefix_alpha=alpha)
    got = bs.nsc_batch(torch.from_numpy(hs).to(DEV), [int(v) for v in hlens])
    assert len(got) == B
    worst = max(_same_nbest(g, w, (case, b)) for b, (g, w) in enumerate(zip(got, ref["nbest"])))
    print("[parity] nsc_batch %s x%d H=%d J=%d V=%d B=%d N=%d alpha=%d beam=%d: prefix terms %s, %d substracted, %d short V, "
          "%d duplicates in kept, %d labels, min gap %.1e, score rel err %.2e"
          % (case + (ref["prefix"], ref["substracted"], ref["short_v"], ref["dup_kept"], ref["labels"], ref["min_gap"], worst)))


@pytest.mark.gpu
@pytest.mark.parametrize("N,alpha", [(1, 1), (2, 0)])
def test_nsc_batch_utterance_without_frames(N, alpha):
    """hlens 0 beside a live utterance: [blank] with score 0, as list and as device tensor; the live one is what it is alone"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    sd = seeded_weights(9, "gru", 1, 12, E_S, 7, 6, D_S, 2.0)
    bs = BeamSearchTransducer(decoder=_decoder(sd, "gru", 1, 12, E_S, 7, 6, D_S), beam_size=3, search_type="nsc", nstep=N,
                              prefix_alpha=alpha)
    hs = torch.randn(2, 5, D_S, generator=torch.Generator().manual_seed(3)).to(DEV)
    alone = bs.nsc_batch(hs[1:], [4])[0]
    for hlens in ([0, 4], torch.tensor([0, 4]).to(DEV)):
        got = bs.nsc_batch(hs, hlens)
        assert [(h.score, h.yseq) for h in got[0]] == [(0.0, [0])]
        _same_nbest(got[1], [(h.score, h.yseq) for h in alone], (N, alpha))    # other row counts in the GEMMs: other roundings


# ---- 3. fixtures -------------------------------------------------------------------------------------------------------------
_FIX = [("nsc3", dict(beam_size=3, search_type="nsc", nstep=1, prefix_alpha=1)),
        ("nsc3n2", dict(beam_size=3, search_type="nsc", nstep=2, prefix_alpha=2)),
        ("nsc2n3", dict(beam_size=2, search_type="nsc", nstep=3, prefix_alpha=1, score_norm=False))]


def _same_lists(got, want, what):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        _same_nbest(g, [(h.score, h.yseq) for h in w], (what, b))


@pytest.mark.gpu
@pytest.mark.parametrize("tag,kw", _FIX, ids=[c[0] for c in _FIX])
@pytest.mark.parametrize("name", ["transducer_rnn.npz", "transducer_gru.npz"])
def test_nsc_batch_vs_per_utterance_search_and_reference(name, tag, kw):
    """the fixture's three utterances with their valid lengths: nsc_batch (hlens as list, device tensor, None) and recognize_batch
    equal the per-utterance search element by element; utterance 0 equals the n-best list the reference recorded"""
    from test_gpu_rnnt_greedy import _golden_model, _valid_lengths
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer, Hypothesis
    p, m = _golden_model(name)
    search = BeamSearchTransducer(decoder=m.dec, **kw)
    hs_pad = m.hs_pad.detach()
    hlens = _valid_lengths(m, p)
    assert max(hlens) == hs_pad.shape[1] and min(hlens) < max(hlens)
    one = [search(hs_pad[b, : hlens[b]]) for b in range(len(hlens))]
    got = search.nsc_batch(hs_pad, hlens)
    _same_lists(got, one, "ragged")
    _same_lists(search.nsc_batch(hs_pad, torch.tensor(hlens).to(DEV)), one, "tensor hlens")
    _same_lists(search.nsc_batch(hs_pad), [search(hs_pad[b]) for b in range(len(hlens))], "hlens=None: whole padded rows")
    # utterance 0 against the reference's record
    lens, want, flat = (p["dec_%s_%s" % (tag, key)].tolist() for key in ("lens", "scores", "yseq"))
    ref, o = [], 0
    for ln, sc in zip(lens, want):
        ref.append((sc, flat[o:o + ln]))
        o += ln
    _same_nbest(got[0], ref, "reference record")
    xs = [p["xs"][b, : int(p["ilens"][b])].numpy() for b in range(3)]
    nb = m.recognize_batch(xs, search)
    _same_lists([[Hypothesis(score=h["score"], yseq=h["yseq"]) for h in r] for r in nb], one, "recognize_batch")
    assert [h["yseq"] for h in nb[0]] == [h["yseq"] for h in m.recognize(xs[0], search)]


def _fallback_case(name, kw):
    from test_gpu_rnnt_greedy import _golden_model, _valid_lengths
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    p, m = _golden_model(name)
    search = BeamSearchTransducer(decoder=m.decoder if hasattr(m, "decoder") else m.dec, **kw)
    hs_pad = m.hs_pad.detach()
    hlens = _valid_lengths(m, p)
    calls = [0]
    inner = search._nsc

    def counted(h):
        calls[0] += 1
        return inner(h)
    search._nsc = counted
    got = search.nsc_batch(hs_pad, hlens)
    assert calls[0] == len(hlens)                          # the per-utterance search ran, once per utterance
    one = [search(hs_pad[b, : hlens[b]]) for b in range(len(hlens))]
    assert [[h.yseq for h in g] for g in got] == [[h.yseq for h in g] for g in one]
    assert [[h.score for h in g] for g in got] == [[h.score for h in g] for g in one]


@pytest.mark.gpu
def test_nsc_batch_fallbacks():
    """a custom prediction network, beam_size 17, nstep 5 and an LM go through the per-utterance loop and return what it returns"""
    from espnet_amd.nets.lm import ClassifierWithState, RNNLM
    from conftest import load_golden, split_golden
    _fallback_case("transducer_tt.npz", dict(beam_size=3, search_type="nsc", nstep=2, prefix_alpha=1))
    _fallback_case("transducer_rnn.npz", dict(beam_size=17, search_type="nsc", nstep=2))
    _fallback_case("transducer_rnn.npz", dict(beam_size=3, search_type="nsc", nstep=5))
    p, _sd, _ = split_golden(load_golden("transducer_rnn.npz"))
    lm = ClassifierWithState(RNNLM(6, 1, 8, None, "lstm", 0.0))
    lm.load_state_dict({k[3:]: v for k, v in p.items() if k.startswith("lm/")})
    _fallback_case("transducer_rnn.npz", dict(beam_size=3, search_type="nsc", nstep=2, lm_weight=0.5, lm=lm.to(DEV).eval()))


# ---- 4. one host read --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,rows", [(3, 256), (7, 12)])
def test_nsc_batch_reads_the_host_once(B, rows, monkeypatch):
    """blocking device-to-host reads counted as test_tsd_batch_reads_the_host_once counts them: exactly one per call for hlens
    None / list / device tensor, also when the batch goes in chunks (7 utterances x 4 slots in chunks of 12 rows: 3 + 3 + 1)"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    T = 12
    sd = seeded_weights(5, "lstm", 1, 64, E_S, 52, 257, D_S, 4.0)
    kw = dict(beam_size=4, search_type="nsc", nstep=2, prefix_alpha=1)
    bs = BeamSearchTransducer(decoder=_decoder(sd, "lstm", 1, 64, E_S, 52, 257, D_S), **kw)
    bs.nsc_max_rows = rows
    hs = torch.randn(B, T, D_S, generator=torch.Generator().manual_seed(B)).to(DEV)
    hl = torch.full((B,), T, dtype=torch.int32).to(DEV)
    whole = BeamSearchTransducer(decoder=bs.decoder, **kw).nsc_batch(hs)
    reads = [0]
    for meth in ("tolist", "item", "cpu", "numpy"):
        orig = getattr(torch.Tensor, meth)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                reads[0] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, meth, counted)
    counts, results = [], []
    for hlens in (None, [T] * B, hl):
        reads[0] = 0
        results.append(bs.nsc_batch(hs, hlens))
        counts.append(reads[0])
    monkeypatch.undo()
    assert counts == [1, 1, 1], counts
    for got in results:                                    # chunks change the GEMMs' row counts, hence roundings, nothing else
        _same_lists(got, whole, "chunks of %d rows" % rows)
