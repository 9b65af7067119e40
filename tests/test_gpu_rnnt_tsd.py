"""Batched time-synchronous transducer beam search on the GPU: eamd_rnnt_tsd_step (csrc/rnnt_tsd.hip) and
BeamSearchTransducer.tsd_batch / E2E.recognize_batch against
  * tests/tsd_restatement.py - float64, pinned to a plain per-utterance statement by tests/test_tsd_restatement.py,
  * the per-utterance tsd search of the same package, and
  * the tsd n-best lists the reference recorded in tests/golden/transducer_rnn.npz / transducer_gru.npz.
Kernel: par, tok, live, lengths, labels, counts, a_src and nA exact - whole arrays, so what the kernel must not write shows as
well; scores within 1e-12 relative (float64 sums and the roundings of logaddexp, the bound of tests/test_gpu_rnnt_alsd.py for the
same arithmetic).  Search: same n-best length, same sequences in the same order, scores within 1e-4 relative (the bound of
tests/test_gpu_transducer_search.py).  Equal sequences are meaningful where float32 cannot flip an ordering decision, so every
float64 decision gap that is used (top-k boundary of a live row of C on a pass v < M - 1, adjacent scores of sorted D and sorted A
down to position W + 1, adjacent keys of the final sort) must be >= 1e-4; this precondition is ASSERTED, and each case takes the
first seed of its own sequence that meets it on the CPU (tests/test_tsd_restatement.py checks that every case finds one; the choice
never looks at a GPU result)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from rnnt_greedy_restatement import seeded_weights, weights_from_state_dict
from tsd_restatement import b_block, new_a, new_state, tsd_batch64, tsd_step64

DEV = "cuda"
GAP = 1e-4


@pytest.fixture(autouse=True)
def _fp32():
    import espnet_amd
    espnet_amd.set_precision("fp32")
    yield
    espnet_amd.set_precision("fp32")


# ---- 1. the pass kernel vs the one-pass restatement ---------------------------------------------------------------------------
_ST, _AK = ("score", "ulen", "count", "yseq"), ("score", "src", "nA")


def _run_step(rec, hlens, st, A, V, T, M, t, v, p):
    """eamd_rnnt_tsd_step on numpy operands -> (blocks, A, par, tok, live) as numpy; par / tok / live start as sentinels"""
    from espnet_amd import ops
    _blocks, n, W = st["score"].shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    s, a = tuple(up(st[key]) for key in _ST), tuple(up(A[key]) for key in _AK)
    par = torch.full((n * W,), -3, dtype=torch.int32, device=DEV)
    tok = torch.full((n * W,), -3, dtype=torch.int64, device=DEV)
    live = torch.full((n * W,), 9, dtype=torch.uint8, device=DEV)
    hl = None if hlens is None else torch.from_numpy(np.asarray(hlens, np.int32)).to(DEV)
    ops.rnnt_tsd_step(up(np.asarray(rec, np.float32)), hl, s, a, par, tok, live, V, T, M, t, v, p)
    torch.cuda.synchronize()
    return (dict(zip(_ST, (x.cpu().numpy() for x in s))), dict(zip(_AK, (x.cpu().numpy() for x in a))), par.cpu().numpy(),
            tok.cpu().numpy(), live.cpu().numpy())


def _close(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):                    # inf - inf
        return bool(np.all((got == want) | (np.abs(got - want) <= 1e-12 * np.maximum(np.abs(got), np.abs(want)))
                           | (np.isnan(got) & np.isnan(want))))


def _check_step(rec, hlens, st, A, V, T, M, t, v, p, stats=None):
    rec = np.asarray(rec, np.float32)
    want = tsd_step64(rec, hlens, st, A, V, T, M, t, v, p, stats)
    got = _run_step(rec, hlens, st, A, V, T, M, t, v, p)
    (ws, wa, wpar, wtok, wlive), (gs, ga, gpar, gtok, glive) = want, got
    what = (st["score"].shape[1:], V, M, t, v, p)
    assert gpar.tolist() == wpar.tolist() and gtok.tolist() == wtok.tolist() and glive.tolist() == wlive.tolist(), what
    for key in ("ulen", "count", "yseq"):
        assert np.array_equal(gs[key], ws[key]), (what, key)
    assert np.array_equal(ga["src"], wa["src"]) and np.array_equal(ga["nA"], wa["nA"]), what
    assert _close(gs["score"], ws["score"]) and _close(ga["score"], wa["score"]), (what, gs["score"], ws["score"])
    return want


def _sentinels(n, W, T, M):
    """blocks and A that hold nothing yet: what a pass does not write must still be there afterwards"""
    st, A = new_state(n, W, T, M), new_a(n, W, M)
    st["score"][:], st["ulen"][:], st["count"][:], st["yseq"][:] = 7.0, -3, -3, -3
    A["score"][:], A["src"][:], A["nA"][:] = 7.0, -3, -3
    return st, A


def _random_b(r, st, n, W, V, T, M, t, p, ties):
    """a B as frame t can meet it in parity p: 1 .. W pairwise distinct sequences of at most t (M - 1) labels in 1 .. V - 1, every
    other one the previous slot's labels plus one where the length allows (so that an extension of one slot is another slot's
    sequence and merges happen); with `ties` scores on a grid of 1 / 4"""
    blk = b_block(M, p)
    val = (lambda: -float(r.integers(1, 12)) / 4.0) if ties else (lambda: -float(r.random()) * 4.0 - 0.01)
    for b in range(n):
        seqs = []
        for _try in range(4 * W):
            if len(seqs) == W:
                break
            y = [0] + [int(x) for x in r.integers(1, V, int(r.integers(0, t * (M - 1) + 1)))]
            if seqs and r.random() < 0.5 and len(seqs[-1]) - 1 < t * (M - 1):
                y = seqs[-1] + [int(r.integers(1, V))]
            if y not in seqs:
                seqs.append(y)
        seqs = seqs[:max(1, int(r.integers(1, W + 1)))] if r.random() < 0.5 else seqs
        st["count"][blk, b] = len(seqs)
        for w, y in enumerate(seqs):
            st["score"][blk, b, w], st["ulen"][blk, b, w] = val(), len(y) - 1
            st["yseq"][blk, b, w, :len(y)] = y


def _random_rec(r, st, n, W, V, cin, ties):
    """k distinct tokens per row; a row whose labels plus one token are the next slot's labels proposes that token first"""
    k = min(W, V - 1)
    rec = np.zeros((n * W, 1 + 2 * k), np.float32)
    for row in range(n * W):
        rec[row, :1 + k] = -r.integers(1, 12, 1 + k) / 4.0 if ties else -r.random(1 + k) * 4.0 - 0.01
        rec[row, 1:1 + k] = -np.sort(-rec[row, 1:1 + k])
        toks = r.permutation(np.arange(1, V))[:k]
        b, w = divmod(row, W)
        if w + 1 < W and st["ulen"][cin, b, w + 1] == st["ulen"][cin, b, w] + 1 and st["count"][cin, b] > w + 1:
            nxt = int(st["yseq"][cin, b, w + 1, st["ulen"][cin, b, w + 1]])
            if 1 <= nxt < V:
                toks[toks == nxt] = toks[0]
                toks[0] = nxt
        rec[row, 1 + k:] = toks
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("n,W,V", [(n, W, V) for n in (1, 3) for W in (1, 2, 3, 8, 16) for V in (2, 3, 6, 40) if W <= V])
def test_tsd_step_vs_restatement(n, W, V):
    """M = 1 .. 4, every pass v < M of random frames: a random B in a random parity, the passes before v run by the restatement (so
    that A and the C blocks are what pass v can meet), ragged hlens with finished utterances beside live ones and hlens NULL, with
    and without score ties; blocks, A and the per-row outputs start as sentinels"""
    T = 5
    r = np.random.default_rng(1000 * n + 10 * W + V)
    stats = {}
    for M in (1, 2, 3, 4):
        for trial in range(4):
            t, p, ties = int(r.integers(0, T)), int(r.integers(0, 2)), bool(trial & 1)
            hlens = None if trial == 0 else r.choice([1, 2, T - 1, T], n).astype(np.int32)
            if trial == 1 and n == 3:
                hlens = np.array([t, t + 1, T], np.int32)          # finished, on its last frame, live
            st, A = _sentinels(n, W, T, M)
            _random_b(r, st, n, W, V, T, M, t, p, ties)
            for v in range(M):
                cin = b_block(M, p) if v == 0 else v
                st, A, *_ = _check_step(_random_rec(r, st, n, W, V, cin, ties), hlens, st, A, V, T, M, t, v, p, stats)
    print("[parity] tsd step n=%d W=%d V=%d: %d merges, %d truncated over 40 passes" % (n, W, V, stats.get("merges", 0),
                                                                                        stats.get("truncated", 0)))


def _blocks(n, W, T, M, p, hyps):
    """hyps: per utterance [(score, labels)] -> sentinel blocks with B's parity p filled"""
    st, A = _sentinels(n, W, T, M)
    blk = b_block(M, p)
    for b, hb in enumerate(hyps):
        st["count"][blk, b] = len(hb)
        for w, (s, y) in enumerate(hb):
            st["score"][blk, b, w], st["ulen"][blk, b, w] = s, len(y) - 1
            st["yseq"][blk, b, w, :len(y)] = y
    return st, A


def _rec(W, k, rows, n_rows):
    """rows: {row: (blank logp, [(logp, token)] * k)}; other rows: -20 everywhere, tokens 1 .. k"""
    rec = np.full((n_rows, 1 + 2 * k), -20.0, np.float32)
    rec[:, 1 + k:] = np.arange(1, k + 1)
    for r_, (bl, ext) in rows.items():
        rec[r_, 0] = bl
        rec[r_, 1:1 + k] = [lp for lp, _t in ext]
        rec[r_, 1 + k:] = [t for _lp, t in ext]
    return rec


@pytest.mark.gpu
def test_tsd_step_crafted_cases():
    la = lambda *v: float(functools.reduce(np.logaddexp, v))      # noqa: E731
    # W = 2, M = 2, frame 1 (the passes of tests/test_tsd_restatement.py): at the frame's end [0, 2] of C equals the A entry that
    # pass 0 added from B, and nA = 3 > W
    n, W, V, T, M, t = 1, 2, 4, 3, 2, 1
    st, A = _blocks(n, W, T, M, 0, [[(-1.0, [0, 2]), (-2.0, [0])]])
    st, A, par, tok, live = _check_step(np.array([[-0.5, -0.25, -4.0, 3, 1], [-0.25, -0.75, -3.0, 2, 1]]), None, st, A, V, T, M, t, 0, 0)
    assert A["nA"].tolist() == [2] and par.tolist() == [0, 1] and tok.tolist() == [3, 2] and live.tolist() == [1, 1]
    stats = {}
    st, A, par, tok, live = _check_step(np.array([[-0.125, -9, -9, 1, 2], [-0.25, -9, -9, 1, 2]]), None, st, A, V, T, M, t, 1, 0, stats)
    assert stats == dict(merges=1, truncated=1, sort_gap=stats["sort_gap"]) and A["nA"].tolist() == [3]
    assert st["score"][2, 0].tolist() == [la(-1.5, -3.0), -1.375] and par.tolist() == [0, 2] and live.tolist() == [0, 0]
    assert st["yseq"][2, 0].tolist() == [[0, 2, -3, -3], [0, 2, 3, -3]] and st["count"][:, 0].tolist() == [2, 2, 2]
    # M = 3: [0, 1, 1] of B is reached again by [0, 1] + 1 on pass 1 and by [0] + 1 + 1 on pass 2: two merges into one entry
    n, W, V, T, M, t = 1, 3, 6, 3, 3, 1
    st, A = _blocks(n, W, T, M, 1, [[(-1.0, [0, 1, 1]), (-1.2, [0, 1]), (-1.5, [0])]])
    low = [(-7.0, 2), (-8.0, 3)]
    rec = _rec(W, 3, {0: (-0.5, [(-6.0, 1)] + low), 1: (-0.5, [(-0.25, 1)] + low), 2: (-0.5, [(-0.25, 1)] + low)}, 3)
    stats = {}
    st, A, par, tok, live = _check_step(rec, None, st, A, V, T, M, t, 0, 1, stats)
    assert par.tolist() == [10, 11, 9] and st["ulen"][1, 0].tolist() == [2, 1, 3] and "merges" not in stats
    rec = _rec(W, 3, {0: (-0.25, [(-5.0, 1)] + low), 1: (-0.25, [(-0.5, 1)] + low), 2: (-0.25, [(-1.0, 1)] + low)}, 3)
    st, A, par, tok, live = _check_step(rec, None, st, A, V, T, M, t, 1, 1, stats)
    assert stats["merges"] == 2 and A["nA"].tolist() == [4] and A["src"][0, :4].tolist() == [9, 10, 11, 5]
    assert A["score"][0, 0] == la(-1.5, -1.7) and st["yseq"][2, 0, 0, :3].tolist() == [0, 1, 1] and par[0] == 4
    rec = _rec(W, 3, {0: (-0.25, low + [(-9.0, 1)]), 1: (-0.25, low + [(-9.0, 1)]), 2: (-0.25, low + [(-9.0, 1)])}, 3)
    st, A, par, tok, live = _check_step(rec, None, st, A, V, T, M, t, 2, 1, stats)
    assert stats["merges"] == 4 and A["score"][0, 0] == la(la(-1.5, -1.7), -2.5) and A["nA"].tolist() == [5]
    assert par.tolist() == [9, 10, 11] and st["count"][0, 0] == 3 and live.tolist() == [0, 0, 0]
    # count < W: one hypothesis, V = 3, two extensions for three slots; the third row points at itself and its block row is untouched
    n, W, V, T, M = 1, 3, 3, 4, 2
    st, A = _blocks(n, W, T, M, 0, [[(-1.0, [0])]])
    st, A, par, tok, live = _check_step(_rec(W, 2, {0: (-0.5, [(-0.5, 2), (-0.5, 1)])}, 3), None, st, A, V, T, M, 0, 0, 0)
    assert st["count"][1, 0] == 2 and par.tolist() == [0, 0, 2] and tok.tolist() == [2, 1, 0] and live.tolist() == [1, 1, 0]
    assert st["score"][1, 0, 2] == 7.0 and st["ulen"][1, 0, 2] == -3
    # NaN sorts as -inf, +inf first
    st, A = _blocks(n, W, T, M, 0, [[(-1.0, [0, 1]), (float("nan"), [0, 2]), (float("inf"), [0])]])
    st, A, par, *_ = _check_step(_rec(W, 2, {}, 3), None, st, A, V, T, M, 1, 0, 0)
    assert par.tolist() == [2, 2, 0]
    # a finished utterance beside a live one, on both passes and in both parities; hlens NULL runs every utterance
    for p in (0, 1):
        hy = [(-1.0, [0, 1]), (-2.0, [0])]
        st, A = _blocks(2, W, T, M, p, [hy, hy])
        rec = _rec(W, 2, {r_: (-0.5, [(-0.25, 2), (-0.75, 1)]) for r_ in range(6)}, 6)
        b0 = b_block(M, p) * 6
        for hlens, idle in ((np.array([1, 4], np.int32), True), (None, False)):
            s1, A1, par, tok, live = _check_step(rec, hlens, st, A, V, T, M, 1, 0, p)
            assert (par[:3].tolist() == [b0, b0 + 1, b0 + 2] and not live[:3].any()) == idle and live[3:].all()
            assert (s1["count"][1, 0] == -3) == idle and (A1["nA"][0] == -3) == idle
            s2, A2, par, tok, live = _check_step(rec, hlens, s1, A1, V, T, M, 1, 1, p)
            other = b_block(M, 1 - p)
            assert s2["count"][other].tolist() == ([2, 3] if idle else [3, 3])
            if idle:
                assert par[:3].tolist() == [b0, b0 + 1, b0 + 2] and s2["score"][other, 0].tolist() == [-1.0, -2.0, 7.0]
                assert s2["yseq"][other, 0, :2, :2].tolist() == [[0, 1], [0, -3]]


@pytest.mark.gpu
def test_tsd_step_limits():
    """more than 16 slots, more slots than tokens, max_sym_exp 5: refused, nothing launched"""
    from espnet_amd import _lib
    T, n = 4, 1
    for W, V, M in ((17, 40, 2), (41, 40, 2), (4, 40, 5)):
        st, A = new_state(n, W, T, M), new_a(n, W, M)
        with pytest.raises(_lib.EamdError):
            _run_step(np.zeros((n * W, 1 + 2 * min(W, V - 1)), np.float32), None, st, A, V, T, M, 0, 0, 0)


# ---- 2. search vs float64 ----------------------------------------------------------------------------------------------------
T_S, E_S, D_S = 12, 6, 8
SEARCH_CASES = [(d, l, h) + shape for d, l, h in itertools.product(("lstm", "gru"), (1, 2), (12, 64))
                for shape in ((7, 6, 20, 2, 3), (7, 6, 3, 3, 2), (52, 257, 3, 2, 8), (52, 257, 8, 2, 4), (7, 6, 3, 4, 16))]


def search_case(dtype, L, H, J, V, B, M, beam, seed):
    sd = seeded_weights(seed, dtype, L, H, E_S, J, V, D_S, {6: 2.0}.get(V, 4.0))
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((B, T_S, D_S)).astype(np.float32)
    hlens = r.integers(T_S // 2, T_S + 1, B)
    hlens[0], hlens[1], hlens[2] = T_S, 1, 2
    return sd, hs, hlens


@functools.lru_cache(maxsize=None)
def search_reference(dtype, L, H, J, V, B, M, beam, seed):
    sd, hs, hlens = search_case(dtype, L, H, J, V, B, M, beam, seed)
    return tsd_batch64(weights_from_state_dict(sd), hs, hlens, beam, M)


@functools.lru_cache(maxsize=None)
def search_seed(dtype, L, H, J, V, B, M, beam):
    base = 31 * H + 7 * J + V + 1000 * L + 100000 * (dtype == "gru") + 17 * B + 3 * M + 1009 * beam
    for i in range(256):
        if search_reference(dtype, L, H, J, V, B, M, beam, base + 104729 * i)["min_gap"] >= GAP:
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
@pytest.mark.parametrize("dtype,L,H,J,V,B,M,beam", SEARCH_CASES)
def test_tsd_batch_vs_float64(dtype, L, H, J, V, B, M, beam):
    """tsd_batch on a seeded DecoderRNNT with ragged lengths (T, 1 and 2 among them) against the whole-search restatement: the same
    n-best lists in the same order, scores within 1e-4 relative; gap precondition asserted"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    case = (dtype, L, H, J, V, B, M, beam)
    seed = search_seed(*case)
    ref = search_reference(*case, seed)
    assert ref["min_gap"] >= GAP, ("precondition: float64 decision gap", ref["min_gap"])
    sd, hs, hlens = search_case(*case, seed)
    bs = BeamSearchTransducer(decoder=_decoder(sd, dtype, L, H, E_S, J, V, D_S), beam_size=beam, search_type="tsd", max_sym_exp=M)
    got = bs.tsd_batch(torch.from_numpy(hs).to(DEV), [int(v) for v in hlens])
    assert len(got) == B
    worst = max(_same_nbest(g, w, (case, b)) for b, (g, w) in enumerate(zip(got, ref["nbest"])))
    print("[parity] tsd_batch %s x%d H=%d J=%d V=%d B=%d M=%d beam=%d: %d merges, %d truncated, %d labels, min gap %.1e, "
          "score rel err %.2e" % (case + (ref["merges"], ref["truncated"], ref["labels"], ref["min_gap"], worst)))


# ---- 3. fixtures -------------------------------------------------------------------------------------------------------------
_FIX = [("tsd3", dict(beam_size=3, search_type="tsd", max_sym_exp=2)),
        ("tsd2", dict(beam_size=2, search_type="tsd", max_sym_exp=3, score_norm=False))]


def _same_lists(got, want, what):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        _same_nbest(g, [(h.score, h.yseq) for h in w], (what, b))


@pytest.mark.gpu
@pytest.mark.parametrize("tag,kw", _FIX, ids=[c[0] for c in _FIX])
@pytest.mark.parametrize("name", ["transducer_rnn.npz", "transducer_gru.npz"])
def test_tsd_batch_vs_per_utterance_search_and_reference(name, tag, kw):
    """the fixture's three utterances with their valid lengths: tsd_batch (hlens as list, device tensor, None) and recognize_batch
    equal the per-utterance search element by element; utterance 0 equals the n-best list the reference recorded"""
    from test_gpu_rnnt_greedy import _golden_model, _valid_lengths
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer, Hypothesis
    p, m = _golden_model(name)
    search = BeamSearchTransducer(decoder=m.dec, **kw)
    hs_pad = m.hs_pad.detach()
    hlens = _valid_lengths(m, p)
    assert max(hlens) == hs_pad.shape[1] and min(hlens) < max(hlens)
    one = [search(hs_pad[b, : hlens[b]]) for b in range(len(hlens))]
    got = search.tsd_batch(hs_pad, hlens)
    _same_lists(got, one, "ragged")
    _same_lists(search.tsd_batch(hs_pad, torch.tensor(hlens).to(DEV)), one, "tensor hlens")
    _same_lists(search.tsd_batch(hs_pad), [search(hs_pad[b]) for b in range(len(hlens))], "hlens=None: whole padded rows")
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
    inner = search._tsd

    def counted(h):
        calls[0] += 1
        return inner(h)
    search._tsd = counted
    got = search.tsd_batch(hs_pad, hlens)
    assert calls[0] == len(hlens)                          # the per-utterance search ran, once per utterance
    one = [search(hs_pad[b, : hlens[b]]) for b in range(len(hlens))]
    assert [[h.yseq for h in g] for g in got] == [[h.yseq for h in g] for g in one]
    assert [[h.score for h in g] for g in got] == [[h.score for h in g] for g in one]


@pytest.mark.gpu
def test_tsd_batch_fallbacks():
    """a custom prediction network, beam_size 17, max_sym_exp 5 and an LM go through the per-utterance loop and return what it
    returns"""
    from espnet_amd.nets.lm import ClassifierWithState, RNNLM
    from conftest import load_golden, split_golden
    _fallback_case("transducer_tt.npz", dict(beam_size=3, search_type="tsd", max_sym_exp=2))
    _fallback_case("transducer_rnn.npz", dict(beam_size=17, search_type="tsd", max_sym_exp=2))
    _fallback_case("transducer_rnn.npz", dict(beam_size=3, search_type="tsd", max_sym_exp=5))
    p, _sd, _ = split_golden(load_golden("transducer_rnn.npz"))
    lm = ClassifierWithState(RNNLM(6, 1, 8, None, "lstm", 0.0))
    lm.load_state_dict({k[3:]: v for k, v in p.items() if k.startswith("lm/")})
    _fallback_case("transducer_rnn.npz", dict(beam_size=3, search_type="tsd", nstep=2, lm_weight=0.5, lm=lm.to(DEV).eval()))


# ---- 4. one host read --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,rows", [(3, 256), (7, 12)])
def test_tsd_batch_reads_the_host_once(B, rows, monkeypatch):
    """blocking device-to-host reads counted as test_alsd_batch_reads_the_host_once counts them: exactly one per call for hlens
    None / list / device tensor, also when the batch goes in chunks (7 utterances x 4 slots in chunks of 12 rows: 3 + 3 + 1)"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    T = 12
    sd = seeded_weights(5, "lstm", 1, 64, E_S, 52, 257, D_S, 4.0)
    bs = BeamSearchTransducer(decoder=_decoder(sd, "lstm", 1, 64, E_S, 52, 257, D_S), beam_size=4, search_type="tsd", max_sym_exp=2)
    bs.tsd_max_rows = rows
    hs = torch.randn(B, T, D_S, generator=torch.Generator().manual_seed(B)).to(DEV)
    hl = torch.full((B,), T, dtype=torch.int32).to(DEV)
    whole = BeamSearchTransducer(decoder=bs.decoder, beam_size=4, search_type="tsd", max_sym_exp=2).tsd_batch(hs)
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
        results.append(bs.tsd_batch(hs, hlens))
        counts.append(reads[0])
    monkeypatch.undo()
    assert counts == [1, 1, 1], counts
    for got in results:                                    # chunks change the GEMMs' row counts, hence roundings, nothing else
        _same_lists(got, whole, "chunks of %d rows" % rows)
