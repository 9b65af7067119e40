"""Batched alignment-length-synchronous transducer beam search on the GPU: eamd_rnnt_alsd_step / eamd_gather_rows
(csrc/rnnt_alsd.hip) and BeamSearchTransducer.alsd_batch / E2E.recognize_batch against
  * tests/alsd_restatement.py - float64, pinned to the reference's loop by tests/test_alsd_restatement.py,
  * the per-utterance alsd search of the same package, and
  * the alsd n-best lists the reference recorded in tests/golden/transducer_rnn.npz / transducer_gru.npz.
Kernel: par, tok, live, frame, lengths, sequences and counts exact; scores within 1e-12 relative (float64 sums and a few roundings
of logaddexp).  Search: same n-best length, same sequences in the same order, scores within 1e-4 relative (the bound of
tests/test_gpu_transducer_search.py).  Equal sequences are meaningful where float32 cannot flip an ordering decision, so every
float64 decision gap (top-k boundary of an active row, adjacent scores of sorted A down to position W + 1, adjacent keys of the
final sort) must be >= 1e-4; this precondition is ASSERTED, and each case takes the first seed of its own sequence that meets it
on the CPU (tests/test_alsd_restatement.py checks that every case finds one; the choice never looks at a GPU result)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from alsd_restatement import alsd_batch64, alsd_step64, new_finals, new_state
from rnnt_greedy_restatement import seeded_weights, weights_from_state_dict

DEV = "cuda"
GAP = 1e-4


@pytest.fixture(autouse=True)
def _fp32():
    import espnet_amd
    espnet_amd.set_precision("fp32")
    yield
    espnet_amd.set_precision("fp32")


# ---- 1. the step kernel vs the one-step restatement -------------------------------------------------------------------------
def _run_step(rec, hlens, st, fin, V, T, u_max, i):
    """eamd_rnnt_alsd_step on numpy operands -> (state, finals, par, tok, live, frame) as numpy"""
    from espnet_amd import ops
    n, W = st["score"].shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    s_in = tuple(up(st[key]) for key in ("score", "ulen", "nhyp", "yseq"))
    s_out = (torch.full((n, W), 7.0, dtype=torch.float64, device=DEV), torch.full((n, W), -3, dtype=torch.int32, device=DEV),
             torch.full((n,), -3, dtype=torch.int32, device=DEV), torch.full(st["yseq"].shape, -3, dtype=torch.int32, device=DEV))
    f = tuple(up(fin[key]) for key in ("score", "len", "yseq", "nfin"))
    par, frame = (torch.full((n * W,), -3, dtype=torch.int32, device=DEV) for _ in range(2))
    tok = torch.full((n * W,), -3, dtype=torch.int64, device=DEV)
    live = torch.full((n * W,), 9, dtype=torch.uint8, device=DEV)
    hl = None if hlens is None else torch.from_numpy(np.asarray(hlens, np.int32)).to(DEV)
    ops.rnnt_alsd_step(up(np.asarray(rec, np.float32)), hl, s_in, s_out, f, par, tok, live, frame, V, T, u_max, i)
    torch.cuda.synchronize()
    out = dict(zip(("score", "ulen", "nhyp", "yseq"), (x.cpu().numpy() for x in s_out)))
    fo = dict(zip(("score", "len", "yseq", "nfin"), (x.cpu().numpy() for x in f)))
    return out, fo, par.cpu().numpy(), tok.cpu().numpy(), live.cpu().numpy(), frame.cpu().numpy()


def _close(a, b):
    return a == b or abs(a - b) <= 1e-12 * max(abs(a), abs(b)) or (a != a and b != b)


def _check_step(rec, hlens, st, fin, V, T, u_max, i, stats=None):
    want = alsd_step64(np.asarray(rec, np.float32), hlens, st, fin, V, T, u_max, i, stats)
    got = _run_step(rec, hlens, st, fin, V, T, u_max, i)
    ws, wf, wpar, wtok, wlive, wframe, _act = want
    gs, gf, gpar, gtok, glive, gframe = got
    n, W = st["score"].shape
    what = (n, W, V, i)
    assert gs["nhyp"].tolist() == ws["nhyp"].tolist(), what
    assert gpar.tolist() == wpar.tolist() and gtok.tolist() == wtok.tolist(), what
    assert glive.tolist() == wlive.tolist() and gframe.tolist() == wframe.tolist(), what
    assert gf["nfin"].tolist() == wf["nfin"].tolist(), what
    for b in range(n):
        for m in range(int(ws["nhyp"][b])):
            u = int(ws["ulen"][b, m])
            assert int(gs["ulen"][b, m]) == u, what
            assert gs["yseq"][b, m, :u + 1].tolist() == ws["yseq"][b, m, :u + 1].tolist(), what
            assert _close(float(gs["score"][b, m]), float(ws["score"][b, m])), (what, b, m, gs["score"][b, m], ws["score"][b, m])
        for q in range(int(wf["nfin"][b])):
            ln = int(wf["len"][b, q])
            assert int(gf["len"][b, q]) == ln, what
            assert gf["yseq"][b, q, :ln].tolist() == wf["yseq"][b, q, :ln].tolist(), what
            assert _close(float(gf["score"][b, q]), float(wf["score"][b, q])), (what, b, q)
    return want, got


def _random_step(r, n, W, V, T, u_max, i, ties):
    """a state as step i can meet it (t = i - ulen + 1 >= 1; labels in 1 .. V - 1) with nhyp < W in places, parents that are one
    label apart so that a blank continuation and an extension meet, and - with `ties` - scores on a grid of 1 / 4 so that equal
    scores are common; rec with k distinct tokens per row"""
    k = min(W, V - 1)
    st, fin = new_state(n, W, T, u_max), new_finals(n, W, u_max)
    rec = np.zeros((n * W, 1 + 2 * k), np.float32)
    val = (lambda *s: -r.integers(1, 12, s) / 4.0) if ties else (lambda *s: -r.random(s) * 4.0 - 0.01)
    for b in range(n):
        nh = int(r.integers(1, W + 1))
        st["nhyp"][b] = nh
        for w in range(nh):
            u = int(r.integers(0, i + 1))
            y = [0] + [int(v) for v in r.integers(1, V, u)]
            if w and r.random() < 0.5:                    # the previous slot's labels plus one, or minus one
                prev = [int(v) for v in st["yseq"][b, w - 1, :st["ulen"][b, w - 1] + 1]]
                y = prev + [int(r.integers(1, V))] if len(prev) - 1 < i and r.random() < 0.5 else (prev[:-1] if len(prev) > 1 else prev)
            st["ulen"][b, w] = len(y) - 1
            st["yseq"][b, w, :len(y)] = y
            st["score"][b, w] = val()
            row = b * W + w
            rec[row, :1 + k] = val(1 + k)
            rec[row, 1 + k:] = r.permutation(np.arange(1, V))[:k]
            if w and len(y) == st["ulen"][b, w - 1] + 2 and y[:-1] == st["yseq"][b, w - 1, :len(y) - 1].tolist():
                toks = rec[row - 1, 1 + k:]                # the shorter parent's best extension is the longer one's last label
                toks[toks == y[-1]] = toks[0]
                toks[0] = y[-1]
        q = int(r.integers(0, 3))                         # finals of earlier steps stay in front
        fin["nfin"][b] = q
        fin["score"][b, :q] = -1.5
        fin["len"][b, :q] = 1
    return rec, st, fin


@pytest.mark.gpu
@pytest.mark.parametrize("n,W,V", [(n, W, V) for n in (1, 3) for W in (1, 2, 3, 8, 16) for V in (2, 3, 6, 40) if W <= V])
def test_alsd_step_vs_restatement(n, W, V):
    """random states of steps early, late and past the end, ragged hlens including 1 and 2, with and without score ties
    (W = min(beam_size, V), so W <= V; k = min(W, V - 1) < W where W == V)"""
    T, u_max = 6, 3
    r = np.random.default_rng(1000 * n + 10 * W + V)
    stats = {}
    for trial in range(8):
        i = int(r.integers(0, T + u_max + 1))
        hlens = None if trial == 0 else r.choice([1, 2, T - 1, T], n).astype(np.int32)
        if trial == 1 and n == 3:
            hlens = np.array([1, 2, T], np.int32)
        rec, st, fin = _random_step(r, n, W, V, T, u_max, i, ties=bool(trial & 1))
        _check_step(rec, hlens, st, fin, V, T, u_max, i, stats)
    print("[parity] alsd step n=%d W=%d V=%d: %d merges, %d dropped over 8 steps" % (n, W, V, stats.get("merges", 0),
                                                                                     stats.get("dropped", 0)))


def _state(T, u_max, W, hyps, n=1):
    """hyps: per utterance [(score, labels)]"""
    st = new_state(n, W, T, u_max)
    for b, hb in enumerate(hyps):
        st["nhyp"][b] = len(hb)
        for w, (s, y) in enumerate(hb):
            st["score"][b, w], st["ulen"][b, w] = s, len(y) - 1
            st["yseq"][b, w, :len(y)] = y
    return st


def _rec(W, k, rows):
    """rows: {row: (blank logp, [(logp, token)] * k)}; other rows: -20 everywhere, tokens 1 .. k"""
    n_rows = max(rows) // W * W + W
    rec = np.full((n_rows, 1 + 2 * k), -20.0, np.float32)
    rec[:, 1 + k:] = np.arange(1, k + 1)
    for r_, (bl, ext) in rows.items():
        rec[r_, 0] = bl
        rec[r_, 1:1 + k] = [lp for lp, _t in ext]
        rec[r_, 1 + k:] = [t for _lp, t in ext]
    return rec


@pytest.mark.gpu
def test_alsd_step_crafted_cases():
    T, u_max, V = 5, 3, 6
    W, k = 3, 3
    la = lambda *v: float(functools.reduce(np.logaddexp, v))      # noqa: E731
    # T_b = 4, i = 2.  [0, 3] (t = 2) by blank and [0] (t = 3 = T_b - 1) + 3 reach the same sequence: merged into the first, the
    # duplicate kept with its own score; [0]'s blank continuation is a final that was not selected (raw score)
    st = _state(T, u_max, W, [[(-1.0, [0, 3]), (-1.5, [0]), (-9.0, [0, 4])]])
    rec = _rec(W, k, {0: (-0.25, [(-5.0, 2), (-9.0, 1), (-9.5, 4)]), 1: (-7.0, [(-0.5, 3), (-9.0, 1), (-9.5, 2)])})
    stats = {}
    (ws, wf, *_), _ = _check_step(rec, np.array([4], np.int32), st, new_finals(1, W, u_max), V, T, u_max, 2, stats)
    assert stats["merges"] == 1 and stats["dropped"] == 0
    assert [ws["yseq"][0, m, :ws["ulen"][0, m] + 1].tolist() for m in range(3)] == [[0, 3], [0, 3], [0, 3, 2]]
    assert ws["score"][0].tolist() == [la(-1.25, -2.0), -2.0, -6.0]
    assert wf["nfin"][0] == 1 and wf["score"][0, 0] == -8.5 and wf["len"][0, 0] == 1
    # the same step with T_b = 3: [0, 3] is on the last frame (final, selected, nothing merges into it), [0] is past it and
    # vanishes while the others are active
    stats = {}
    (ws, wf, *_), _ = _check_step(rec, np.array([3], np.int32), st, new_finals(1, W, u_max), V, T, u_max, 2, stats)
    assert stats["dropped"] == 1 and "merges" not in stats and wf["nfin"][0] == 2 and wf["score"][0, 0] == -1.25
    # T_b = 3, i = 2, all three slots on the last frame; two of them hold [0, 3] (a duplicate an earlier step kept): the first final
    # was selected and grew by the recombination, the second was selected and is a duplicate (raw), the third was not selected
    st = _state(T, u_max, W, [[(-1.0, [0, 3]), (-1.5, [0, 3]), (-0.5, [0, 4])]])
    rec = _rec(W, k, {0: (-0.25, [(-9.0, 2), (-9.0, 1), (-9.5, 4)]), 1: (-0.25, [(-9.0, 2), (-9.0, 1), (-9.5, 4)]),
                      2: (-9.0, [(-0.5, 1), (-9.0, 2), (-9.5, 3)])})
    stats = {}
    (ws, wf, *_), _ = _check_step(rec, np.array([3], np.int32), st, new_finals(1, W, u_max), V, T, u_max, 2, stats)
    assert stats["merges"] == 1 and ws["score"][0].tolist() == [-1.0, la(-1.25, -1.75), -1.75]
    assert wf["nfin"][0] == 3 and wf["score"][0, :3].tolist() == [la(-1.25, -1.75), -1.75, -9.5]
    # three equal sequences: [0, 2, 2] by blank, [0, 2] + 2 from two slots: both add to the first
    W, k = 4, 4
    st = _state(T, u_max, W, [[(-1.0, [0, 2, 2]), (-1.5, [0, 2]), (-1.75, [0, 2])]])
    ext = lambda lp: [(lp, 2), (-9.0, 1), (-9.5, 3), (-9.75, 4)]      # noqa: E731
    rec = _rec(W, k, {0: (-0.25, ext(-8.0)), 1: (-6.0, ext(-0.5)), 2: (-6.5, ext(-0.5))})
    stats = {}
    (ws, wf, *_), _ = _check_step(rec, None, st, new_finals(1, W, u_max), V, T, u_max, 3, stats)
    assert stats["merges"] == 2 and ws["score"][0, :3].tolist() == [la(la(-1.25, -2.0), -2.25), -2.0, -2.25]
    # equal scores: A's order decides (slot 0's blank continuation, then its extensions in the record's order)
    st = _state(T, u_max, W, [[(-1.0, [0, 1]), (-1.0, [0, 2]), (-1.0, [0, 3])]])
    rec = _rec(W, k, {r_: (-0.5, [(-0.5, 4), (-0.5, 3), (-0.5, 2), (-0.5, 1)]) for r_ in range(3)})
    _w, (_gs, _gf, gpar, gtok, _gl, _gfr) = _check_step(rec, None, st, new_finals(1, W, u_max), V, T, u_max, 2)
    assert gpar.tolist() == [0, 0, 0, 0] and gtok.tolist() == [0, 4, 3, 2]
    # NaN sorts as -inf, +inf first
    st = _state(T, u_max, W, [[(-1.0, [0, 1]), (float("nan"), [0, 2]), (float("inf"), [0, 3])]])
    _w, (_gs, _gf, gpar, *_r) = _check_step(rec, None, st, new_finals(1, W, u_max), V, T, u_max, 2)
    assert gpar.tolist() == [2, 2, 2, 2]
    # hlens 1, 2, T and beyond T in one batch, nhyp < W, at steps where utterances are over (i >= T_b + u_max_b), where no slot is
    # active (B carried) and past the last step of all
    W, k = 3, 3
    hy = [(-1.0, [0]), (-2.0, [0, 1])]
    st = _state(T, u_max, W, [hy, hy, hy, hy], n=4)
    rec = _rec(W, k, {r_: (-0.5, [(-0.25, 4), (-0.75, 3), (-1.0, 2)]) for r_ in range(12)})
    fin = new_finals(4, W, u_max)
    carried = 0
    for i in (1, 2, 4, 5, 7, 8):
        (ws, wf, wpar, _t, wlive, _f, act), _ = _check_step(rec, np.array([1, 2, T, T + 3], np.int32), st, fin, V, T, u_max, i)
        assert not act[0].any() and wpar[:3].tolist() == [0, 1, 2] and not wlive[:3].any() and ws["nhyp"][0] == 2
        assert act[2].any() == (i <= T - 1) and act[3].tolist() == act[2].tolist()      # the longer slot: t = i - 1 + 1
        carried += int(not act[2].any())
    assert carried == 3                                     # i = 5, 7: no active slot; i = 8 = T + u_max: past the last step
    # every slot past the last frame while the utterance is not over: B is carried (the reference's `if B_:`)
    st = _state(T, u_max, W, [[(-1.0, [0]), (-2.0, [0, 1])]])
    (ws, wf, _p, _t, _l, _f, act), _ = _check_step(rec[:3], None, st, new_finals(1, W, u_max), V, T, u_max, 6)
    assert not act.any() and ws["score"][0, :2].tolist() == [-1.0, -2.0] and wf["nfin"][0] == 0
    # a full final list is never written past its end (a guard: the reference's list cannot be full)
    fin["nfin"][:] = W * (u_max + 2)
    _gs, gf, *_r = _run_step(rec, None, _state(T, u_max, W, [hy, hy, hy, hy], n=4), fin, V, T, u_max, 4)
    assert gf["nfin"].tolist() == [W * (u_max + 2)] * 4


@pytest.mark.gpu
def test_alsd_step_limits():
    """more than 16 slots, or more slots than tokens: refused, nothing launched"""
    from espnet_amd import _lib
    T, u_max, V, n = 4, 2, 40, 1
    for W in (17, 41):
        st, fin = new_state(n, W, T, u_max), new_finals(n, W, u_max)
        with pytest.raises(_lib.EamdError):
            _run_step(np.zeros((n * W, 1 + 2 * min(W, V - 1)), np.float32), None, st, fin, V, T, u_max, 0)


# ---- 2. gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("njobs", [1, 16])
def test_gather_rows_vs_index_select(njobs):
    from espnet_amd import ops
    g = torch.Generator().manual_seed(njobs)
    jobs, want = [], []
    for j in range(njobs):
        width = (4, 68, 7)[j % 3] if njobs > 1 else 68
        m, rows = 5 + 3 * j, (1, 9, 300)[j % 3]
        src = torch.randn(m, width, generator=g).to(DEV)
        idx = torch.randint(0, m, (rows,), generator=g, dtype=torch.int32)
        idx[: rows // 2] = idx[0]                          # repeated indices
        idx = idx.to(DEV)
        dst = torch.full((rows, width), float("nan"), device=DEV)
        jobs.append((dst, src, idx))
        want.append(src.index_select(0, idx.long()))
    ops.gather_rows(jobs)
    for (dst, _s, _i), w in zip(jobs, want):
        assert torch.equal(dst, w)
    if njobs == 1:                                         # width 4, and a view whose rows are not 16-byte aligned
        src = torch.randn(6, 4, generator=g).to(DEV)
        idx = torch.tensor([5, 5, 0, 3], dtype=torch.int32).to(DEV)
        dst = torch.empty(4, 4, device=DEV)
        ops.gather_rows([(dst, src, idx)])
        assert torch.equal(dst, src.index_select(0, idx.long()))
        flat = torch.randn(6 * 4 + 1, generator=g).to(DEV)
        ops.gather_rows([(dst, flat[1:].view(6, 4), idx)])
        assert torch.equal(dst, flat[1:].view(6, 4).index_select(0, idx.long()))


# ---- 3. search vs float64 ----------------------------------------------------------------------------------------------------
T_S, E_S, D_S = 12, 6, 8
# every value of (dtype, L, H), (J, V), B, u_max and beam, each (dtype, L, H) with every beam while the other three rotate (24
# searches; the full product would be 192)
SEARCH_CASES = []
for _q, (_d, _l, _h) in enumerate(itertools.product(("lstm", "gru"), (1, 2), (12, 64))):
    for _j, _beam in enumerate((2, 3, 8)):
        _B = (3, 20)[(_q // 2 + _j) % 2]
        # 20 utterances x 8 slots at V = 257 take some 2400 top-k boundaries among 256 close log-probabilities: no seed keeps them
        # all 1e-4 apart, so beam 8 meets V = 257 on 3 utterances and 20 utterances on V = 6 (k = V - 1: no boundary)
        _J, _V = (7, 6) if (_beam, _B) == (8, 20) else ((7, 6), (52, 257))[(_q + _j) % 2]
        SEARCH_CASES.append((_d, _l, _h, _J, _V, _B, (4, 20)[(_q // 4 + _j // 2 + _q) % 2], _beam))


def search_case(dtype, L, H, J, V, B, u_max, beam, seed):
    sd = seeded_weights(seed, dtype, L, H, E_S, J, V, D_S, {6: 2.0}.get(V, 4.0))
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((B, T_S, D_S)).astype(np.float32)
    hlens = r.integers(T_S // 2, T_S + 1, B)
    hlens[0], hlens[1], hlens[2] = T_S, 1, 2
    return sd, hs, hlens


@functools.lru_cache(maxsize=None)
def search_reference(dtype, L, H, J, V, B, u_max, beam, seed):
    sd, hs, hlens = search_case(dtype, L, H, J, V, B, u_max, beam, seed)
    return alsd_batch64(weights_from_state_dict(sd), hs, hlens, beam, u_max)


@functools.lru_cache(maxsize=None)
def search_seed(dtype, L, H, J, V, B, u_max, beam):
    base = 31 * H + 7 * J + V + 1000 * L + 100000 * (dtype == "gru") + 17 * B + 3 * u_max + 1009 * beam
    for i in range(256):
        if search_reference(dtype, L, H, J, V, B, u_max, beam, base + 104729 * i)["min_gap"] >= GAP:
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
@pytest.mark.parametrize("dtype,L,H,J,V,B,u_max,beam", SEARCH_CASES)
def test_alsd_batch_vs_float64(dtype, L, H, J, V, B, u_max, beam):
    """alsd_batch on a seeded DecoderRNNT with ragged lengths (T, 1 and 2 among them) against the whole-search restatement: the
    same n-best lists in the same order, scores within 1e-4 relative; gap precondition asserted"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    case = (dtype, L, H, J, V, B, u_max, beam)
    seed = search_seed(*case)
    ref = search_reference(*case, seed)
    assert ref["min_gap"] >= GAP, ("precondition: float64 decision gap", ref["min_gap"])
    sd, hs, hlens = search_case(*case, seed)
    bs = BeamSearchTransducer(decoder=_decoder(sd, dtype, L, H, E_S, J, V, D_S), beam_size=beam, search_type="alsd", u_max=u_max)
    got = bs.alsd_batch(torch.from_numpy(hs).to(DEV), [int(v) for v in hlens])
    assert len(got) == B
    worst = max(_same_nbest(g, w, (case, b)) for b, (g, w) in enumerate(zip(got, ref["nbest"])))
    print("[parity] alsd_batch %s x%d H=%d J=%d V=%d B=%d u_max=%d beam=%d: %d finals, %d merges, %d dropped, %d without finals, "
          "min gap %.1e, score rel err %.2e" % (case + (ref["finals"], ref["merges"], ref["dropped"], ref["no_final"], ref["min_gap"],
                                                         worst)))


# ---- 4. fixtures -------------------------------------------------------------------------------------------------------------
_FIX = [("alsd3", dict(beam_size=3, search_type="alsd", u_max=10)),
        ("alsd2", dict(beam_size=2, search_type="alsd", u_max=4, score_norm=False))]


def _same_lists(got, want, what):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        _same_nbest(g, [(h.score, h.yseq) for h in w], (what, b))


@pytest.mark.gpu
@pytest.mark.parametrize("tag,kw", _FIX, ids=[c[0] for c in _FIX])
@pytest.mark.parametrize("name", ["transducer_rnn.npz", "transducer_gru.npz"])
def test_alsd_batch_vs_per_utterance_search_and_reference(name, tag, kw):
    """the fixture's three utterances with their valid lengths: alsd_batch (hlens as list, device tensor, None) and recognize_batch
    equal the per-utterance search element by element; utterance 0 equals the n-best list the reference recorded"""
    from test_gpu_rnnt_greedy import _golden_model, _valid_lengths
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer, Hypothesis
    p, m = _golden_model(name)
    search = BeamSearchTransducer(decoder=m.dec, **kw)
    hs_pad = m.hs_pad.detach()
    hlens = _valid_lengths(m, p)
    assert max(hlens) == hs_pad.shape[1] and min(hlens) < max(hlens)
    one = [search(hs_pad[b, : hlens[b]]) for b in range(len(hlens))]
    got = search.alsd_batch(hs_pad, hlens)
    _same_lists(got, one, "ragged")
    _same_lists(search.alsd_batch(hs_pad, torch.tensor(hlens).to(DEV)), one, "tensor hlens")
    _same_lists(search.alsd_batch(hs_pad), [search(hs_pad[b]) for b in range(len(hlens))], "hlens=None: whole padded rows")
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
    inner = search._alsd

    def counted(h):
        calls[0] += 1
        return inner(h)
    search._alsd = counted
    got = search.alsd_batch(hs_pad, hlens)
    assert calls[0] == len(hlens)                          # the per-utterance search ran, once per utterance
    one = [search(hs_pad[b, : hlens[b]]) for b in range(len(hlens))]
    assert [[h.yseq for h in g] for g in got] == [[h.yseq for h in g] for g in one]
    assert [[h.score for h in g] for g in got] == [[h.score for h in g] for g in one]


@pytest.mark.gpu
def test_alsd_batch_fallbacks():
    """a custom prediction network, an LM and beam_size 17 go through the per-utterance loop and return what it returns"""
    from espnet_amd.nets.lm import ClassifierWithState, RNNLM
    from conftest import load_golden, split_golden
    _fallback_case("transducer_tt.npz", dict(beam_size=3, search_type="alsd", u_max=10))
    _fallback_case("transducer_rnn.npz", dict(beam_size=17, search_type="alsd", u_max=10))
    p, _sd, _ = split_golden(load_golden("transducer_rnn.npz"))
    lm = ClassifierWithState(RNNLM(6, 1, 8, None, "lstm", 0.0))
    lm.load_state_dict({k[3:]: v for k, v in p.items() if k.startswith("lm/")})
    _fallback_case("transducer_rnn.npz", dict(beam_size=3, search_type="alsd", nstep=2, lm_weight=0.5, lm=lm.to(DEV).eval()))


# ---- 5. one host read --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,rows", [(3, 256), (7, 12)])
def test_alsd_batch_reads_the_host_once(B, rows, monkeypatch):
    """blocking device-to-host reads counted as test_greedy_batch_reads_the_host_once counts them: exactly one per call for hlens
    None / list / device tensor, also when the batch goes in chunks (7 utterances x 4 slots in chunks of 12 rows: 3 + 3 + 1)"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    T = 12
    sd = seeded_weights(5, "lstm", 1, 64, E_S, 52, 257, D_S, 4.0)
    bs = BeamSearchTransducer(decoder=_decoder(sd, "lstm", 1, 64, E_S, 52, 257, D_S), beam_size=4, search_type="alsd", u_max=6)
    bs.alsd_max_rows = rows
    hs = torch.randn(B, T, D_S, generator=torch.Generator().manual_seed(B)).to(DEV)
    hl = torch.full((B,), T, dtype=torch.int32).to(DEV)
    whole = BeamSearchTransducer(decoder=bs.decoder, beam_size=4, search_type="alsd", u_max=6).alsd_batch(hs)
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
        results.append(bs.alsd_batch(hs, hlens))
        counts.append(reads[0])
    monkeypatch.undo()
    assert counts == [1, 1, 1], counts
    for got in results:                                    # chunks change the GEMMs' row counts, hence roundings, nothing else
        _same_lists(got, whole, "chunks of %d rows" % rows)
