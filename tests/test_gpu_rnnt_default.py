"""Batched default (Graves A / B) transducer beam search on the GPU: eamd_rnnt_default_step and eamd_scatter_rows
(csrc/rnnt_default.hip) and BeamSearchTransducer.default_batch / E2E.recognize_batch against
  * tests/default_restatement.py - float64, pinned to a plain per-utterance statement by tests/test_default_restatement.py,
  * the per-utterance default search of the same package, and
  * the n-best lists the reference recorded in tests/golden/transducer_rnn.npz / transducer_gru.npz.
Kernel: every array of the state and every per-utterance output exact - whole arrays that start as sentinels, so what the kernel must
not write shows as well; scores within 1e-12 relative (float64 sums of a float64 and a float32; the restatement adds the same values
in the same order, so they are in fact equal).  Search: same n-best length, same sequences in the same order, scores within 1e-4
relative (the bound of tests/test_gpu_transducer_search.py), no overflow.  Equal sequences are meaningful where float32 cannot flip an
ordering decision, so every float64 decision gap (top-2 of A at each pop, the top-k boundary of each row, each score of B against
bound, adjacent scores of ahead, adjacent keys of the final sort) must be >= 1e-4, no frame may take more than default_max_pops
pops and the slowest utterance must stay within the step budget; this precondition is ASSERTED, and each case takes the first seed of
its own sequence that meets it in the float64 restatement alone (tests/test_default_restatement.py checks that every case finds
one; the choice never looks at a GPU result)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from default_restatement import C_NA, C_NB, C_NLOG, C_POPS, C_T, OUT, STATE, default_batch64, default_step64, new_state
from rnnt_greedy_restatement import seeded_weights, weights_from_state_dict

DEV = "cuda"
GAP = 1e-4


@pytest.fixture(autouse=True)
def _fp32():
    import espnet_amd
    espnet_amd.set_precision("fp32")
    yield
    espnet_amd.set_precision("fp32")


# ---- 1. the step kernel vs the one-step restatement ----------------------------------------------------------------------------
_SENT = dict(par=-3, tok=-3, dst=-3, live=9, frame=-3, alive=9)
_ODT = dict(par=torch.int32, tok=torch.int64, dst=torch.int32, live=torch.uint8, frame=torch.int32, alive=torch.uint8)


def _device_step(rec, hlens, st, W, V, T):
    """eamd_rnnt_default_step on numpy operands -> (state, outputs) as numpy; the outputs start as sentinels"""
    from espnet_amd import ops
    n = st["ctr"].shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    d = {key: up(st[key]) for key in STATE}
    o = {key: torch.full((n,), _SENT[key], dtype=_ODT[key], device=DEV) for key in OUT}
    hl = None if hlens is None else up(np.asarray(hlens, np.int32))
    ops.rnnt_default_step(up(np.asarray(rec, np.float32)), hl, tuple(d[key] for key in STATE[:5]), tuple(d[key] for key in STATE[5:8]),
                          d["cur"], d["ctr"], d["log"], d["flags"], *[o[key] for key in OUT], W, V, T)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in d.items()}, {key: v.cpu().numpy() for key, v in o.items()}


def _close(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return bool(np.all((got == want) | (np.abs(got - want) <= 1e-12 * np.maximum(np.abs(got), np.abs(want)))
                           | (np.isnan(got) & np.isnan(want))))


def _check_step(rec, hlens, st, W, V, T, stats=None):
    rec = np.asarray(rec, np.float32)
    ws, wo = default_step64(rec, hlens, st, W, V, T, stats)
    gs, go = _device_step(rec, hlens, st, W, V, T)
    what = (st["ctr"].tolist(), W, V, T)
    for key in OUT:
        assert go[key].tolist() == wo[key].tolist(), (what, key, go[key], wo[key])
    for key in STATE:
        if key in ("a_score", "b_score", "cur"):
            assert _close(gs[key], ws[key]), (what, key, gs[key], ws[key])
        else:
            assert np.array_equal(gs[key], ws[key]), (what, key, gs[key], ws[key])
    return ws, wo


def _sentinel_state(n, P, log_cap, hlens, T):
    """new_state with every entry that holds nothing yet set to a sentinel"""
    st, out = new_state(n, P, log_cap, hlens, T)
    for key in STATE[:8]:
        keep = st[key][:, 0].copy()
        st[key][:] = 7.0 if key.endswith("score") else -3
        if key.startswith("b_"):
            st[key][:, 0] = np.where(st["ctr"][:, C_NB] > 0, keep, st[key][:, 0])
    st["log"][:, 1:] = -3
    return st, out


def _random_rec(r, n, k, V, ties):
    rec = np.zeros((n, 1 + 2 * k), np.float32)
    for b in range(n):
        rec[b, 0] = -r.integers(0, 4) / 4.0 if ties else -r.random() * 0.8 - 0.01
        ext = -r.integers(1, 12, k) / 4.0 if ties else -r.random(k) * 4.0 - 0.01
        rec[b, 1:1 + k] = -np.sort(-ext)
        rec[b, 1 + k:] = r.permutation(np.arange(1, V))[:k]
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("n,W,V", [(n, W, V) for n in (1, 3) for W in (1, 2, 3, 8, 16) for V in (2, 3, 6, 40) if W <= V])
def test_default_step_vs_restatement(n, W, V):
    """two searches on random joint rows, step by step, every step on the device and in the restatement from the same state: with
    score ties on a grid of 1 / 4 and a small P (the cut, and frames that overflow), and without ties at P = 256.  The states are
    those a search meets: mid-frame, a pop that ends a frame, the last frame, a finished utterance beside live ones (nothing of it
    changes), hlens 0, 1 and 2 beside T, and hlens NULL"""
    T, k = 4, min(W, V - 1)
    r = np.random.default_rng(1000 * n + 10 * W + V)
    stats = {}
    for ties in (True, False):
        P = W + 5 if ties else 256
        hlens = None if (n == 1 and ties) else np.array(([T, 0, 1] if ties else [2, T, 1])[:n], np.int32)
        log_cap = 40 if ties else 1 + 64 * W * T
        st, _ = _sentinel_state(n, P, log_cap, hlens, T)
        for _step in range(64 * W * T):                                       # the searches run to their end
            st, out = _check_step(_random_rec(r, n, k, V, ties), hlens, st, W, V, T, stats)
            if (st["flags"][0] | st["flags"][1]).all():
                break
        assert (st["flags"][0] | st["flags"][1]).all() and (ties or st["flags"][0].all())
        s1, out = _check_step(_random_rec(r, n, k, V, ties), hlens, st, W, V, T)    # every utterance has stopped: nothing changes
        assert all(np.array_equal(s1[key], st[key]) for key in STATE) and not out["alive"].any()
    print("[parity] default step n=%d W=%d V=%d: pops per frame %s, %d long ahead lists, %d entries cut, smallest gap %.2g"
          % (n, W, V, sorted(set(sum(stats.get("pops", {}).values(), []))), stats.get("long_ahead", 0), stats.get("cut", 0),
             stats.get("gap", np.inf)))


def _made(n, W, V, T, P, log_cap, ctr, cur, A=(), B=()):
    """a hand-made state of one utterance: ctr[:7], A = [(score, seq, row, log, tok)], B = [(score, row, log)]"""
    st, _ = _sentinel_state(n, P, log_cap, [T] * n, T)
    st["ctr"][0, :7] = ctr
    st["cur"][0] = cur
    st["log"][0, 1:ctr[4]] = 0
    for x, e in enumerate(A):
        for key, v in zip(STATE[:5], e):
            st[key][0, x] = v
    for x, e in enumerate(B):
        for key, v in zip(STATE[5:8], e):
            st[key][0, x] = v
    return st


@pytest.mark.gpu
def test_default_step_crafted_cases():
    n, W, V, T, P = 1, 2, 6, 3, 8
    # the first maximum: a carried entry and a fresh child tie at -1.0; the carried one is earlier in list order
    st = _made(n, W, V, T, P, 16, [1, 1, 1, 0, 3, 2, 2], -0.5, A=[(-1.0, 1, 1, 1, 0)])
    s1, out = _check_step([[-9.0, -0.5, -2.0, 3, 5]], None, st, W, V, T)
    assert (out["par"][0], out["tok"][0], out["dst"][0], out["live"][0], out["alive"][0]) == (1, 0, P + 1, 0, 1)
    assert s1["a_tok"][0, :2].tolist() == [3, 5] and s1["a_score"][0, 2] == 7.0 and s1["log"][0, 3].tolist() == [1, 0]
    # ... and the child first when it is strictly better
    s1, out = _check_step([[-9.0, -0.25, -2.0, 3, 5]], None, st, W, V, T)
    assert (out["par"][0], out["tok"][0], out["live"][0]) == (P, 3, 1) and s1["log"][0, 3].tolist() == [2, 3]
    # ahead of W + 2 entries: all of them are carried into the next frame
    stats = {}
    st = _made(n, W, V, T, P, 16, [0, 4, 0, 3, 4, 8, 3], -0.875, B=[(-1.0, 0, 0), (-1.25, 1, 1), (-1.125, 2, 2)])
    s1, out = _check_step([[-0.0625, -5.0, -6.0, 1, 2]], None, st, W, V, T, stats)
    assert stats["long_ahead"] == 1 and s1["ctr"][0, :7].tolist() == [1, 1, 3, 0, 5, 4, 4] and s1["a_seq"][0, :3].tolist() == [2, 1, 0]
    # ... and, on the last frame, into B in ascending order
    st["ctr"][0, C_T] = T - 1
    s1, out = _check_step([[-0.0625, -5.0, -6.0, 1, 2]], None, st, W, V, T)
    assert s1["flags"][:, 0].tolist() == [1, 0] and s1["ctr"][0, C_NB] == 4 and out["alive"][0] == 0
    assert s1["b_score"][0, :4].tolist() == [-1.25, -1.125, -1.0, -0.9375]
    # NaN orders as -inf: the NaN child goes last, a NaN in B is never ahead
    st = _made(n, W, V, T, P, 16, [0, 2, 0, 1, 2, 2, 1], -0.5, B=[(float("nan"), 0, 0)])
    s1, out = _check_step([[-0.5, float("nan"), -1.0, 3, 5]], None, st, W, V, T)
    assert out["tok"][0] == 5 and s1["ctr"][0, C_T] == 0 and np.isnan(s1["a_score"][0, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("W,V,P", [(2, 6, 2), (16, 40, 256)])
def test_default_step_cuts_a_at_exactly_p(W, V, P):
    """A holds P - 1 entries and gains k: the P best stay, in order, one of them is popped"""
    n, T, k = 1, 3, min(W, V - 1)
    r = np.random.default_rng(P)
    A = [(-1.0 - float(x) / 8, x, x % P, 1, 0) for x in range(P - 1)]
    st = _made(n, W, V, T, P, 600, [1, P - 1, P - 1, 0, 2, P - 1, 1], -0.5, A=A)
    rec = _random_rec(r, n, k, V, False)
    rec[0, 0] = -50.0
    stats = {}
    s1, out = _check_step(rec, None, st, W, V, T, stats)
    assert stats["cut"] == k - 1 and s1["ctr"][0, C_NA] == P - 1 and s1["ctr"][0, C_POPS] == P and out["alive"][0] == 1
    # the (P + 1)-th pop of the frame: overflow, and the utterance is frozen
    s2, out = _check_step(rec, None, s1, W, V, T)
    assert s2["flags"][:, 0].tolist() == [0, 1] and out["alive"][0] == 0 and out["live"][0] == 0 and s2["ctr"][0, C_POPS] == P
    s3, out = _check_step(rec, None, s2, W, V, T)
    assert all(np.array_equal(s3[key], s2[key]) for key in STATE)


@pytest.mark.gpu
def test_default_step_full_log_and_limits():
    from espnet_amd import _lib, ops
    n, W, V, T, P = 1, 2, 6, 3, 8
    st = _made(n, W, V, T, P, 3, [1, 1, 1, 0, 3, 2, 2], -0.5, A=[(-1.0, 1, 1, 1, 0)])
    s1, out = _check_step([[-9.0, -0.5, -2.0, 3, 5]], None, st, W, V, T)
    assert s1["flags"][:, 0].tolist() == [0, 1] and out["alive"][0] == 0 and s1["ctr"][0, C_NLOG] == 3 and s1["ctr"][0, C_NA] == 3
    # W = 17, P = 257, P < W: refused before any launch, nothing is written
    for W_, V_, P_ in ((17, 40, 32), (4, 40, 257), (4, 40, 3)):
        st, _ = _sentinel_state(n, P_, 8, [T], T)
        with pytest.raises(_lib.EamdError):
            _device_step(np.zeros((n, 1 + 2 * min(W_, V_ - 1)), np.float32), None, st, W_, V_, T)
    torch.cuda.synchronize()
    lib = _lib.lib()
    assert lib.eamd_rnnt_default_step(*([None] * 20), 1, 2, 6, 3, 8, 2, 4, None) < 0                  # NULL operands
    z = torch.zeros(64, device=DEV, dtype=torch.float64)
    p = z.data_ptr()
    assert lib.eamd_rnnt_default_step(p, None, *([p] * 18), 1, 2, 6, 3, 8, 1, 4, None) < 0           # k != min(W, V - 1)
    assert lib.eamd_rnnt_default_step(p, None, *([p] * 10), None, *([p] * 7), 1, 2, 6, 3, 8, 2, 4, None) < 0
    assert lib.eamd_scatter_rows(None, None, None, None, None, None, None, 1, None) < 0
    torch.cuda.synchronize()
    assert float(z.abs().sum()) == 0.0
    assert ops.rnnt_default_step and ops.scatter_rows


# ---- 2. eamd_scatter_rows -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("njobs", [1, 16])
def test_scatter_rows_vs_index_assignment(njobs):
    """dst[idx[i]] = src[i] where mask[i]: widths with and without float4 moves, masks and no mask, indices outside dst ignored"""
    from espnet_amd import ops
    r = np.random.default_rng(njobs)
    jobs, want = [], []
    for j in range(njobs):
        width, rows, m = (7, 64, 12, 1)[j % 4], 5 + 3 * j, 1 + 2 * j
        dst = r.standard_normal((rows, width)).astype(np.float32)
        src = r.standard_normal((m, width)).astype(np.float32)
        idx = r.permutation(rows + 2)[:m].astype(np.int32) - 1                   # distinct; -1 and `rows` are outside
        mask = None if j % 3 == 0 else (r.random(m) < 0.6).astype(np.uint8)
        ref = dst.copy()
        for i in range(m):
            if 0 <= idx[i] < rows and (mask is None or mask[i]):
                ref[idx[i]] = src[i]
        want.append(ref)
        jobs.append(tuple(None if a is None else torch.from_numpy(a).to(DEV) for a in (dst, src, idx, mask)))
    ops.scatter_rows(jobs)
    torch.cuda.synchronize()
    for j, (job, ref) in enumerate(zip(jobs, want)):
        assert np.array_equal(job[0].cpu().numpy(), ref), j


# ---- 3. search vs float64 ----------------------------------------------------------------------------------------------------
T_S, E_S, D_S = 6, 6, 8
# (J, V, B, beam)
SEARCH_CASES = [(d, l, h) + shape for d, l, h in itertools.product(("lstm", "gru"), (1, 2), (12, 64))
                for shape in ((7, 6, 20, 3), (7, 6, 3, 2), (7, 6, 3, 8), (52, 257, 3, 4), (52, 257, 3, 8), (52, 257, 2, 16))]
P_S, BUDGET_S = 256, 8             # the class defaults, which the search tests do not change


def search_case(dtype, L, H, J, V, B, beam, seed):
    sd = seeded_weights(seed, dtype, L, H, E_S, J, V, D_S, {6: 4.0}.get(V, 8.0))
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((B, T_S, D_S)).astype(np.float32)
    hlens = r.integers(T_S // 2, T_S + 1, B)
    hlens[0], hlens[1] = T_S, 1
    if B > 2:
        hlens[2] = 2
    return sd, hs, hlens


@functools.lru_cache(maxsize=None)
def search_reference(dtype, L, H, J, V, B, beam, seed):
    sd, hs, hlens = search_case(dtype, L, H, J, V, B, beam, seed)
    W = min(beam, V)
    return default_batch64(weights_from_state_dict(sd), hs, hlens, beam, P_S, max_steps=BUDGET_S * W * int(max(hlens)))


def precondition(case, ref):
    """float64 alone: every ordering decision at least GAP apart, no frame above P and no utterance beyond the step budget"""
    return ref["min_gap"] >= GAP and not any(ref["overflow"])


@functools.lru_cache(maxsize=None)
def search_seed(dtype, L, H, J, V, B, beam):
    base = 31 * H + 7 * J + V + 1000 * L + 100000 * (dtype == "gru") + 17 * B + 1009 * beam
    for i in range(256):
        case = (dtype, L, H, J, V, B, beam)
        if precondition(case, search_reference(*case, base + 104729 * i)):
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
@pytest.mark.parametrize("dtype,L,H,J,V,B,beam", SEARCH_CASES)
def test_default_batch_vs_float64(dtype, L, H, J, V, B, beam):
    """default_batch on a seeded DecoderRNNT with ragged lengths (T, 1 and 2 among them) against the whole-search restatement: the
    same n-best lists in the same order, scores within 1e-4 relative, no overflow, the device's pop counts those of the restatement;
    precondition asserted"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    case = (dtype, L, H, J, V, B, beam)
    seed = search_seed(*case)
    ref = search_reference(*case, seed)
    assert precondition(case, ref), ("precondition: float64 decision gap, pops", ref["min_gap"], ref["overflow"])
    sd, hs, hlens = search_case(*case, seed)
    bs = BeamSearchTransducer(decoder=_decoder(sd, dtype, L, H, E_S, J, V, D_S), beam_size=beam)
    assert (bs.default_max_pops, bs.default_step_budget) == (P_S, BUDGET_S)
    got = bs.default_batch(torch.from_numpy(hs).to(DEV), [int(v) for v in hlens])
    assert len(got) == B and bs.overflowed == []
    worst = max(_same_nbest(g, w, (case, b)) for b, (g, w) in enumerate(zip(got, ref["nbest"])))
    assert [p[0] for p in bs.pops] == ref["total"] and [p[2] for p in bs.pops] == [max(p) for p in ref["pops"]]
    W = min(beam, V)
    print("[parity] default_batch %s x%d H=%d J=%d V=%d B=%d beam=%d: pops per frame mean %.2f W, max %.2f W, %d duplicates, %d long "
          "ahead lists, %d steps, %d host reads, min gap %.1e, score rel err %.2e"
          % (case + (sum(ref["total"]) / float(sum(hlens)) / W, max(max(p) for p in ref["pops"]) / float(W), ref["dups"],
                     ref["long_ahead"], bs.passes, bs.host_reads, ref["min_gap"], worst)))


@pytest.mark.gpu
def test_default_batch_utterance_without_frames():
    """hlens 0 beside a live utterance: [blank] with score 0, as list and as device tensor; the live one is what it is alone"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    sd = seeded_weights(9, "gru", 1, 12, E_S, 7, 6, D_S, 4.0)
    bs = BeamSearchTransducer(decoder=_decoder(sd, "gru", 1, 12, E_S, 7, 6, D_S), beam_size=3)
    hs = torch.randn(2, 5, D_S, generator=torch.Generator().manual_seed(3)).to(DEV)
    alone = bs.default_batch(hs[1:], [4])[0]
    for hlens in ([0, 4], torch.tensor([0, 4]).to(DEV)):
        got = bs.default_batch(hs, hlens)
        assert [(h.score, h.yseq) for h in got[0]] == [(0.0, [0])]
        _same_nbest(got[1], [(h.score, h.yseq) for h in alone], "beside an empty row")
    assert [(h.score, h.yseq) for h in bs.default_batch(hs[:1], [0])[0]] == [(0.0, [0])]


# ---- 4. fixtures -------------------------------------------------------------------------------------------------------------
_FIX = [("beam3", dict(beam_size=3, search_type="default")), ("beam3_nonorm", dict(beam_size=3, search_type="default", score_norm=False)),
        ("beam2", dict(beam_size=2))]


def _same_lists(got, want, what):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        _same_nbest(g, [(h.score, h.yseq) for h in w], (what, b))


@pytest.mark.gpu
@pytest.mark.parametrize("tag,kw", _FIX, ids=[c[0] for c in _FIX])
@pytest.mark.parametrize("name", ["transducer_rnn.npz", "transducer_gru.npz"])
def test_default_batch_vs_per_utterance_search_and_reference(name, tag, kw):
    """the fixture's three utterances with their valid lengths: default_batch (hlens as list, device tensor, None) and recognize_batch
    equal the per-utterance search element by element; utterance 0 equals the n-best list the reference recorded, where the fixture
    holds one"""
    from test_gpu_rnnt_greedy import _golden_model, _valid_lengths
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer, Hypothesis
    p, m = _golden_model(name)
    search = BeamSearchTransducer(decoder=m.dec, **kw)
    hs_pad = m.hs_pad.detach()
    hlens = _valid_lengths(m, p)
    assert max(hlens) == hs_pad.shape[1] and min(hlens) < max(hlens)
    one = [search(hs_pad[b, : hlens[b]]) for b in range(len(hlens))]
    got = search.default_batch(hs_pad, hlens)
    print("[parity] %s %s: pops (total, frames, most of a frame) %s, overflowed %s, %d steps, %d host reads"
          % (name, tag, search.pops, search.overflowed, search.passes, search.host_reads))
    _same_lists(got, one, "ragged")
    _same_lists(search.default_batch(hs_pad, torch.tensor(hlens).to(DEV)), one, "tensor hlens")
    _same_lists(search.default_batch(hs_pad), [search(hs_pad[b]) for b in range(len(hlens))], "hlens=None: whole padded rows")
    if "dec_%s_lens" % tag in p:
        lens, want, flat = (p["dec_%s_%s" % (tag, key)].tolist() for key in ("lens", "scores", "yseq"))
        ref, o = [], 0
        for ln, sc in zip(lens, want):
            ref.append((sc, flat[o:o + ln]))
            o += ln
        _same_nbest(got[0], ref, "reference record")
    else:
        assert tag == "beam2"
    xs = [p["xs"][b, : int(p["ilens"][b])].numpy() for b in range(3)]
    nb = m.recognize_batch(xs, search)
    _same_lists([[Hypothesis(score=h["score"], yseq=h["yseq"]) for h in r] for r in nb], one, "recognize_batch")
    assert [h["yseq"] for h in nb[0]] == [h["yseq"] for h in m.recognize(xs[0], search)]


def _fallback_case(name, kw, precision=None):
    import espnet_amd
    from test_gpu_rnnt_greedy import _golden_model, _valid_lengths
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    p, m = _golden_model(name)
    search = BeamSearchTransducer(decoder=m.decoder if hasattr(m, "decoder") else m.dec, **kw)
    hs_pad = m.hs_pad.detach()
    hlens = _valid_lengths(m, p)
    calls = [0]
    inner = search._default

    def counted(h):
        calls[0] += 1
        return inner(h)
    search._default = counted
    if precision:
        espnet_amd.set_precision(precision)
    got = search.default_batch(hs_pad, hlens)
    assert calls[0] == len(hlens)                          # the per-utterance search ran, once per utterance
    one = [search(hs_pad[b, : hlens[b]]) for b in range(len(hlens))]
    assert [[h.yseq for h in g] for g in got] == [[h.yseq for h in g] for g in one]
    assert [[h.score for h in g] for g in got] == [[h.score for h in g] for g in one]


@pytest.mark.gpu
def test_default_batch_fallbacks():
    """a custom prediction network, beam_size 17, an LM and bf16 precision go through the per-utterance loop and return what it returns"""
    from espnet_amd.nets.lm import ClassifierWithState, RNNLM
    from conftest import load_golden, split_golden
    _fallback_case("transducer_tt.npz", dict(beam_size=3))
    _fallback_case("transducer_rnn.npz", dict(beam_size=17))
    p, _sd, _ = split_golden(load_golden("transducer_rnn.npz"))
    lm = ClassifierWithState(RNNLM(6, 1, 8, None, "lstm", 0.0))
    lm.load_state_dict({k[3:]: v for k, v in p.items() if k.startswith("lm/")})
    _fallback_case("transducer_rnn.npz", dict(beam_size=3, lm_weight=0.5, lm=lm.to(DEV).eval()))
    _fallback_case("transducer_rnn.npz", dict(beam_size=3), precision="bf16")


def _benign():
    case = ("lstm", 1, 12, 7, 6, 20, 3)
    seed = search_seed(*case)
    return case, search_reference(*case, seed), search_case(*case, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["default_max_pops", "default_step_budget"])
def test_default_batch_overflow_is_searched_again(knob):
    """default_max_pops = W: every utterance with a frame of more than W pops overflows; default_step_budget = 1: every utterance that
    needs more than W max(T_b) pops is cut off.  Either way it is searched again per utterance and the lists are the exact ones"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    case, ref, (sd, hs, hlens) = _benign()
    dtype, L, H, J, V, B, beam = case
    W = min(beam, V)
    bs = BeamSearchTransducer(decoder=_decoder(sd, dtype, L, H, E_S, J, V, D_S), beam_size=beam)
    setattr(bs, knob, W if knob == "default_max_pops" else 1)
    calls = [0]
    inner = bs._default

    def counted(h):
        calls[0] += 1
        return inner(h)
    bs._default = counted
    got = bs.default_batch(torch.from_numpy(hs).to(DEV), [int(v) for v in hlens])
    if knob == "default_max_pops":
        want = [b for b in range(B) if max(ref["pops"][b]) > W]
    else:
        want = [b for b in range(B) if ref["total"][b] > W * int(max(hlens))]
        assert bs.passes == W * int(max(hlens)) and bs.host_reads == 2
    assert want and bs.overflowed == want and calls[0] == len(want)
    for b, (g, w) in enumerate(zip(got, ref["nbest"])):
        _same_nbest(g, w, (knob, b))


# ---- 5. host reads -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,rows", [(3, 64), (7, 3)])
def test_default_batch_host_reads(B, rows, monkeypatch):
    """blocking device-to-host reads counted as test_nsc_batch_reads_the_host_once counts them: per chunk of utterances one read of
    the flags after the first W max(T_b) steps and one after every further default_chunk_steps - as many as the restatement's pop
    counts predict -, and one result copy per call (7 utterances in chunks of 3: 3 + 3 + 1)"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    T, beam, chunk = 6, 4, 5
    hlens = [T - (b % 3) for b in range(B)]
    for seed in range(5, 69):                              # the first seed whose float64 decisions are GAP apart, as in search_seed
        sd = seeded_weights(seed, "lstm", 1, 64, E_S, 52, 257, D_S, 8.0)
        hs = np.random.default_rng(seed + B).standard_normal((B, T, D_S)).astype(np.float32)
        ref = default_batch64(weights_from_state_dict(sd), hs, hlens, beam)
        if ref["min_gap"] >= GAP and not any(ref["overflow"]):
            break
    assert ref["min_gap"] >= GAP and not any(ref["overflow"])
    predicted, steps = 1, 0
    for b0 in range(0, B, rows):
        first = beam * max(hlens[b0:b0 + rows])
        more = max(0, max(ref["total"][b0:b0 + rows]) - first)
        assert first + more <= 8 * first
        predicted += 1 + -(-more // chunk)
        steps += first + -(-more // chunk) * chunk
    bs = BeamSearchTransducer(decoder=_decoder(sd, "lstm", 1, 64, E_S, 52, 257, D_S), beam_size=beam)
    bs.default_max_rows, bs.default_chunk_steps = rows, chunk
    hs_d = torch.from_numpy(hs).to(DEV)
    reads = [0]
    for meth in ("tolist", "item", "cpu", "numpy"):
        orig = getattr(torch.Tensor, meth)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                reads[0] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, meth, counted)
    got = bs.default_batch(hs_d, hlens)
    monkeypatch.undo()
    assert reads[0] == bs.host_reads == predicted, (reads[0], bs.host_reads, predicted)
    assert bs.passes == steps and bs.overflowed == []
    for b, (g, w) in enumerate(zip(got, ref["nbest"])):
        _same_nbest(g, w, ("chunks of %d" % rows, b))
