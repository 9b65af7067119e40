"""RNN LM shallow fusion in the batched alsd / tsd transducer searches on the GPU: eamd_rnnt_alsd_step_lm / eamd_rnnt_tsd_step_lm
(csrc/rnnt_alsd.hip, csrc/rnnt_tsd.hip, the float32 rule of csrc/rnnt_search.h), ops.transducer_expand_rows_lm_dev and
BeamSearchTransducer.alsd_batch / tsd_batch / E2E.recognize_batch with lm=ClassifierWithState(RNNLM), lm_batched=True against
  * tests/rnnt_lm_restatement.py - np.float32 arithmetic, pinned to torch's by tests/test_rnnt_lm_restatement.py,
  * the per-utterance search of the same package with the same LM, and
  * the n-best lists the reference recorded with an LM (dec_alsd3_lm_*, dec_tsd3_lm_* of tests/golden/transducer_rnn.npz /
    transducer_gru.npz).
Step kernels: par, tok, live, frame, lengths, counts and sequences exact; a score no merge touched is a few IEEE float32 adds and one
multiply and must be BIT-EQUAL to the restatement (a contracted multiply-add would show); a merged score within four float32 ulps,
4 * 2**-23 * max(1, |want|): one for the device's rounding, up to three for expf, log1pf and the add of numpy's float32 logaddexp.
Searches: the same number of hypotheses, the same sequences in the same order, scores within 1e-4 * max(1, |s|) (the bound of
tests/test_gpu_transducer_search.py), `_fallback` patched to raise and ONE blocking device-to-host copy per call.  Equal sequences
are meaningful where float32 model arithmetic cannot flip an ordering decision, so every decision gap of the restatement (top-k
boundary of an active row, adjacent scores of the sorted lists down to position W + 1, adjacent keys of the final sort) must be
>= 1e-4; this precondition is ASSERTED, and each case takes the first seed of its own sequence that meets it on the CPU
(tests/test_rnnt_lm_restatement.py checks that every case finds one; the choice never looks at a GPU result)."""
import functools

import numpy as np
import pytest
import torch

from alsd_restatement import new_finals
from rnnt_greedy_restatement import seeded_weights, weights_from_state_dict
from rnnt_lm_restatement import (alsd_lm_batch, alsd_lm_step, lm_weights_from_state_dict, seeded_lm, tsd_lm_batch, tsd_lm_step)
from tsd_restatement import b_block

DEV = "cuda"
GAP = 1e-4
ULP4 = 4 * 2.0 ** -23


@pytest.fixture(autouse=True)
def _fp32():
    import espnet_amd
    espnet_amd.set_precision("fp32")
    yield
    espnet_amd.set_precision("fp32")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _check_scores(got, want, merged, what):
    """untouched scores bit-equal, merged ones within four float32 ulps -> the worst merged error in units of the bound"""
    got, want, merged = (np.asarray(x).reshape(-1) for x in (got, want, merged))
    plain = ~merged
    same = (_bits(got[plain]) == _bits(want[plain])) | (np.isnan(got[plain]) & np.isnan(want[plain]))
    assert same.all(), (what, got[plain][~same], want[plain][~same])
    worst = 0.0
    for g, w in zip(got[merged], want[merged]):
        err = 0.0 if g == w or (g != g and w != w) else abs(g - w) / (ULP4 * max(1.0, abs(w)))
        worst = max(worst, err)
        assert err <= 1.0, (what, g, w, err)
    return worst


def _lm_columns(r, rec, k, ties):
    """the record of width 1 + 2k with k raw LM log-probabilities behind it: on a grid of 1 / 4 with `ties`, else random"""
    q = -r.integers(1, 12, (len(rec), k)) / 4.0 if ties else -r.random((len(rec), k)) * 4.0 - 0.01
    return np.concatenate([rec, q.astype(np.float32)], 1)


def _as_f32(score, ulen):
    """with LM fusion the stored score of a hypothesis with labels holds a float32 value; [blank] (ulen == 0) keeps its full
    double, so that a float32 sum or merge on that path would show"""
    return np.where(ulen > 0, score.astype(np.float32).astype(np.float64), score)


# ---- 1. the step kernels vs the one-step restatement --------------------------------------------------------------------------
def _run_alsd(rec, hlens, st, fin, V, T, u_max, i, w):
    from espnet_amd import ops
    n, W = st["score"].shape
    s_in = tuple(_up(st[key]) for key in ("score", "ulen", "nhyp", "yseq"))
    s_out = (torch.full((n, W), 7.0, dtype=torch.float64, device=DEV), torch.full((n, W), -3, dtype=torch.int32, device=DEV),
             torch.full((n,), -3, dtype=torch.int32, device=DEV), torch.full(st["yseq"].shape, -3, dtype=torch.int32, device=DEV))
    f = tuple(_up(fin[key]) for key in ("score", "len", "yseq", "nfin"))
    par, frame = (torch.full((n * W,), -3, dtype=torch.int32, device=DEV) for _ in range(2))
    tok = torch.full((n * W,), -3, dtype=torch.int64, device=DEV)
    live = torch.full((n * W,), 9, dtype=torch.uint8, device=DEV)
    hl = None if hlens is None else _up(np.asarray(hlens, np.int32))
    ops.rnnt_alsd_step_lm(_up(np.asarray(rec, np.float32)), hl, s_in, s_out, f, par, tok, live, frame, V, T, u_max, i, w)
    torch.cuda.synchronize()
    out = dict(zip(("score", "ulen", "nhyp", "yseq"), (x.cpu().numpy() for x in s_out)))
    fo = dict(zip(("score", "len", "yseq", "nfin"), (x.cpu().numpy() for x in f)))
    return out, fo, par.cpu().numpy(), tok.cpu().numpy(), live.cpu().numpy(), frame.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n,W,V", [(n, W, V) for n in (1, 3) for W in (1, 2, 3, 8, 16) for V in (2, 3, 6, 40) if W <= V])
def test_alsd_step_lm_vs_restatement(n, W, V):
    """random states of steps early, late and past the end (tests/test_gpu_rnnt_alsd.py: _random_step - parents one label apart,
    nhyp < W in places, roots beside labelled slots), ragged hlens including 1 and 2; values on a grid of 1 / 4 with weight 0.5
    (ties) and random with weight 0.3; outputs poisoned beforehand"""
    from test_gpu_rnnt_alsd import _random_step
    T, u_max = 6, 3
    k = min(W, V - 1)
    r = np.random.default_rng(2000 * n + 10 * W + V)
    stats, worst = {}, 0.0
    for trial in range(8):
        i = int(r.integers(0, T + u_max + 1))
        ties = bool(trial & 1)
        w = 0.5 if ties else 0.3
        hlens = None if trial == 0 else r.choice([1, 2, T - 1, T], n).astype(np.int32)
        if trial == 1 and n == 3:
            hlens = np.array([1, 2, T], np.int32)
        rec, st, fin = _random_step(r, n, W, V, T, u_max, i, ties=ties)
        rec = _lm_columns(r, rec, k, ties)
        st["score"] = _as_f32(st["score"], st["ulen"])
        ws, wf, wpar, wtok, wlive, wframe, _act, merged = alsd_lm_step(rec, hlens, st, fin, V, T, u_max, i, w, stats)
        gs, gf, gpar, gtok, glive, gframe = _run_alsd(rec, hlens, st, fin, V, T, u_max, i, w)
        what = (n, W, V, i, trial)
        assert gs["nhyp"].tolist() == ws["nhyp"].tolist(), what
        assert gpar.tolist() == wpar.tolist() and gtok.tolist() == wtok.tolist(), what
        assert glive.tolist() == wlive.tolist() and gframe.tolist() == wframe.tolist(), what
        assert gf["nfin"].tolist() == wf["nfin"].tolist(), what
        for b in range(n):
            nh, nf = int(ws["nhyp"][b]), int(wf["nfin"][b])
            assert gs["ulen"][b, :nh].tolist() == ws["ulen"][b, :nh].tolist(), what
            for m in range(nh):
                u = int(ws["ulen"][b, m])
                assert gs["yseq"][b, m, :u + 1].tolist() == ws["yseq"][b, m, :u + 1].tolist(), what
            worst = max(worst, _check_scores(gs["score"][b, :nh], ws["score"][b, :nh], merged["score"][b, :nh], what))
            assert gf["len"][b, :nf].tolist() == wf["len"][b, :nf].tolist(), what
            for q in range(nf):
                ln = int(wf["len"][b, q])
                assert gf["yseq"][b, q, :ln].tolist() == wf["yseq"][b, q, :ln].tolist(), what
            worst = max(worst, _check_scores(gf["score"][b, :nf], wf["score"][b, :nf], merged["fin"][b, :nf], what))
    print("[parity] alsd_lm step n=%d W=%d V=%d: %d merges (%d in float32), %d dropped over 8 steps, worst merged score %.2f of the "
          "4-ulp bound" % (n, W, V, stats.get("merges", 0), stats.get("merges32", 0), stats.get("dropped", 0), worst))


_ST, _AK = ("score", "ulen", "count", "yseq"), ("score", "src", "nA")


def _run_tsd(rec, hlens, st, A, V, T, M, t, v, p, w):
    from espnet_amd import ops
    _blocks, n, W = st["score"].shape
    s, a = tuple(_up(st[key]) for key in _ST), tuple(_up(A[key]) for key in _AK)
    par = torch.full((n * W,), -3, dtype=torch.int32, device=DEV)
    tok = torch.full((n * W,), -3, dtype=torch.int64, device=DEV)
    live = torch.full((n * W,), 9, dtype=torch.uint8, device=DEV)
    hl = None if hlens is None else _up(np.asarray(hlens, np.int32))
    ops.rnnt_tsd_step_lm(_up(np.asarray(rec, np.float32)), hl, s, a, par, tok, live, V, T, M, t, v, p, w)
    torch.cuda.synchronize()
    return (dict(zip(_ST, (x.cpu().numpy() for x in s))), dict(zip(_AK, (x.cpu().numpy() for x in a))), par.cpu().numpy(),
            tok.cpu().numpy(), live.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("n,W,V", [(n, W, V) for n in (1, 3) for W in (1, 2, 3, 8, 16) for V in (2, 3, 6, 40) if W <= V])
def test_tsd_step_lm_vs_restatement(n, W, V):
    """M = 1, 2, 4, every pass v < M of random frames (tests/test_gpu_rnnt_tsd.py: _random_b, _random_rec - a random B in a random
    parity with [blank] beside labelled slots, slots one label apart so that merges happen, count < W in places; the passes before v
    run by the restatement), ragged hlens with finished utterances beside live ones; grid values with weight 0.5 and random ones
    with weight 0.3; blocks, A and the per-row outputs start as sentinels.  Every pass starts from the restatement's state, so a
    merged score's error does not travel"""
    from test_gpu_rnnt_tsd import _random_b, _random_rec, _sentinels
    T = 5
    k = min(W, V - 1)
    r = np.random.default_rng(3000 * n + 10 * W + V)
    stats, worst = {}, 0.0
    for M in (1, 2, 4):
        for trial in range(4):
            t, p, ties = int(r.integers(0, T)), int(r.integers(0, 2)), bool(trial & 1)
            w = 0.5 if ties else 0.3
            hlens = None if trial == 0 else r.choice([1, 2, T - 1, T], n).astype(np.int32)
            if trial == 1 and n == 3:
                hlens = np.array([t, t + 1, T], np.int32)          # finished, on its last frame, live
            st, A = _sentinels(n, W, T, M)
            _random_b(r, st, n, W, V, T, M, t, p, ties)
            st["score"] = _as_f32(st["score"], st["ulen"])
            for v in range(M):
                cin = b_block(M, p) if v == 0 else v
                cout = v + 1 if v < M - 1 else b_block(M, 1 - p)
                rec = _lm_columns(r, _random_rec(r, st, n, W, V, cin, ties), k, ties)
                ws, wa, wpar, wtok, wlive, merged = tsd_lm_step(rec, hlens, st, A, V, T, M, t, v, p, w, stats)
                gs, ga, gpar, gtok, glive = _run_tsd(rec, hlens, st, A, V, T, M, t, v, p, w)
                what = (n, W, V, M, t, v, p, trial)
                assert gpar.tolist() == wpar.tolist() and gtok.tolist() == wtok.tolist() and glive.tolist() == wlive.tolist(), what
                for key in ("ulen", "count", "yseq"):
                    assert np.array_equal(gs[key], ws[key]), (what, key)
                assert np.array_equal(ga["src"], wa["src"]) and np.array_equal(ga["nA"], wa["nA"]), what
                grown = np.zeros(ws["score"].shape, bool)
                grown[cout] = merged["score"]
                worst = max(worst, _check_scores(gs["score"], ws["score"], grown, what))
                worst = max(worst, _check_scores(ga["score"], wa["score"], merged["a"], what))
                st, A = ws, wa
    print("[parity] tsd_lm step n=%d W=%d V=%d: %d merges (%d in float32), %d truncated over 28 passes, worst merged score %.2f of "
          "the 4-ulp bound" % (n, W, V, stats.get("merges", 0), stats.get("merges32", 0), stats.get("truncated", 0), worst))


@pytest.mark.gpu
def test_step_lm_limits():
    """a non-finite lm_weight, more than 16 slots and a record of the width without LM terms are refused, nothing launched"""
    from alsd_restatement import new_state
    from espnet_amd import _lib
    import tsd_restatement as ts
    T, u_max, V, n, W, M = 4, 2, 40, 1, 3, 2
    k = min(W, V - 1)
    st, fin = new_state(n, W, T, u_max), new_finals(n, W, u_max)
    bst, A = ts.new_state(n, W, T, M), ts.new_a(n, W, M)
    for w in (float("nan"), float("inf")):
        with pytest.raises(_lib.EamdError):
            _run_alsd(np.zeros((n * W, 1 + 3 * k), np.float32), None, st, fin, V, T, u_max, 0, w)
        with pytest.raises(_lib.EamdError):
            _run_tsd(np.zeros((n * W, 1 + 3 * k), np.float32), None, bst, A, V, T, M, 0, 0, 0, w)
    with pytest.raises(_lib.EamdError):
        _run_alsd(np.zeros((n * W, 1 + 2 * k), np.float32), None, st, fin, V, T, u_max, 0, 0.5)
    with pytest.raises(_lib.EamdError):
        _run_tsd(np.zeros((n * W, 1 + 2 * k), np.float32), None, bst, A, V, T, M, 0, 0, 0, 0.5)
    st17, fin17 = new_state(n, 17, T, u_max), new_finals(n, 17, u_max)
    with pytest.raises(_lib.EamdError):
        _run_alsd(np.zeros((n * 17, 1 + 3 * 17), np.float32), None, st17, fin17, V, T, u_max, 0, 0.5)


# ---- 2. the record left on the device -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V", [6, 5000, 6145])
def test_expand_rows_lm_dev_equals_the_host_path(V):
    """byte-equal to what ops.transducer_expand_rows(..., lm=, lm_row=) reads back, with lm_row repeating and permuting rows"""
    from espnet_amd import ops
    from test_gpu_transducer_search import _rows
    n, n_lm = 5, 4
    x = _rows(V, n, V).to(DEV)
    lm = torch.log_softmax(torch.randn(n_lm, V, generator=torch.Generator().manual_seed(2)), -1).to(DEV)
    for k in (1, 3):
        for lm_row in ([3, 1, 1, 0, 3], [4 - 1 - i for i in range(4)] + [2]):
            rows, _ = ops.transducer_expand_rows(x, k, lm=lm, lm_row=lm_row)
            want = np.array([[bl] + [e[0] for e in ext] + [float(e[1]) for e in ext] + list(q) for bl, ext, q in rows], np.float32)
            idx = torch.tensor(lm_row, dtype=torch.int32).to(DEV)
            got = ops.transducer_expand_rows_lm_dev(x, k, lm, idx)
            assert got.is_cuda and tuple(got.shape) == (n, 1 + 3 * k)
            assert got.cpu().numpy().tobytes() == want.tobytes(), (V, k, lm_row)
            assert ops.transducer_expand_rows_lm_dev(x, k, lm, idx, in_range=True).cpu().numpy().tobytes() == want.tobytes()
    # an index the host path would refuse is clamped to lm's rows on the device
    far = torch.tensor([-7, 0, 1, 2, 99], dtype=torch.int32).to(DEV)
    near = torch.tensor([0, 0, 1, 2, n_lm - 1], dtype=torch.int32).to(DEV)
    assert (ops.transducer_expand_rows_lm_dev(x, 1, lm, far).cpu().numpy().tobytes()
            == ops.transducer_expand_rows_lm_dev(x, 1, lm, near).cpu().numpy().tobytes())


# ---- 3. the searches vs the per-utterance search with the same LM -------------------------------------------------------------
T_S, E_S, D_S, H_S, J_S = 8, 6, 8, 12, 7
LMS = {"lstm8": ("lstm", 1, 8), "lstm8x2": ("lstm", 2, 8), "lstm64": ("lstm", 1, 64), "lstm64x2": ("lstm", 2, 64),
       "gru16": ("gru", 1, 16), "gru8x2": ("gru", 2, 8)}
# (kind, prediction network, its layers, V, B, beam, u_max (alsd) / max_sym_exp (tsd), score_norm, LM, lm_weight): every value of
# every column, each LM variant in both searches
SEARCH_CASES = [
    ("alsd", "lstm", 1, 6, 1, 2, 2, True, "lstm8", 0.5),
    ("alsd", "gru", 2, 40, 3, 3, 10, False, "lstm64", 0.3),
    ("alsd", "lstm", 2, 40, 5, 8, 10, True, "gru16", 0.5),
    ("alsd", "gru", 1, 6, 5, 8, 2, True, "lstm64x2", 0.3),
    ("alsd", "lstm", 1, 40, 3, 2, 10, False, "lstm8x2", 0.5),
    ("alsd", "gru", 1, 6, 3, 3, 10, True, "gru8x2", 0.3),
    ("tsd", "lstm", 1, 6, 1, 2, 1, True, "lstm8", 0.5),
    ("tsd", "gru", 2, 40, 3, 3, 2, False, "lstm64", 0.3),
    ("tsd", "lstm", 2, 40, 5, 8, 3, True, "gru16", 0.5),
    ("tsd", "gru", 1, 6, 5, 8, 2, True, "lstm64x2", 0.3),
    ("tsd", "lstm", 1, 40, 3, 2, 3, False, "lstm8x2", 0.5),
    ("tsd", "gru", 1, 6, 3, 3, 2, True, "gru8x2", 0.3),
]
# (case, rows per loop): 5 utterances x 3 slots in chunks of 9 rows = 3 + 2 utterances
CHUNK_CASES = [(("alsd", "lstm", 1, 6, 5, 3, 10, True, "lstm64", 0.5), 9), (("tsd", "gru", 1, 40, 5, 3, 2, True, "lstm8", 0.3), 9)]


def search_case(kind, dtype, L, V, B, beam, arg, score_norm, lm, w, seed):
    sd = seeded_weights(seed, dtype, L, H_S, E_S, J_S, V, D_S, {6: 2.0}.get(V, 4.0))
    lsd = seeded_lm(seed + 2, *LMS[lm], V)
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((B, T_S, D_S)).astype(np.float32)
    hlens = r.integers(T_S // 2, T_S + 1, B)
    hlens[0] = T_S
    if B > 2:
        hlens[1], hlens[2] = 1, 2
    return sd, lsd, hs, hlens


@functools.lru_cache(maxsize=None)
def search_reference(kind, dtype, L, V, B, beam, arg, score_norm, lm, w, seed):
    sd, lsd, hs, hlens = search_case(kind, dtype, L, V, B, beam, arg, score_norm, lm, w, seed)
    run = alsd_lm_batch if kind == "alsd" else tsd_lm_batch
    return run(weights_from_state_dict(sd), lm_weights_from_state_dict(lsd), hs, hlens, beam, arg, w, score_norm)


@functools.lru_cache(maxsize=None)
def search_seed(kind, dtype, L, V, B, beam, arg, score_norm, lm, w):
    base = (7 * V + 1000 * L + 100000 * (dtype == "gru") + 17 * B + 3 * arg + 1009 * beam + 13 * sorted(LMS).index(lm)
            + 500000 * (kind == "tsd") + int(10 * w))
    for i in range(256):
        if search_reference(kind, dtype, L, V, B, beam, arg, score_norm, lm, w, base + 104729 * i)["min_gap"] >= GAP:
            return base + 104729 * i
    raise AssertionError("no seed meets the preconditions")


def _search(case, seed):
    """the case's BeamSearchTransducer on the GPU with its LM, the encoder states and the lengths"""
    from test_gpu_rnnt_alsd import _decoder
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    from espnet_amd.nets.lm import ClassifierWithState, RNNLM
    kind, dtype, L, V, B, beam, arg, score_norm, lm, w = case
    sd, lsd, hs, hlens = search_case(*case, seed)
    typ, layers, units = LMS[lm]
    net = ClassifierWithState(RNNLM(V, layers, units, None, typ, 0.0))
    net.load_state_dict({key[3:]: torch.from_numpy(v) for key, v in lsd.items()})
    kw = dict(u_max=arg) if kind == "alsd" else dict(max_sym_exp=arg)
    bs = BeamSearchTransducer(decoder=_decoder(sd, dtype, L, H_S, E_S, J_S, V, D_S), beam_size=beam, search_type=kind,
                              score_norm=score_norm, lm=net.to(DEV).eval(), lm_weight=w, lm_batched=True, **kw)
    return bs, torch.from_numpy(hs).to(DEV), [int(v) for v in hlens]


def _no_fallback(*a, **k):
    raise AssertionError("the device loop did not take this batch")


def _count_reads(monkeypatch, reads):
    """blocking device-to-host reads, counted as tests/test_gpu_rnnt_alsd.py counts them"""
    for meth in ("tolist", "item", "cpu", "numpy"):
        orig = getattr(torch.Tensor, meth)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                reads[0] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, meth, counted)


def _same_nbest(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    worst = 0.0
    for j, (g, h) in enumerate(zip(got, want)):
        assert list(g.yseq) == list(h.yseq), (what, j, g.yseq, h.yseq)
        err = abs(g.score - h.score) / max(1.0, abs(h.score))
        worst = max(worst, err)
        assert err <= 1e-4, (what, j, g.score, h.score)
    return worst


def _batched_vs_per_utterance(case, monkeypatch, rows=None):
    seed = search_seed(*case)
    ref = search_reference(*case, seed)
    assert ref["min_gap"] >= GAP, ("precondition: decision gap of the restatement", ref["min_gap"])
    bs, hs, hlens = _search(case, seed)
    kind = case[0]
    if rows is not None:
        setattr(bs, kind + "_max_rows", rows)
    one = [bs(hs[b, :hlens[b]]) for b in range(len(hlens))]
    monkeypatch.setattr(bs, "_fallback", _no_fallback)
    reads = [0]
    _count_reads(monkeypatch, reads)
    got = getattr(bs, kind + "_batch")(hs, hlens)
    monkeypatch.undo()
    assert reads[0] == 1, reads[0]
    assert len(got) == len(one)
    worst = max(_same_nbest(g, o, (case, b)) for b, (g, o) in enumerate(zip(got, one)))
    # the restatement chose the seed; it also names the sequences
    assert [[list(h.yseq) for h in g] for g in got] == [[y for _s, y in nb] for nb in ref["nbest"]], case
    print("[parity] %s_batch + LM %s: %d merges (%d in float32), min gap %.1e, score rel err %.2e"
          % (kind, case[1:], ref["merges"], ref["merges32"], ref["min_gap"], worst))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEARCH_CASES, ids=["-".join(str(v) for v in c) for c in SEARCH_CASES])
def test_lm_batch_vs_per_utterance_search(case, monkeypatch):
    """alsd_batch / tsd_batch with an RNN LM on seeded models with ragged lengths (T, 1 and 2 among them) against the per-utterance
    search with the same LM: the device loop takes the batch (`_fallback` raises), one blocking copy, the same n-best lists in the
    same order, scores within 1e-4 relative; gap precondition asserted"""
    _batched_vs_per_utterance(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case,rows", CHUNK_CASES, ids=[c[0][0] for c in CHUNK_CASES])
def test_lm_batch_in_two_chunks(case, rows, monkeypatch):
    """*_max_rows small enough to force two chunks: still one blocking copy and the per-utterance search's lists"""
    _batched_vs_per_utterance(case, monkeypatch, rows)


# ---- 4. the lists the reference recorded with an LM ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tag,kw", [("alsd3_lm", dict(beam_size=3, search_type="alsd", nstep=2, lm_weight=0.5)),
                                    ("tsd3_lm", dict(beam_size=3, search_type="tsd", nstep=2, lm_weight=0.5))])
@pytest.mark.parametrize("name", ["transducer_rnn.npz", "transducer_gru.npz"])
def test_recognize_batch_with_lm_vs_reference_record(name, tag, kw, monkeypatch):
    """E2E.recognize_batch with the fixture's RNNLM (the model built as _model of tests/test_gpu_transducer_search.py builds it): the
    device loop takes the batch; utterance 0 equals the n-best list the reference recorded, every utterance equals the per-utterance
    search on its rows of the batch's encoder states"""
    from dataclasses import asdict
    from test_gpu_rnnt_greedy import _valid_lengths
    from test_gpu_transducer_search import _decoder, _model
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    p, m, lm, _x = _model(name)
    search = BeamSearchTransducer(decoder=_decoder(m), lm=lm, lm_batched=True, **kw)
    xs = [p["xs"][b, : int(p["ilens"][b])].numpy() for b in range(3)]
    with torch.no_grad():
        m(p["xs"].to(DEV), p["ilens"], p["ys"].to(DEV))      # m.hs_pad: the padded encoder states of the batch in eval mode
    hs_pad, hlens = m.hs_pad.detach(), _valid_lengths(m, p)
    one = [[asdict(h) for h in search(hs_pad[b, :hlens[b]])] for b in range(3)]
    monkeypatch.setattr(search, "_fallback", _no_fallback)
    nb = m.recognize_batch(xs, search)
    monkeypatch.undo()
    lens, want, flat = (p["dec_%s_%s" % (tag, key)].tolist() for key in ("lens", "scores", "yseq"))
    assert len(nb[0]) == len(lens)
    o = 0
    for h, ln, sc in zip(nb[0], lens, want):
        assert h["yseq"] == flat[o:o + ln], (tag, h["yseq"], flat[o:o + ln])
        assert abs(h["score"] - sc) <= 1e-4 * max(1.0, abs(sc)), (tag, h["score"], sc)
        o += ln
    for b in range(3):
        assert [h["yseq"] for h in nb[b]] == [h["yseq"] for h in one[b]], (tag, b)
        for h, g in zip(nb[b], one[b]):
            assert abs(h["score"] - g["score"]) <= 1e-4 * max(1.0, abs(g["score"])), (tag, b)


# ---- 5. what still falls back ---------------------------------------------------------------------------------------------------
def _counted(search, name):
    """the per-utterance search `name` wrapped to keep what it returns"""
    inner, kept = getattr(search, name), []

    def counted(h):
        kept.append(inner(h))
        return kept[-1]
    setattr(search, name, counted)
    return kept


@pytest.mark.gpu
def test_lm_fallbacks():
    """what still loops over the per-utterance search and returns what it returns: nsc and default with the RNN LM; alsd / tsd
    with the RNN LM when the switch lm_batched is off (the default: with an LM they did so before); with the switch on, an LM in
    training mode with dropout and an LM that is no ClassifierWithState(RNNLM), a TransformerLM.  The TransformerLM case checks
    the ROUTING only: that LM has no `predict`, so the per-utterance search cannot run it at all (nor can the reference's), and
    there are no results to compare.  With dropout the LM's outputs are random: the lists must be the per-utterance loop's own"""
    import argparse
    from test_gpu_rnnt_greedy import _golden_model, _valid_lengths
    from test_gpu_transducer_search import _model
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    from espnet_amd.nets.lm import ClassifierWithState, RNNLM, TransformerLM
    _p, _m, lm, _x = _model("transducer_rnn.npz")
    p, m = _golden_model("transducer_rnn.npz")
    hs_pad, hlens = m.hs_pad.detach(), _valid_lengths(m, p)
    new = lambda kind, lm_, **kw: BeamSearchTransducer(decoder=m.dec, beam_size=3, search_type=kind, lm=lm_, lm_weight=0.5,      # noqa: E731
                                                       **kw)
    for kind, kw in (("nsc", dict(nstep=2)), ("default", {}), ("alsd", {}), ("tsd", {})):
        search = new(kind, lm, lm_batched=kind in ("nsc", "default"), **kw)
        assert not getattr(search, "_%s_batched_ok" % kind)()
        kept = _counted(search, "_" + kind)
        got = getattr(search, kind + "_batch")(hs_pad, hlens)
        assert len(kept) == len(hlens) and all(g is o for g, o in zip(got, kept))
        one = [search(hs_pad[b, :hlens[b]]) for b in range(len(hlens))]
        assert [[(h.yseq, h.score) for h in g] for g in got] == [[(h.yseq, h.score) for h in g] for g in one]
    noisy = ClassifierWithState(RNNLM(6, 1, 8, None, "lstm", 0.5))
    noisy.load_state_dict(lm.state_dict())
    noisy.to(DEV).train()
    tlm = TransformerLM(6, argparse.Namespace(pos_enc="none", embed_unit=8, att_unit=8, head=2, unit=16, layer=1,
                                              dropout_rate=0.0)).to(DEV).eval()
    for kind in ("alsd", "tsd"):
        assert new(kind, lm, lm_batched=True)._lm_batched_ok() and not new(kind, lm)._lm_batched_ok()
        for other in (noisy, tlm):
            search = new(kind, other, lm_batched=True)
            assert not search._lm_batched_ok() and not getattr(search, "_%s_batched_ok" % kind)()
            inner, asked, handed = search._fallback, [], []

            def spy(name, hs, hl, _inner=inner, _asked=asked, _handed=handed, _run=other is noisy):
                _asked.append((name, hl))
                _handed.append(_inner(name, hs, hl) if _run else ["per utterance"])
                return _handed[-1]
            search._fallback = spy
            got = getattr(search, kind + "_batch")(hs_pad, hlens)
            assert asked == [("_" + kind, hlens)] and got is handed[0]
            if other is noisy:
                assert len(got) == len(hlens) and all(isinstance(g, list) and g for g in got)
        noisy.eval()
        assert new(kind, noisy, lm_batched=True)._lm_batched_ok()      # the same LM in eval mode is taken
        noisy.train()
    for w in (float("nan"), float("inf")):
        assert not BeamSearchTransducer(decoder=m.dec, beam_size=3, search_type="alsd", lm=lm, lm_weight=w,
                                        lm_batched=True)._lm_batched_ok()
