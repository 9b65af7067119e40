"""tests/rnnt_lm_restatement.py (the np.float32 restatement the GPU tests of RNN LM fusion in the batched alsd / tsd searches compare
against) pinned on the CPU:
  * the scalar rule, bit for bit, to the torch arithmetic BeamSearchTransducer._alsd / _tsd perform - `score + lp`,
    `+= lm_weight * torch.tensor(q, dtype=torch.float32)`, np.logaddexp on those tensors - for parents without and with labels;
    this settles how torch rounds lm_weight * q (the weight is rounded to float32, the product is one float32 multiply);
  * the whole searches to a per-utterance loop over hypothesis objects that carries scores exactly as _alsd / _tsd do (Python
    doubles until the first LM term, float32 0-d tensors after it), on seeded small models;
  * every search case of tests/test_gpu_rnnt_lm_fusion.py finds a seed that meets its decision-gap precondition."""
import numpy as np
import pytest
import torch

from rnnt_greedy_restatement import act64, pred_step64, seeded_weights, weights_from_state_dict
from rnnt_lm_restatement import (alsd_lm_batch, alsd_lm_step, lm_add, lm_ext, lm_key, lm_merge, lm_rows64, lm_weights_from_state_dict,
                                 log_softmax64, seeded_lm, tsd_lm_batch, tsd_lm_step)

f32 = np.float32
# np.logaddexp on 0-d tensors, as the searches call it: numpy 2 warns about torch's __array_wrap__ signature on every call
pytestmark = pytest.mark.filterwarnings("ignore:__array_wrap__:DeprecationWarning")


def _bits(x):
    return np.float64(float(x)).tobytes()


def _is32(x):
    """np.logaddexp on float32 0-d tensors: a float32 value (a tensor again through __array_wrap__, or a numpy scalar)"""
    return str(x.dtype).endswith("float32")


# ---- the scalar rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.1, 0.3, 0.5])
def test_scalar_rule_equals_torch_bit_for_bit(w):
    r = np.random.default_rng(int(w * 10))
    n = 3000
    lp = (-r.random(n) * 12).astype(f32)
    q = (-r.random(n) * 12).astype(f32)
    bl = (-r.random(n) * 3).astype(f32)
    root = -r.random(n) * 9                                   # a double: [blank] after some blank continuations
    for j in range(n):
        lpj, qj, blj = float(lp[j]), float(q[j]), float(bl[j])   # the record's float32 values as the host reads them (tolist)
        # u == 0: the parent's score is a Python double
        S = float(root[j])
        s = S + lpj
        s += w * torch.tensor(qj, dtype=torch.float32)
        assert s.dtype == torch.float32 and _bits(s) == _bits(lm_ext(S, 0, lp[j], q[j], w)), (j, "ext, u == 0")
        assert _bits(S + blj) == _bits(lm_add(S, 0, bl[j])), (j, "blank, u == 0")
        # u > 0: the parent's score is the float32 tensor an extension produced
        parent = s
        S32 = float(parent)
        t = parent + blj
        assert t.dtype == torch.float32 and _bits(t) == _bits(lm_add(S32, 1, bl[j])), (j, "blank, u > 0")
        e = parent + lpj
        e += w * torch.tensor(qj, dtype=torch.float32)
        assert e.dtype == torch.float32 and _bits(e) == _bits(lm_ext(S32, 1, lp[j], q[j], w)), (j, "ext, u > 0")
        # merges: float32 tensors (and what np.logaddexp made of them before) with u > 0, doubles with u == 0
        m = np.logaddexp(t, e)
        assert _is32(m) and _bits(m) == _bits(lm_merge(float(t), float(e), 2)), (j, "merge, u > 0")
        assert _bits(np.logaddexp(t, t)) == _bits(lm_merge(float(t), float(t), 2)), (j, "merge of equal scores")
        m2 = np.logaddexp(m, parent)                          # what np.logaddexp returned with a tensor
        assert _is32(m2) and _bits(m2) == _bits(lm_merge(float(m), S32, 2)), (j, "merge of a merged score")
        t2 = m + blj                                          # a merged score goes on in float32
        assert _bits(t2) == _bits(lm_add(float(m), 2, bl[j])), (j, "blank after a merge")
        assert _bits(np.logaddexp(S, S + blj)) == _bits(lm_merge(S, S + blj, 0)), (j, "merge, u == 0")
        # the n-best key
        assert _bits(e / 3) == _bits(lm_key(float(e), 3, True)) and _bits(m / 4) == _bits(lm_key(float(m), 4, True)), (j, "key")
        assert _bits(S / 1) == _bits(lm_key(S, 1, True)) and lm_key(float(e), 3, False) == float(e)


def test_the_product_is_rounded_before_the_sum():
    """values at which a fused multiply-add, a double product or a double weight would give another float32"""
    r = np.random.default_rng(7)
    fused = dbl_w = 0
    for _ in range(4000):
        S, lp, q = f32(-r.random() * 9), f32(-r.random() * 9), f32(-r.random() * 9)
        for w in (0.1, 0.3):
            want = lm_ext(float(S), 1, lp, q, w)
            base = f32(S) + f32(lp)
            fused += float(f32(float(base) + float(f32(w)) * float(q))) != want       # one rounding of the exact sum
            dbl_w += float(f32(base + f32(w * float(q)))) != want                     # the weight kept as a double
            t = torch.tensor(float(S), dtype=torch.float32) + float(lp)
            t += w * torch.tensor(float(q), dtype=torch.float32)
            assert _bits(t) == _bits(want)
    assert fused > 0 and dbl_w > 0, (fused, dbl_w)            # the test can tell them apart


# ---- the whole searches ---------------------------------------------------------------------------------------------------------
class _H:
    def __init__(self, score, yseq):
        self.score, self.yseq = score, yseq


class _Nets:
    """prediction network, LM and joint network in float64 per label sequence, the rows rounded to float32 as the search reads them"""

    def __init__(self, w, lmw, act="tanh"):
        self.w, self.lmw, self.act, self.cache = w, lmw, act, {}

    def _top(self, net, yseq, name):
        key = (name, tuple(yseq))
        if key not in self.cache:
            L, H = len(net["layers"]), net["layers"][0][1].shape[1]
            st = (np.zeros((L, 1, H)), np.zeros((L, 1, H)))
            for t in yseq:
                st = pred_step64(net, np.array([t]), st, np.ones(1, bool))
            self.cache[key] = st[0][-1]
        return self.cache[key]

    def rows(self, enc_t, yseq, k):
        """-> (blank logp, [(logp, token, raw LM logp)] * k best non-blank) as Python floats holding float32 values"""
        w = self.w
        d = self._top(w, yseq, "pred") @ w["lin_dec_w"].T
        logp = log_softmax64(act64(enc_t[None, :] + d, self.act) @ w["lin_out_w"].T + w["lin_out_b"])[0]
        lm = lm_rows64(self.lmw, self._top(self.lmw, yseq, "lm"))[0]
        order = np.argsort(-logp[1:], kind="stable")[:k] + 1
        return float(f32(logp[0])), [(float(f32(logp[t])), int(t), float(f32(lm[t]))) for t in order]


def _nbest(hyps, score_norm):
    if score_norm:
        hyps = sorted(hyps, key=lambda x: x.score / len(x.yseq), reverse=True)
    else:
        hyps = sorted(hyps, key=lambda x: x.score, reverse=True)
    return [(float(x.score), x.yseq) for x in hyps]


def reference_alsd_lm(nets, h, beam_size, u_max_arg, lm_weight, score_norm=True):
    """BeamSearchTransducer._alsd with an LM on one utterance's encoder states h [T, D_enc], on hypothesis objects"""
    w = nets.w
    V = w["lin_out_w"].shape[0]
    beam = min(beam_size, V)
    k = min(beam, V - 1)
    T = h.shape[0]
    u_max = min(u_max_arg, T - 1)
    enc = np.asarray(h, np.float64) @ w["lin_enc_w"].T + w["lin_enc_b"]
    B = [_H(0.0, [0])]
    final = []
    for i in range(T + u_max):
        B_, ts = [], []
        for b in B:
            t = i - (len(b.yseq) - 1) + 1
            if t > T - 1:
                continue
            B_.append(b)
            ts.append(t)
        if not B_:
            continue
        A = []
        for b, t in zip(B_, ts):
            blank_lp, ext = nets.rows(enc[t], b.yseq, k)
            nb = _H(b.score + blank_lp, b.yseq)
            A.append(nb)
            if t == T - 1:
                final.append(nb)
            for lp, tok, q in ext:
                s = b.score + lp
                s += lm_weight * torch.tensor(q, dtype=torch.float32)
                A.append(_H(s, b.yseq + [tok]))
        B = sorted(A, key=lambda x: x.score, reverse=True)[:beam]
        seen = []
        for b in B:
            if b.yseq in [f.yseq for f in seen]:
                f = seen[[f.yseq for f in seen].index(b.yseq)]
                f.score = np.logaddexp(f.score, b.score)
            else:
                seen.append(b)
    if final:
        return _nbest(final, score_norm)
    return [(float(x.score), x.yseq) for x in B]


def reference_tsd_lm(nets, h, beam_size, max_sym_exp, lm_weight, score_norm=True):
    """BeamSearchTransducer._tsd with an LM on one utterance's encoder states h [T, D_enc], on hypothesis objects"""
    w = nets.w
    V = w["lin_out_w"].shape[0]
    beam = min(beam_size, V)
    k = min(beam, V - 1)
    enc = np.asarray(h, np.float64) @ w["lin_enc_w"].T + w["lin_enc_b"]
    B = [_H(0.0, [0])]
    for t in range(h.shape[0]):
        A = []
        C = B
        for _v in range(max_sym_exp):
            rows = [nets.rows(enc[t], c.yseq, k) for c in C]
            seq_A = [a.yseq for a in A]
            for c, (blank_lp, _ext) in zip(C, rows):
                if c.yseq not in seq_A:
                    A.append(_H(c.score + blank_lp, c.yseq))
                else:
                    a = A[seq_A.index(c.yseq)]
                    a.score = np.logaddexp(a.score, c.score + blank_lp)
            D = []
            for c, (_b, ext) in zip(C, rows):
                for lp, tok, q in ext:
                    s = c.score + lp
                    s += lm_weight * torch.tensor(q, dtype=torch.float32)
                    D.append(_H(s, c.yseq + [tok]))
            C = sorted(D, key=lambda x: x.score, reverse=True)[:beam]
        B = sorted(A, key=lambda x: x.score, reverse=True)[:beam]
    return _nbest(B, score_norm)


def _case(seed, dtype, L, V, typ, lm_layers, units, n, T):
    sd = seeded_weights(seed, dtype, L, 12, 6, 7, V, 8, {2: 0.0, 6: 2.0}.get(V, 4.0))
    lsd = seeded_lm(seed + 2, typ, lm_layers, units, V)
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((n, T, 8)).astype(np.float32)
    hlens = r.integers(3, T + 1, n)
    hlens[0], hlens[-1] = T, 1
    if n > 2:
        hlens[1] = 2
    return weights_from_state_dict(sd), lm_weights_from_state_dict(lsd), hs, hlens


def _equal(got, want, what):
    assert [y for _s, y in got] == [y for _s, y in want], (what, got, want)
    for (s, _y), (s_ref, _y2) in zip(got, want):
        assert _bits(s) == _bits(s_ref), (what, s, s_ref)     # the same float32 operations in the same order


_NETS = [("lstm", 1, 6, "lstm", 1, 8), ("gru", 2, 6, "gru", 2, 8), ("lstm", 2, 40, "lstm", 2, 16), ("gru", 1, 2, "lstm", 1, 8)]


@pytest.mark.parametrize("dtype,L,V,typ,lm_layers,units", _NETS)
@pytest.mark.parametrize("beam,u_max,score_norm,lm_weight", [(2, 4, False, 0.5), (3, 20, True, 0.3), (8, 5, True, 0.1)])
def test_alsd_lm_batch_equals_the_per_utterance_loop(dtype, L, V, typ, lm_layers, units, beam, u_max, score_norm, lm_weight):
    w, lmw, hs, hlens = _case(3 + beam, dtype, L, V, typ, lm_layers, units, 5, 9)
    got = alsd_lm_batch(w, lmw, hs, hlens, beam, u_max, lm_weight, score_norm)
    nets = _Nets(w, lmw)
    for b in range(len(hlens)):
        _equal(got["nbest"][b], reference_alsd_lm(nets, hs[b, :hlens[b]], beam, u_max, lm_weight, score_norm), b)
    assert got["no_final"] >= 1 and got["finals"] > 0 and got["min_gap"] >= 0


@pytest.mark.parametrize("dtype,L,V,typ,lm_layers,units", _NETS)
@pytest.mark.parametrize("beam,M,score_norm,lm_weight", [(2, 3, False, 0.5), (3, 2, True, 0.3), (8, 1, True, 0.1), (3, 4, True, 0.5)])
def test_tsd_lm_batch_equals_the_per_utterance_loop(dtype, L, V, typ, lm_layers, units, beam, M, score_norm, lm_weight):
    w, lmw, hs, hlens = _case(5 + beam, dtype, L, V, typ, lm_layers, units, 5, 7)
    got = tsd_lm_batch(w, lmw, hs, hlens, beam, M, lm_weight, score_norm)
    nets = _Nets(w, lmw)
    for b in range(len(hlens)):
        _equal(got["nbest"][b], reference_tsd_lm(nets, hs[b, :hlens[b]], beam, M, lm_weight, score_norm), b)
    assert got["min_gap"] >= 0


def test_merges_in_float32_happen():
    """the searches above would not tell a double merge from a float32 one if none happened"""
    tot = 0
    for beam, M in ((3, 2), (8, 3)):
        w, lmw, hs, hlens = _case(5 + beam, "lstm", 1, 6, "lstm", 1, 8, 5, 7)
        tot += tsd_lm_batch(w, lmw, hs, hlens, beam, M, 0.3)["merges32"]
        tot += alsd_lm_batch(w, lmw, hs, hlens, beam, 5, 0.3)["merges32"]
    assert tot > 0


def test_one_step_on_a_hand_made_step():
    """alsd: [0, 3] by blank (u = 1: float32) meets [0] + 3 (u = 0: a double sum, then the float32 LM term); the first occurrence
    grows by the float32 logaddexp, the duplicate keeps its score.  tsd: the same pair in A"""
    from alsd_restatement import new_finals, new_state
    import tsd_restatement as ts
    n, W, V, T, u_max, k, w = 1, 3, 6, 4, 3, 3, 0.3
    st = new_state(n, W, T, u_max)
    st["nhyp"][0] = 2
    st["ulen"][0] = [1, 0, 0]
    st["yseq"][0, 0, :2] = [0, 3]
    st["score"][0] = [float(f32(-1.1)), -1.5000000001, 0.0]
    rec = np.full((3, 1 + 3 * k), -9.0, f32)
    rec[:, k + 1:2 * k + 1] = [3, 2, 4]
    rec[0, 0] = -0.3
    rec[1, 1], rec[1, 2 * k + 1] = -0.7, -0.9
    out, fo, par, tok, live, _frame, _act, merged = alsd_lm_step(rec, None, st, new_finals(n, W, u_max), V, T, u_max, 1, w)
    first = float(f32(-1.1) + f32(-0.3))
    second = float(f32(-1.5000000001 + float(f32(-0.7))) + f32(0.3) * f32(-0.9))
    assert out["score"][0, 1] == second and out["score"][0, 0] == float(np.logaddexp(f32(first), f32(second)))
    assert merged["score"][0].tolist() == [True, False, False] and par.tolist() == [0, 1, 1] and live.tolist() == [0, 1, 0]
    M = 2
    bst, A = ts.new_state(n, W, T, M), ts.new_a(n, W, M)
    bst["count"][1, 0], bst["ulen"][1, 0, 0], bst["score"][1, 0, 0] = 1, 1, second
    bst["yseq"][1, 0, 0, :2] = [0, 3]
    bst["count"][0, 0], bst["ulen"][0, 0, 0], bst["score"][0, 0, 0] = 1, 1, float(f32(-1.1))
    bst["yseq"][0, 0, 0, :2] = [0, 3]
    A["nA"][0], A["score"][0, 0], A["src"][0, 0] = 1, first, 0
    s2, A2, par, _tok, _live, merged = tsd_lm_step(rec, None, bst, A, V, T, M, 0, 1, 0, w)
    grown = float(np.logaddexp(f32(first), f32(second) + f32(-0.3)))
    assert A2["nA"][0] == 1 and A2["score"][0, 0] == grown and merged["a"][0, 0]
    assert s2["count"][2, 0] == 1 and s2["score"][2, 0, 0] == grown and merged["score"][0, 0] and par[0] == 0


def test_every_gpu_search_case_finds_a_seed():
    """the deterministic seed search of tests/test_gpu_rnnt_lm_fusion.py, run with the restatement alone"""
    import test_gpu_rnnt_lm_fusion as g
    cases = g.SEARCH_CASES + [c for c, _rows in g.CHUNK_CASES]
    for col, vals in enumerate([("alsd", "tsd"), ("lstm", "gru"), (1, 2), (6, 40), (1, 3, 5), (2, 3, 8), (1, 2, 3, 10), (True, False),
                                tuple(g.LMS), (0.5, 0.3)]):
        assert {c[col] for c in cases} == set(vals), col
    for kind, args in (("alsd", (2, 10)), ("tsd", (1, 2, 3))):
        assert {c[6] for c in g.SEARCH_CASES if c[0] == kind} == set(args)
        assert {c[8] for c in g.SEARCH_CASES if c[0] == kind} == set(g.LMS)
    merges32 = 0
    for case in cases:
        seed = g.search_seed(*case)
        ref = g.search_reference(*case, seed)
        assert ref["min_gap"] >= g.GAP
        merges32 += ref["merges32"]
    assert merges32 > 0
