"""n-gram LM shallow fusion on the GPU: eamd_ngram_score against the back-off definition in float64 (tests/test_ngram.py), the
scorer interfaces against each other, and BeamSearch / BatchBeamSearch with the n-gram scorer - device loop, host loop and the
host loop with a pure-Python scorer built on the float64 definition."""
import argparse
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_ngram import (ARPA_BEAM, ARPA_TEST, all_contexts, arpa_dict, check_contexts, definition, fixture_tokens, table_walk,
                        write_random_arpa)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4                                   # of test_decode_fusion_golden: scores to TOL * max(1, |s|)
TOKENS30 = ["<blank>", "<unk>", "a", "e", "i", "o", "u"] + ["t%d" % i for i in range(7, 29)] + ["<eos>"]


def _launch(lm, ctx_prev, toks, first=False):
    """one launch; the newest tokens travel as the last column of an int64 prefix matrix (a strided view, no copy)"""
    from espnet_amd import ops
    n = len(toks)
    ys = torch.full((n, 3), 7, dtype=torch.int64)
    ys[:, -1] = torch.as_tensor(toks, dtype=torch.int64)
    ys = ys.to(DEV)
    col = ys[:, -1]
    assert n == 1 or col.stride(0) == 3
    cp = torch.as_tensor(np.asarray(ctx_prev, dtype=np.int32).reshape(n, lm.order - 1)).to(DEV)
    logp, ctx_new = ops.ngram_score(lm, cp, col, first=first)
    torch.cuda.synchronize()
    assert logp.shape == (n, lm.uni_tok.numel()) and logp.dtype == torch.float32 and ctx_new.dtype == torch.int32
    return logp.cpu().numpy(), ctx_new.cpu().numpy()


def _token_of(lm):
    """word id -> one token id that reads it"""
    out = {}
    for t, w in enumerate(lm.tok2word.cpu().tolist()):
        out.setdefault(w, t)
    return out


@pytest.mark.parametrize("path", [ARPA_TEST, ARPA_BEAM])
def test_kernel_fixture_all_contexts(path):
    """every context (c0, c1) of length 1 and 2 over every word: c0 as the newest token (as the <s> of the first-step flag where
    c0 = <s>, which no token reads), c1 from ctx_prev, whose last slot falls out"""
    from espnet_amd.nets.ngram import ArpaLM
    toks = fixture_tokens(path)
    lm = ArpaLM(path, toks).to(DEV)
    grams, _ = arpa_dict(path)
    tok_of = _token_of(lm)
    ctxs = [c for c in all_contexts(lm, 2) if c[0] >= 0]
    plain = [c for c in ctxs if c[0] != lm.bos]
    first = [c for c in ctxs if c[0] == lm.bos]
    assert len(plain) + len(first) == len(lm.words) + len(lm.words) ** 2 and all(c[0] in tok_of for c in plain)
    rnd = random.Random(1)
    for group, flag in ((plain, False), (first, True)):
        prev = [(c[1], rnd.randrange(len(lm.words))) for c in group]                 # the oldest slot is dropped
        newest = [rnd.randrange(len(toks)) if flag else tok_of[c[0]] for c in group]
        rows, ctx_new = _launch(lm, prev, newest, first=flag)
        assert ctx_new.tolist() == [list(c) for c in group]
        worst = check_contexts(lm, grams, rows, group)
        for r, c in zip(rows, group):                                                # and bit for bit the numpy walk over the tables
            assert np.array_equal(r, table_walk(lm, c)), c
        print("[ngram] %s first=%s: %d contexts, worst error / bound %.3f" % (os.path.basename(path), flag, len(group), worst))


_RANDOM = {}


def _random_lm(tmp_path_factory, V):
    if V not in _RANDOM:
        from espnet_amd.nets.ngram import ArpaLM
        path = str(tmp_path_factory.mktemp("ngram") / ("r4_%d.arpa" % V))
        toks = write_random_arpa(path, 4, V - 6, min(3000, 12 * V), seed=V, n_tokens=V)
        _RANDOM[V] = (ArpaLM(path, toks).to(DEV), arpa_dict(path)[0], toks)
    return _RANDOM[V]


@pytest.mark.parametrize("n", [1, 3, 320])
@pytest.mark.parametrize("V", [37, 64, 5000])
def test_kernel_random_four_gram(tmp_path_factory, V, n):
    """a seeded random 4-gram model; V = 37: scalar stores and rows that are not 16-byte aligned, 64 and 5000: 16-byte stores.
    The rows cycle through: a depth-3 match, an empty slot, out-of-range token ids (either side), <unk> in the context, a miss
    at depth 1, random words."""
    lm, grams, toks = _random_lm(tmp_path_factory, V)
    assert lm.order == 4 and len(toks) == V
    tok_of = _token_of(lm)
    rnd = random.Random(100 * V + n)
    W = len(lm.words)
    wid = lambda g: [lm.words[w] for w in g]                                        # noqa: E731
    tri = sorted({h[:3] for h in grams if len(h) == 4})                             # contexts that a listed 4-gram extends
    bigrams = {tuple(wid(h)) for h in grams if len(h) == 2}
    uni = [lm.words[w] for w in lm.words if w not in ("<s>", "</s>", "<unk>")]
    kinds = []
    for k in range(24):
        g = wid(rnd.choice(tri))
        a, b = rnd.choice(uni), rnd.choice(uni)
        while (b, a) in bigrams:                                                     # "b a" is not listed: the walk stops at depth 1
            b = rnd.choice(uni)
        kinds.append([(tok_of[g[2]], (g[1], g[0], rnd.choice(uni))),               # depth 3: the history ends in the trigram g
                      (tok_of[a], (-1, -1, -1)),                                    # empty slots
                      (V + rnd.randrange(9), (a, b, -1)),                           # token id past the vocabulary: <unk>
                      (-1 - rnd.randrange(9), (g[2], g[1], g[0])),                  # negative token id: <unk>
                      (tok_of[a], (lm.unk, b, a)),                                  # <unk> inside the context
                      (tok_of[a], (b, rnd.choice(uni), -1)),                        # miss at depth 1
                      (rnd.randrange(V), tuple(rnd.randrange(W) for _ in range(3)))][k % 7])
    rows_in = [kinds[r % len(kinds)] for r in range(n)]
    t2w = lm.tok2word.cpu().tolist()
    expect = [((t2w[t] if 0 <= t < V else lm.unk),) + tuple(c[:2]) for t, c in rows_in]
    rows, ctx_new = _launch(lm, [c for _, c in rows_in], [t for t, _ in rows_in])
    assert ctx_new.tolist() == [list(c) for c in expect]
    worst = check_contexts(lm, grams, rows, expect)
    walks = {}
    for r, c in zip(rows, expect):
        if c not in walks:
            walks[c] = table_walk(lm, c)
        assert np.array_equal(r, walks[c]), c
    depths = {_depth(lm, c) for c in walks}
    assert 3 in depths and (n < 7 or 1 in depths)
    print("[ngram] random 4-gram V=%d n=%d: %d distinct contexts, worst error / bound %.3f" % (V, n, len(walks), worst))


def _depth(lm, ctx):
    cs, cw, cn = lm.child_start.cpu().numpy(), lm.child_word.cpu().numpy(), lm.child_node.cpu().numpy()
    node, d = 0, 0
    for w in ctx:
        lo, hi = cs[node], cs[node + 1]
        p = lo + int(np.searchsorted(cw[lo:hi], w))
        if w < 0 or p >= hi or cw[p] != w:
            break
        node, d = int(cn[p]), d + 1
    return d


def test_first_step_flag_and_unigram_model(tmp_path):
    """first: the newest word is <s> whatever the token; an order-1 model has no context at all (N - 1 = 0 columns)"""
    from espnet_amd import ops
    from espnet_amd.nets.ngram import ArpaLM
    toks = fixture_tokens(ARPA_BEAM)
    lm = ArpaLM(ARPA_BEAM, toks).to(DEV)
    rows, ctx_new = _launch(lm, [(3, 4)] * 5, [0, 2, len(toks) - 1, 999, -5], first=True)
    assert ctx_new.tolist() == [[lm.bos, 3]] * 5 and all(np.array_equal(r, rows[0]) for r in rows)
    assert abs(float(rows[0][toks.index("a")]) - -0.4849466) <= 1e-6          # bigram <s> a
    p = tmp_path / "uni.arpa"
    p.write_text("\\data\\\nngram 1=4\n\n\\1-grams:\n-0.5\t<s>\n-1.5\t</s>\n-0.7\ta\n-2.5\t<unk>\n\n\\end\\\n")
    uni = ArpaLM(str(p), ["<blank>", "a", "<eos>"]).to(DEV)
    logp, ctx = ops.ngram_score(uni, torch.empty(2, 0, dtype=torch.int32, device=DEV), torch.tensor([1, 2], device=DEV))
    assert ctx.shape == (2, 0) and logp.cpu().tolist() == [[-2.5, float(np.float32(-0.7)), -1.5]] * 2


def test_scorer_interfaces_agree_bitwise():
    """score, batch_score, score_tree and NgramPartScorer.score_partial on the same prefixes: the same rows, bit for bit, and
    the literal sentence sums of the reference's test/test_ngram.py through the scorer"""
    from espnet_amd.nets.ngram import NgramFullScorer, NgramPartScorer
    toks = fixture_tokens(ARPA_TEST)
    full, part = NgramFullScorer(ARPA_TEST, toks), NgramPartScorer(ARPA_TEST, toks)
    x = torch.zeros(4, 8, device=DEV)
    g = torch.Generator().manual_seed(5)
    n, L = 6, 5
    ys = torch.cat([torch.full((n, 1), len(toks) - 1), torch.randint(0, len(toks), (n, L - 1), generator=g)], 1).to(DEV)
    assert full.batch_init_state(x) is None and part.init_state(x) is None
    tree, states, one, pstate = None, [None] * n, [None] * n, [None] * n
    ids = torch.arange(len(toks), device=DEV)
    for l in range(1, L + 1):
        lp_t, tree = full.score_tree(ys[:, :l], tree, x.expand(n, 4, 8))
        lp_b, st = full.batch_score(ys[:, :l], states, x.expand(n, 4, 8))
        assert torch.equal(lp_t, lp_b) and torch.equal(tree, st) and tree.shape == (n, 2) and tree.dtype == torch.int32
        for i in range(n):
            lp_1, one[i] = full.score(ys[i, :l], one[i], x)
            lp_p, pstate[i] = part.score_partial(ys[i, :l], ids, pstate[i], x)
            assert torch.equal(lp_1, lp_t[i]) and torch.equal(lp_p, lp_t[i]) and torch.equal(one[i], tree[i])
            sub = torch.tensor([3, 1, 3], device=DEV)
            assert torch.equal(part.score_partial(ys[i, :l], sub, None if l == 1 else states[i], x)[0], lp_t[i][sub])
        lp_pb, pst = part.score_partial_batch(ys[:, :l], ids.expand(n, -1)[:, :4], states, x)
        assert torch.equal(lp_pb, lp_t[:, :4]) and torch.equal(part.select_state(pst, (2, 1)), tree[2])
        states = [full.select_state(st, i) for i in range(n)]
    # a re-ordering as the device loop does it: index_select on the bare tensor
    from espnet_amd.nets.beam_search import BeamSearch
    idx = torch.tensor([5, 0, 0, 3, 1, 2], device=DEV)
    assert torch.equal(BeamSearch._tree_index(tree, idx), tree[idx])
    for words, want in ((["I", "like", "apple", "<eos>"], -1.04778921), (["you", "love", "coffee", "<eos>"], -1.18522948)):
        y, state, total = [len(toks) - 1], None, 0.0
        for w in words:
            lp, state = full.score(torch.tensor(y, device=DEV), state, x)
            total += float(lp[toks.index(w)])
            y.append(toks.index(w))
        assert abs(total - want) <= 1e-6, (words, total)


# ---- searches ---------------------------------------------------------------------------------------------------------------
def _def_scorer(path, tokens):
    """a pure-Python full scorer on the float64 definition (hypothesis by hypothesis, as the reference's scorer runs)"""
    from espnet_amd.nets.scorer_interface import ScorerInterface

    class DefinitionScorer(ScorerInterface):
        def __init__(self):
            self.grams, self.order = arpa_dict(path)
            self.words = ["</s>" if t == "<eos>" else t for t in tokens]
            self.rows = {}

        def init_state(self, x):
            return None

        def score(self, y, state, x):
            hist = ("<s>",) if len(y) == 1 else (state + (self.words[int(y[-1])],))
            hist = hist[-(self.order - 1):]
            if hist not in self.rows:
                self.rows[hist] = torch.tensor([definition(self.grams, self.order, hist, w)[0] for w in self.words],
                                               dtype=torch.float64).to(torch.float32).to(x.device)
            return self.rows[hist], hist

    return DefinitionScorer()


def _same_nbest(name, got, ref, nbest=3):
    assert [h.yseq.tolist() for h in got[:nbest]] == [h.yseq.tolist() for h in ref[:nbest]], name
    for a, b in zip(got[:nbest], ref[:nbest]):
        assert abs(float(a.score) - float(b.score)) <= TOL * max(1.0, abs(float(b.score))), (name, float(a.score), float(b.score))
        for k in b.scores:
            assert abs(float(a.scores[k]) - float(b.scores[k])) <= TOL * max(1.0, abs(float(b.scores[k]))), (name, k)


def _well_separated(ref, nbest=3):
    """neighbouring scores of the float64 side differ by more than twice the tolerance: otherwise the order is not defined"""
    s = [float(h.score) for h in ref[:nbest + 1]]
    assert len(s) >= nbest
    for a, b in zip(s, s[1:]):
        assert abs(a - b) > 2 * TOL * max(1.0, abs(a), abs(b)), s


def _three_way(name, mk, path, tokens, enc, ratio):
    """device loop, host loop and the host loop with the definition scorer -> the device loop's n-best"""
    from espnet_amd.nets.ngram import NgramFullScorer
    bs = mk(NgramFullScorer(path, tokens))
    assert bs._device_loop_ok(enc) and "ngram" in bs.full_scorers
    dev_nbest = bs(enc, maxlenratio=ratio)
    bs.device_loop = False
    host_nbest = bs(enc, maxlenratio=ratio)
    ref = mk(_def_scorer(path, tokens))
    assert not ref._device_loop_ok(enc)
    ref_nbest = ref(enc, maxlenratio=ratio)
    print("[parity] %s: device %s host %s definition %s" % (name, *[[round(float(h.score), 4) for h in x[:4]]
                                                                     for x in (dev_nbest, host_nbest, ref_nbest)]))
    _well_separated(ref_nbest)
    _same_nbest(name + " device loop", dev_nbest, ref_nbest)
    _same_nbest(name + " host loop", host_nbest, ref_nbest)
    return dev_nbest


def _fusion_setup():
    from test_gpu_model import _fusion_models
    p, model, lms = _fusion_models()
    with torch.no_grad():
        enc, _ = model.encode(p["speech"].unsqueeze(0).to(DEV), torch.tensor([p["speech"].shape[0]]))
    return model, lms, enc[0]


@pytest.mark.parametrize("batch", [False, True])
def test_search_with_ngram_fusion(batch):
    """BeamSearch / BatchBeamSearch with decoder + ctc 0.3 + length_bonus + ngram 0.5 on the V = 30 fusion model"""
    from espnet_amd.nets.batch_beam_search import BatchBeamSearch
    from espnet_amd.nets.beam_search import BeamSearch
    from espnet_amd.nets.ctc_prefix_score import CTCPrefixScorer, LengthBonus
    model, _, enc = _fusion_setup()
    cls = BatchBeamSearch if batch else BeamSearch

    def mk(ngram, w=0.5):
        scorers = dict(decoder=model.decoder, ctc=CTCPrefixScorer(model.ctc, model.eos), length_bonus=LengthBonus(30), ngram=ngram)
        return cls(scorers, dict(decoder=0.7, ctc=0.3, length_bonus=0.1, ngram=w), 4, 30, model.sos, model.eos, pre_beam_score_key="full")

    assert len(TOKENS30) == 30 and model.eos == 29
    with_ngram = _three_way(cls.__name__, mk, ARPA_BEAM, TOKENS30, enc, 0.0)
    from espnet_amd.nets.ngram import NgramFullScorer
    off = mk(NgramFullScorer(ARPA_BEAM, TOKENS30), w=0.0)
    assert "ngram" not in off.scorers
    without = off(enc)
    assert [h.yseq.tolist() for h in with_ngram[:3]] != [h.yseq.tolist() for h in without[:3]]      # the scorer acts


_WIDTH = {}


def _width_setup(tmp_path_factory):
    """the config-2 width model of tests/test_gpu_model.py (V = 5000) and a seeded random trigram model over its vocabulary"""
    if not _WIDTH:
        from test_gpu_model import c2width_setup
        _, model, _, encs = c2width_setup()
        path = str(tmp_path_factory.mktemp("ngram") / "tri5000.arpa")
        toks = write_random_arpa(path, 3, 4900, 6000, seed=11, n_tokens=5000)
        _WIDTH.update(model=model, enc=encs[2], path=path, toks=toks)
    return _WIDTH["model"], _WIDTH["enc"], _WIDTH["path"], _WIDTH["toks"]


def test_search_at_decode_width(tmp_path_factory):
    """V = 5000 (a multiple of 4: the candidate-selection kernels run), beam 10"""
    from espnet_amd.nets.beam_search import BeamSearch
    from espnet_amd.nets.ctc_prefix_score import CTCPrefixScorer, LengthBonus
    model, enc, path, toks = _width_setup(tmp_path_factory)

    def mk(ngram):
        scorers = dict(decoder=model.decoder, ctc=CTCPrefixScorer(model.ctc, model.eos), length_bonus=LengthBonus(5000), ngram=ngram)
        return BeamSearch(scorers, dict(decoder=0.7, ctc=0.3, length_bonus=0.1, ngram=0.5), 10, 5000, model.sos, model.eos,
                          pre_beam_score_key="full")

    bs = mk(None)
    C_ = dict(V=5000, beam=10, Tpad=int(enc.shape[0]), ctc=bs.part_scorers["ctc"], names=["decoder", "length_bonus", "ngram"])
    assert bs._step_plan(C_)[0]                                   # the candidate-selection path
    _three_way("decode width", mk, path, toks, enc, 0.2)


def test_forward_batch_and_step_graphs():
    """forward_batch of the four utterances of test_beam_search_batch_of_utterances = one search each (four full scorers:
    decoder, lm, length_bonus, ngram); with graph_steps the capturing and the replaying search equal the eager one.  The
    graphs run in a child process (tests/ngram_graph_check.py), as the other step-graph tests do."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "ngram_graph_check.py")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "[parity] ngram forward_batch and step graphs" in r.stdout


def test_recognize_plumbing(tmp_path_factory):
    """E2E.recognize / recognize_batch(..., ngram=scorer) = the direct search; build_ngram_scorer honours "full" and "part", and
    with "part" the search takes the host loop and matches the definition scorer"""
    from espnet_amd.nets.beam_search import BeamSearch, _recog_searcher
    from espnet_amd.nets.ctc_prefix_score import CTCPrefixScorer, LengthBonus
    from espnet_amd.nets.ngram import NgramFullScorer, NgramPartScorer, build_ngram_scorer
    from conftest import seeded_weights
    model, enc, path, toks = _width_setup(tmp_path_factory)
    xs = seeded_weights().decode_r4_inputs()
    ra = argparse.Namespace(beam_size=10, penalty=0.1, ctc_weight=0.3, maxlenratio=0.2, minlenratio=0.0, lm_weight=0.0, nbest=3,
                            ngram_weight=0.5, ngram_model=path, ngram_scorer="full")
    full = build_ngram_scorer(ra, toks)
    assert type(full) is NgramFullScorer
    scorers = dict(decoder=model.decoder, ctc=CTCPrefixScorer(model.ctc, model.eos), length_bonus=LengthBonus(5000), ngram=full)
    direct = BeamSearch(scorers, dict(decoder=0.7, ctc=0.3, length_bonus=0.1, ngram=0.5), 10, 5000, model.sos, model.eos,
                        pre_beam_score_key="full")(enc, maxlenratio=0.2)
    got = model.recognize(xs[2], ra, toks, ngram=full)
    assert [h["yseq"] for h in got] == [h.yseq.tolist() for h in direct[:3]]
    assert all(abs(a["score"] - float(b.score)) <= 1e-5 * max(1.0, abs(float(b.score))) for a, b in zip(got, direct))
    assert "ngram" in got[0]["scores"]
    both = model.recognize_batch([xs[2], xs[2][:200]], ra, toks, ngram=full)
    assert [h["yseq"] for h in both[0]] == [h["yseq"] for h in got]
    assert [h["yseq"] for h in both[1]] == [h["yseq"] for h in model.recognize(xs[2][:200], ra, toks, ngram=full)]
    assert "ngram" not in _recog_searcher(model, ra, None).scorers
    # "part": two partial scorers -> the host loop; the same row gathered at the pre-beam ids
    ra.ngram_scorer = "part"
    part = build_ngram_scorer(ra, toks)
    assert type(part) is NgramPartScorer
    bs = _recog_searcher(model, ra, None, part)
    assert "ngram" in bs.part_scorers and not bs._device_loop_ok(enc)
    host = bs(enc, maxlenratio=0.2)

    from espnet_amd.nets.scorer_interface import PartialScorerInterface
    inner = _def_scorer(path, toks)

    class PartDefinition(PartialScorerInterface):
        """the definition scorer as a partial scorer: its row at the requested ids"""

        def score_partial_batch(self, ys, ids, states, x=None):
            rows, sts = zip(*[inner.score(ys[i], states[i], ys) for i in range(len(states))])
            return torch.stack(rows).gather(1, ids.long()), list(sts)

        def select_state(self, state, i, new_id=None):
            return state[i[0]]

    ref = _recog_searcher(model, ra, None, PartDefinition())(enc, maxlenratio=0.2)
    _well_separated(ref)
    _same_nbest("part scorer, host loop", host, ref)
