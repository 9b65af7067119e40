"""CTC prefix beam search on the GPU (csrc/ctc_beam.hip through nets.ctc_prefix_beam): every hypothesis of an unpruned search
against the exact CTC sequence probability, pruned searches with and without an n-gram LM against the float64 restatement
(tests/ctc_prefix_beam_restatement.py), the n-gram point query against the row kernel, and the model-level entry points.

The restatement is fed the SAME fp32 log-posteriors converted to float64: the candidate sets are then identical by
construction and only near-ties at the beam's edge or inside the n-best could differ.  Every pruned case therefore first
asserts, on the restatement alone, that the smallest gap between the W-th and (W+1)-th ranked entry over all frames and the
smallest gap between neighbours of the final n-best are at least 100 x the case's score tolerance (the seeds were chosen for
this on the CPU).  Score tolerances: at most 4 x the largest |device - float64| measured on an MI355X, noted beside each."""
import argparse
import math

import pytest
import torch

from ctc_prefix_beam_restatement import ArpaDefinition, ctc_log_prob, peaked_posteriors, prefix_beam_search
from test_ngram import ARPA_BEAM, ARPA_TEST, fixture_tokens, write_random_arpa

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARPA = dict(test=ARPA_TEST, beam=ARPA_BEAM)
NGRAM_WEIGHT, PENALTY = 0.3, 0.5


def lm_tokens(path, V):
    """a token list of V entries over a fixture's words: <blank>, the words, tokens the file does not list (<unk>), <eos>"""
    words = fixture_tokens(path)[1:-2]
    assert V >= len(words) + 2
    return ["<blank>"] + words + ["x%d" % i for i in range(V - 2 - len(words))] + ["<eos>"]


def run_case(logp, hlens, W, K, nbest, lm=None, tol=None, label="", min_recreated=0):
    """logp fp32 [B, T, V] on the host.  The restatement per utterance (margins asserted against 100 x tol first), then the
    device search of the whole batch: sequences equal, scores within tol -> (largest |device - float64|, smallest margin).
    min_recreated: the restatement's node-id bookkeeping must see at least so many merges into a prefix whose parent string
    is in the beam under another id than the one it was created from (asserted before the device runs)"""
    from espnet_amd.nets.ctc_prefix_beam import CTCPrefixBeamSearch
    from espnet_amd.nets.ngram import ArpaLM
    B, T, V = logp.shape
    path = ARPA[lm] if lm else None
    toks = lm_tokens(path, V) if lm else None
    pen, w = (PENALTY, NGRAM_WEIGHT) if lm else (0.0, 0.0)
    definition = ArpaDefinition(path, toks) if lm else None
    want, margin, recreated = [], math.inf, 0
    for b in range(B):
        track = {}
        nb, m_beam, m_nbest = prefix_beam_search(logp[b, :hlens[b]].numpy(), W, K, nbest, pen, definition, w, track=track)
        want.append(nb)
        margin = min(margin, m_beam, m_nbest)
        recreated += track["recreated_parent_merges"]
    assert recreated >= min_recreated, "%s: %d re-created-parent merges in the restatement, %d wanted" % (label, recreated, min_recreated)
    if tol is not None:
        assert margin >= 100 * tol, "%s: margin %.2e of the inputs below 100 x tolerance %.1e: choose another seed" % (label, margin, tol)
    search = CTCPrefixBeamSearch(W, K, nbest, pen, ngram=ArpaLM(path, toks) if lm else None, ngram_weight=w)
    got = search.forward_batch(logp.to(DEV), hlens)
    worst = 0.0
    for b in range(B):
        assert [h["yseq"] for h in got[b]] == [[V - 1] + list(l) + [V - 1] for _, l, _ in want[b]], (label, b)
        worst = max([worst] + [abs(h["score"] - r[0]) for h, r in zip(got[b], want[b])])
    print("[ctc prefix beam] %s: largest |device - float64| %.3e, margin %.2e, re-created-parent merges %d"
          % (label, worst, margin, recreated))
    if tol is not None:
        assert worst <= tol, (label, worst, tol)
    return worst, margin


# ---- 1. nothing pruned: the exact sequence probability ----------------------------------------------------------------------
EXHAUSTIVE_TOL = 1.5e-6        # measured 4.5e-7


def test_exhaustive_against_the_forward_recursion():
    """B = 3, T = 4, V = 4, hlens (4, 3, 2), K = 2, W = 32: every label string over two tokens that fits into the frames (15 / 9 / 5
    of the 31 / 15 / 7 strings; the others have probability 0 and are never kept) is a hypothesis, and its score is the float64
    log p(y | x) of the CTC forward recursion.  Independent of the restatement."""
    from espnet_amd.nets.ctc_prefix_beam import CTCPrefixBeamSearch
    logp = torch.log_softmax(torch.randn(3, 4, 4, generator=torch.Generator().manual_seed(0)), dim=-1)
    hlens = [4, 3, 2]
    got = CTCPrefixBeamSearch(32, 2, 32).forward_batch(logp.to(DEV), hlens)
    worst = 0.0
    for b, (n, hl) in enumerate(zip((15, 9, 5), hlens)):
        seqs = [tuple(h["yseq"][1:-1]) for h in got[b]]
        assert len(seqs) == n == len(set(seqs)) and all(h["yseq"][0] == 3 == h["yseq"][-1] for h in got[b])
        assert all(c in (1, 2) for s in seqs for c in s)
        scores = [h["score"] for h in got[b]]
        assert scores == sorted(scores, reverse=True)
        for h, s in zip(got[b], seqs):
            worst = max(worst, abs(h["score"] - ctc_log_prob(logp[b, :hl].numpy(), s)))
    print("[ctc prefix beam] exhaustive: largest |device - float64 log p(y|x)| %.3e" % worst)
    assert worst <= EXHAUSTIVE_TOL


# ---- 2. pruned searches against the restatement --------------------------------------------------------------------------------
# name: (B, T, V, W, K, nbest, hlens, {lm: seed}, {lm: tolerance}).  Measured largest |device - float64| (none / test / beam) and
# the margins of the chosen seeds:
#   t60     6.7e-6 / 1.43e-5 / 6.6e-6    margins 4.1e-3 / 4.2e-3 / 7.9e-3
#   t33     1.8e-6 / 4.5e-6 / 2.1e-6     margins 1.9e-2 / 1.0e-2 / 1.3e-2
#   limits  1.23e-6 / 1.24e-6 / 1.01e-6  margins 3.1e-3 / 4.4e-3 / 3.0e-3   (W = K = 32, both limits of the kernel)
#   w1      9.7e-7 / 1.38e-6 / 1.23e-6   margins 1.1e-1 / 2.5e-1 / 1.9e-1
CASES = {
    "t60": (3, 60, 30, 8, 6, 4, (60, 41, 1), dict(none=178, test=59, beam=25), dict(none=2.5e-5, test=4e-5, beam=2.5e-5)),
    "t33": (2, 33, 12, 5, 3, 5, (33, 20), dict(none=1, test=5, beam=0), dict(none=7e-6, test=1.5e-5, beam=8e-6)),
    "limits": (2, 20, 40, 32, 32, 4, (20, 13), dict(none=56, test=52, beam=48), dict(none=4.5e-6, test=4.5e-6, beam=4e-6)),
    "w1": (2, 25, 12, 1, 4, 1, (25, 9), dict(none=4, test=3, beam=3), dict(none=3.5e-6, test=5e-6, beam=4.5e-6)),
}


@pytest.mark.parametrize("lm", ["none", "test", "beam"])
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(name, lm):
    B, T, V, W, K, nbest, hlens, seeds, tols = CASES[name]
    logp = peaked_posteriors(seeds[lm], B, T, V)
    run_case(logp, list(hlens), W, K, nbest, None if lm == "none" else lm, tols[lm], "%s / %s" % (name, lm))


# ---- 3. a long utterance: arena growth, backtrace, fp32 drift ------------------------------------------------------------------
LONG_SEED, LONG_TOL = 14, 3.5e-5   # measured 9.0e-6; margin of seed 14: 2.8e-2


def test_long_input():
    """T = 700, V = 30, W = K = 10, a constant +8 on one class per frame"""
    logp = peaked_posteriors(LONG_SEED, 1, 700, 30, peak=8.0, constant=True)
    run_case(logp, [700], 10, 10, 10, None, LONG_TOL, "long")


# ---- 3b. merges that only the comparison of the parent chains finds ---------------------------------------------------------------
# A prefix that left the beam and is spelled again gets a second node id, while a longer prefix still in the beam remembers
# the first one; the extension of the re-created prefix must still merge into it, which the kernel finds by walking both
# parent chains (same_string in csrc/ctc_beam.hip).  W = K = 3 at T = 100 makes prefixes leave and return; the restatement
# counts, with the kernel's id bookkeeping, the merges that the parent-id test alone would miss, and each case must have
# some.  name: (peak, seed, lm, V, tolerance).  Measured largest |device - float64|, margin and merges counted (scores near -160
# over 100 flat frames, where one fp32 ulp is 1.5e-5):
#   peak2    2.81e-5   3.9e-3   3        flat6    9.0e-6   7.3e-3   2
#   flat21   2.86e-5   4.3e-3   2        beam_lm  4.7e-6   2.9e-3   1   (ngram_beam_search_test.arpa, weight 0.3, penalty 0.5)
RECREATED = {
    "peak2": (2.0, 1, "none", 5, 3.8e-5),
    "flat6": (0.0, 6, "none", 5, 3.5e-5),
    "flat21": (0.0, 21, "none", 5, 4.3e-5),
    "beam_lm": (2.0, 32, "beam", 10, 1.8e-5),
}


@pytest.mark.parametrize("name", list(RECREATED))
def test_merge_into_a_prefix_whose_parent_was_recreated(name):
    peak, seed, lm, V, tol = RECREATED[name]
    logp = peaked_posteriors(seed, 1, 100, V, peak=peak)
    run_case(logp, [100], 3, 3, 3, None if lm == "none" else lm, tol, "recreated / %s" % name, min_recreated=1)


# ---- 4. the n-gram point query ---------------------------------------------------------------------------------------------------
def _pairs_check(lm, n, seed):
    from espnet_amd import ops
    g = torch.Generator().manual_seed(seed)
    V, Cw, nw = lm.n_vocab, lm.order - 1, len(lm.words)
    ctx0 = (torch.randint(0, nw + 1, (n, Cw), generator=g) - 1).to(torch.int32).to(DEV)            # -1 = empty among them
    tok_prev = torch.randint(0, V, (n,), generator=g).to(DEV)
    tok = torch.randint(0, V, (n,), generator=g).to(DEV)
    rows, ctx = ops.ngram_score(lm, ctx0, tok_prev)
    lp, ctx_new = ops.ngram_score_pairs(lm, ctx.contiguous(), tok)
    _, ctx_want = ops.ngram_score(lm, ctx, tok)
    torch.cuda.synchronize()
    want = rows.gather(1, tok.view(-1, 1)).view(-1)
    assert lp.dtype == torch.float32 and ctx_new.dtype == torch.int32
    assert torch.equal(lp.view(torch.int32), want.view(torch.int32)), "the point query is not bit-equal to the row's element"
    assert torch.equal(ctx_new, ctx_want)
    return int((ctx[:, 0] >= 0).sum())


@pytest.mark.parametrize("which", ["test", "beam"])
def test_ngram_score_pairs_equals_the_row_elements(which):
    from espnet_amd.nets.ngram import ArpaLM
    path = ARPA[which]
    lm = ArpaLM(path, lm_tokens(path, 14)).to(DEV)
    assert _pairs_check(lm, 3000, 1) > 0


def test_ngram_score_pairs_on_a_four_gram(tmp_path):
    """deeper walks and longer successor lists than the fixtures have: a seeded random 4-gram over 40 words, 60 tokens"""
    from espnet_amd.nets.ngram import ArpaLM
    path = str(tmp_path / "r4.arpa")
    toks = write_random_arpa(path, 4, 40, 400, seed=5, n_tokens=60)
    lm = ArpaLM(path, toks).to(DEV)
    assert lm.order == 4
    _pairs_check(lm, 5000, 2)


# ---- 5. model level ----------------------------------------------------------------------------------------------------------------
def _ctc_conformer():
    from espnet_amd.nets.e2e_asr_conformer import E2E
    torch.manual_seed(0)
    ns = argparse.Namespace(adim=64, aheads=4, elayers=2, eunits=128, dlayers=1, dunits=128, mtlalpha=1.0, dropout_rate=0.0,
                            transformer_encoder_pos_enc_layer_type="rel_pos", transformer_encoder_selfattn_layer_type="rel_selfattn",
                            macaron_style=True, use_cnn_module=True, cnn_module_kernel=15)
    return E2E(40, 30, ns).to(DEV).eval()


def _same_nbest(a, b, rel=0.0):
    """-> the largest |difference of scores| / max(1, |score|)"""
    assert len(a) == len(b) > 0 and [h["yseq"] for h in a] == [h["yseq"] for h in b]
    diff = max(abs(x["score"] - y["score"]) / max(1.0, abs(y["score"])) for x, y in zip(a, b))
    assert diff <= rel, (diff, rel)
    return diff


# recognize_batch against recognize: the same frames go through the output layer as one product of more rows, which may round
# differently.  Measured largest relative score difference 6.1e-8 (one fp32 rounding); no margin is asserted for these model
# posteriors, so equal sequences rest on the differences staying at that size
BATCH_REL = 2.4e-7


def test_recognize_runs_the_prefix_beam_search():
    """recognize(ctc_weight=1, beam_size=4, nbest=2) = CTCPrefixBeamSearch on the model's own log-softmax (scores with ==);
    recognize_batch of three utterances of different lengths = recognize of each alone (the output layer of the padded batch
    runs as one product of more rows, which may round differently: scores to BATCH_REL); an n-gram scorer is passed on;
    beam_size == 1 stays the greedy path.  On the parent commit the first call raises NotImplementedError."""
    from espnet_amd.nets.ctc_prefix_beam import CTCPrefixBeamSearch
    from espnet_amd.nets.ngram import NgramFullScorer
    model = _ctc_conformer()
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(n, 40, generator=g) for n in (83, 60, 47)]
    ra = argparse.Namespace(ctc_weight=1.0, beam_size=4, nbest=2, penalty=0.0)
    got = model.recognize(xs[0], ra)
    with torch.no_grad():
        logp = model.ctc.log_softmax(model.encode(xs[0]).unsqueeze(0))[0]
    _same_nbest(got, CTCPrefixBeamSearch(4, nbest=2)(logp))
    assert len(got) == 2 and got[0]["yseq"][0] == model.sos and got[0]["yseq"][-1] == model.eos and got[0]["score"] >= got[1]["score"]
    batch = model.recognize_batch(xs, ra)
    assert len(batch) == 3
    worst = max(_same_nbest(hyps, model.recognize(x, ra), rel=BATCH_REL) for x, hyps in zip(xs, batch))
    print("[ctc prefix beam] recognize_batch against recognize: largest relative score difference %.3e" % worst)
    # the n-gram scorer and the options reach the search
    toks = lm_tokens(ARPA_BEAM, 30)
    scorer = NgramFullScorer(ARPA_BEAM, toks)
    ra2 = argparse.Namespace(ctc_weight=1.0, beam_size=4, nbest=2, penalty=0.5, ngram_weight=0.3, ctc_cand_size=6)
    fused = model.recognize(xs[0], ra2, ngram=scorer)
    _same_nbest(fused, CTCPrefixBeamSearch(4, 6, 2, 0.5, ngram=scorer.lm, ngram_weight=0.3)(logp))
    assert [h["score"] for h in fused] != [h["score"] for h in got]
    greedy = model.recognize(xs[0], argparse.Namespace(ctc_weight=1.0, beam_size=1))
    assert len(greedy) == 1 and greedy[0]["score"] == 0.0 and greedy[0]["yseq"][0] == model.sos


def test_speech2text_time_search():
    """Speech2Text(ctc_search="time") returns (text, token, token_int, hyp) of the search the espnet1 side runs on the same
    encoder output"""
    from espnet_amd.espnet2 import CTC, ConformerEncoder, ESPnetASRModel, Speech2Text, TransformerDecoder
    from espnet_amd.espnet2.asr_inference import CharTokenizer
    from espnet_amd.nets.beam_search import Hypothesis
    torch.manual_seed(2)
    enc = ConformerEncoder(20, output_size=64, attention_heads=4, linear_units=96, num_blocks=2, dropout_rate=0.0,
                           positional_dropout_rate=0.0, attention_dropout_rate=0.0, macaron_style=True, cnn_module_kernel=7)
    dec = TransformerDecoder(30, 64, attention_heads=4, linear_units=96, num_blocks=1, dropout_rate=0.0, positional_dropout_rate=0.0)
    model = ESPnetASRModel(vocab_size=30, encoder=enc, decoder=dec, ctc=CTC(30, 64, ctc_type="builtin"), ctc_weight=1.0)
    token_list = ["<blank>"] + [str(i) for i in range(1, 28)] + ["<space>", "<sos/eos>"]
    s2t = Speech2Text(model, token_list=token_list, tokenizer=CharTokenizer(), device=DEV, beam_size=5, ctc_weight=1.0, penalty=0.2,
                      nbest=3, ctc_search="time")
    speech = torch.randn(90, 20, generator=torch.Generator().manual_seed(3))
    res = s2t(speech.numpy())
    with torch.no_grad():
        enc_out, _ = model.encode(speech.unsqueeze(0).to(DEV), torch.full([1], 90, dtype=torch.long))
    want = model.ctc.prefix_beam_search(enc_out, [enc_out.shape[1]], beam_size=5, nbest=3, penalty=0.2)[0]
    assert len(res) == len(want) == 3
    for (text, token, token_int, hyp), w in zip(res, want):
        assert isinstance(hyp, Hypothesis) and hyp.yseq.tolist() == w["yseq"] and float(hyp.score) == w["score"]
        assert token_int == [t for t in w["yseq"][1:-1] if t != 0] and token == [token_list[t] for t in token_int]
        assert text == "".join(" " if t == "<space>" else t for t in token)
    # with an n-gram LM and a candidate count: the same options reach the same search
    from espnet_amd.nets.ngram import ArpaLM
    lm = ArpaLM(ARPA_BEAM, lm_tokens(ARPA_BEAM, 30))
    fused = Speech2Text(model, token_list=token_list, tokenizer=CharTokenizer(), device=DEV, beam_size=5, ctc_weight=1.0, penalty=0.2,
                        nbest=3, ctc_search="time", ngram=lm, ngram_weight=0.3, ctc_cand_size=6)(speech.numpy())
    want_lm = model.ctc.prefix_beam_search(enc_out, [enc_out.shape[1]], beam_size=5, cand_size=6, nbest=3, penalty=0.2, ngram=lm,
                                           ngram_weight=0.3)[0]
    assert [r[3].yseq.tolist() for r in fused] == [w["yseq"] for w in want_lm]
    assert [float(r[3].score) for r in fused] == [w["score"] for w in want_lm]
    assert [float(r[3].score) for r in fused] != [w["score"] for w in want]
