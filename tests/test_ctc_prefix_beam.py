"""CTC prefix beam search, host side: the float64 dictionary restatement (tests/ctc_prefix_beam_restatement.py) against the
exact CTC forward recursion, the argument refusals of every layer, and the C ABI of the new entry points.  No kernel is
launched here (tests/test_gpu_ctc_prefix_beam.py does that)."""
import argparse
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from ctc_prefix_beam_restatement import ArpaDefinition, candidates, ctc_log_prob, peaked_posteriors, prefix_beam_search
from test_ngram import ARPA_BEAM, ARPA_TEST, fixture_tokens


# ---- the restatement against the exact CTC sequence probability ---------------------------------------------------------
@pytest.mark.parametrize("T,n_strings,n_feasible", [(4, 31, 15), (5, 63, 25)])
def test_restatement_gives_the_exact_sequence_probability(T, n_strings, n_feasible):
    """V = 4 (two real tokens), K = 2, W = 64: nothing is pruned.  Of the 31 / 63 label strings of up to T tokens, those that fit
    into T frames (a repeated token needs a blank between: len + repeats <= T; 15 / 25 of them) are in the beam with their
    exact log p(y | x), the others have log p = -inf in the forward recursion and are absent (an entry at -inf is never kept).
    The posterior gives <eos>, which is never appended, no mass, so the beam's mass is 1"""
    logits = torch.randn(T, 4, generator=torch.Generator().manual_seed(T), dtype=torch.float64)
    logits[:, 3] = -math.inf
    logp = torch.log_softmax(logits, dim=-1).numpy()
    nbest, _, _ = prefix_beam_search(logp, W=64, K=2, nbest=64)
    strings = [s for n in range(T + 1) for s in itertools.product((1, 2), repeat=n)]
    got = {h[1]: h[2] for h in nbest}
    assert len(strings) == n_strings and len(got) == len(nbest) == n_feasible and set(got) <= set(strings)
    worst = 0.0
    for s in strings:
        want = ctc_log_prob(logp, s)
        if s in got:
            worst = max(worst, abs(got[s] - want))
        else:
            assert want == -math.inf, s
    mass = sum(math.exp(v) for v in got.values())
    print("[ctc prefix beam] T = %d: %d strings, %d feasible, worst |restatement - forward| %.2e, mass - 1 = %.2e"
          % (T, len(strings), len(got), worst, mass - 1))
    assert worst <= 1e-12 and abs(mass - 1.0) <= 1e-12
    assert all(a[0] >= b[0] for a, b in zip(nbest, nbest[1:]))


def test_restatement_candidates_and_lm_terms():
    """ties go to the lower id and neither blank nor eos is a candidate; with an LM the rank score carries
    ngram_weight * sum of log10 p and the final score the </s> term"""
    assert candidates(np.asarray([9.0, 1.0, 3.0, 3.0, 0.5, 9.0]), 3) == [2, 3, 1]
    toks = fixture_tokens(ARPA_BEAM)
    V = len(toks)
    lm = ArpaDefinition(ARPA_BEAM, toks)
    logp = peaked_posteriors(0, 1, 12, V)[0].numpy()
    plain, _, _ = prefix_beam_search(logp, W=64, K=V - 2, nbest=64)
    fused, _, _ = prefix_beam_search(logp, W=64, K=V - 2, nbest=64, penalty=0.5, lm=lm, ngram_weight=0.3)
    by_prefix = {h[1]: h for h in plain}
    for s, l, tot in fused:
        if l in by_prefix:                       # pruned differently, but a shared prefix has the same acoustic mass
            want = sum(lm(l[:i], l[i]) for i in range(len(l))) + lm(l, V - 1)
            assert abs(s - (tot + 0.3 * want + 0.5 * len(l))) <= 1e-12


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_search_refuses_what_it_cannot_do():
    from espnet_amd.nets.ctc_prefix_beam import MAX_BEAM, MAX_CAND, MAX_FRAMES, CTCPrefixBeamSearch
    assert (MAX_BEAM, MAX_CAND, MAX_FRAMES) == (32, 32, 2048)
    with pytest.raises(ValueError, match="blank"):
        CTCPrefixBeamSearch(4, blank=1)
    with pytest.raises(ValueError, match="beam_size"):
        CTCPrefixBeamSearch(MAX_BEAM + 1)
    with pytest.raises(ValueError, match="cand_size"):
        CTCPrefixBeamSearch(4, cand_size=MAX_CAND + 1)
    with pytest.raises(ValueError, match="nbest"):
        CTCPrefixBeamSearch(4, nbest=5)
    with pytest.raises(TypeError, match="ngram"):
        CTCPrefixBeamSearch(4, ngram=object())
    s = CTCPrefixBeamSearch(4, cand_size=11, eos=11)
    with pytest.raises(ValueError, match="eos"):
        s.search_device(torch.zeros(1, 3, 20), [3])                 # eos is not the last id
    with pytest.raises(ValueError, match="cand_size"):
        CTCPrefixBeamSearch(4, cand_size=11).search_device(torch.zeros(1, 3, 12), [3])
    with pytest.raises(ValueError, match="frames"):
        CTCPrefixBeamSearch(4).search_device(torch.zeros(1, MAX_FRAMES + 1, 12), [3])
    for hl in ([0], [4], [3, 3]):
        with pytest.raises(ValueError, match="hlens"):
            CTCPrefixBeamSearch(4).search_device(torch.zeros(1, 3, 12), hl)
    from espnet_amd.nets.ngram import ArpaLM
    lm = ArpaLM(ARPA_TEST, fixture_tokens(ARPA_TEST))
    with pytest.raises(ValueError, match="n-gram"):
        CTCPrefixBeamSearch(4, ngram=lm, ngram_weight=0.3).search_device(torch.zeros(1, 3, lm.n_vocab + 1), [3])


def test_query_tables_are_the_successors_sorted_by_token():
    from espnet_amd.nets.ngram import ArpaLM
    for path in (ARPA_TEST, ARPA_BEAM):
        lm = ArpaLM(path, fixture_tokens(path))
        st, tok, lp = lm.succ_start.numpy(), lm.succ_tok.numpy(), lm.succ_lp.numpy()
        qt, ql = lm.qsucc_tok.numpy(), lm.qsucc_lp.numpy()
        for m in range(lm.node_bo.numel()):
            s, e = st[m], st[m + 1]
            assert list(qt[s:e]) == sorted(qt[s:e]) and len(set(qt[s:e])) == e - s
            assert sorted(zip(tok[s:e], lp[s:e])) == list(zip(qt[s:e], ql[s:e]))
        assert lm.to("cpu").qsucc_tok.dtype == torch.int32


def test_speech2text_time_search_needs_a_pure_ctc_weight():
    from espnet_amd.espnet2 import Speech2Text
    with pytest.raises(ValueError, match="ctc_weight"):
        Speech2Text(None, ctc_search="time", ctc_weight=0.5)
    with pytest.raises(ValueError, match="ctc_search"):
        Speech2Text(None, ctc_search="frames", ctc_weight=1.0)
    with pytest.raises(ValueError, match="beam_size"):
        Speech2Text(None, ctc_search="time", ctc_weight=1.0, beam_size=33)
    # options of the time-synchronous search are not dropped silently by the label-synchronous one
    with pytest.raises(ValueError, match="ngram"):
        Speech2Text(None, ctc_weight=1.0, ngram=object(), ngram_weight=0.3)
    with pytest.raises(ValueError, match="ctc_cand_size"):
        Speech2Text(None, ctc_weight=0.3, ctc_cand_size=8)


def test_pure_ctc_recognize_refuses_a_neural_lm():
    """before any encoder work: no GPU needed"""
    from espnet_amd.nets.e2e_asr_conformer import E2E
    ns = argparse.Namespace(adim=16, aheads=2, elayers=1, eunits=16, dlayers=1, dunits=16, mtlalpha=1.0, dropout_rate=0.0)
    model = E2E(8, 6, ns)
    ra = argparse.Namespace(ctc_weight=1.0, beam_size=3, nbest=1, penalty=0.0)
    with pytest.raises(ValueError, match="rnnlm"):
        model.recognize(torch.zeros(20, 8), ra, rnnlm=torch.nn.Linear(1, 1))
    with pytest.raises(ValueError, match="rnnlm"):
        model.recognize_batch([torch.zeros(20, 8)], ra, rnnlm=torch.nn.Linear(1, 1))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_refuse_bad_arguments_without_a_gpu():
    from espnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "espnet_amd.h")).read()
    for s in ("eamd_ctc_prefix_beam", "eamd_ctc_beam_workspace_bytes", "eamd_ngram_score_pairs"):
        assert s in _lib.SYMBOLS and s + "(" in hdr
    lib = _lib.lib()
    i64, f = ctypes.c_int64, ctypes.c_float
    assert lib.eamd_ctc_beam_workspace_bytes(2, 10, 4) == 2 * (10 * 4 + 1) * 8 and lib.eamd_ctc_beam_workspace_bytes(0, 10, 4) == 0
    none9 = [None] * 9

    def beam(logp, cv, ci, hl, B, T, V, W, K, nbest, tables, N, ws, ws_bytes, out):
        return lib.eamd_ctc_prefix_beam(logp, i64(V), cv, ci, hl, B, T, V, W, K, nbest, f(0.0), *tables, 1, N, 0, 0, f(0.0), ws,
                                        i64(ws_bytes), out, None)

    assert beam(None, None, None, None, 1, 4, 6, 2, 2, 1, none9, 0, None, 0, None) == -1
    # valid-looking (never dereferenced) host addresses: the limits are refused before any launch
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30
    assert beam(p, p, p, p, 1, 4, 6, 33, 2, 1, none9, 0, p, big, p) == _lib.EAMD_EUNSUPPORTED          # beam > 32
    assert beam(p, p, p, p, 1, 4, 40, 2, 33, 1, none9, 0, p, big, p) == _lib.EAMD_EUNSUPPORTED         # candidates > 32
    assert beam(p, p, p, p, 1, 2049, 6, 2, 2, 1, none9, 0, p, big, p) == _lib.EAMD_EUNSUPPORTED        # frames > 2048
    assert beam(p, p, p, p, 1, 4, 6, 2, 2, 1, [p] * 9, 9, p, big, p) == _lib.EAMD_EUNSUPPORTED         # LM order > 8
    assert beam(p, p, p, p, 1, 4, 6, 2, 5, 1, none9, 0, p, big, p) == -1                                # K > V - 2
    assert beam(p, p, p, p, 1, 4, 6, 2, 2, 3, none9, 0, p, big, p) == -1                                # nbest > beam
    assert beam(p, p, p, p, 1, 4, 6, 2, 2, 1, none9, 0, p, 8, p) == -1                                  # workspace too small
    assert beam(p, p, p, p, 1, 4, 6, 2, 2, 1, [p] + [None] * 8, 3, p, big, p) == -1                     # an LM without its tables

    def pairs(tables, N, ctx, tok, lp, ctx_new, n):
        return lib.eamd_ngram_score_pairs(*tables, 1, 8, N, 0, ctx, tok, lp, ctx_new, n, None)

    assert pairs(none9, 3, None, None, None, None, 1) == -1
    assert pairs([p] * 9, 3, p, p, p, p, 0) == -1
    assert pairs([p] * 9, 9, p, p, p, p, 1) == _lib.EAMD_EUNSUPPORTED
    assert pairs([p] * 9, 3, None, p, p, p, 1) == -1                                                    # N > 1 needs contexts
