"""CER / WER scoring, CPU side: a pure-Python restatement of the reference's ErrorCalculator (e2e_asr_common.py:132-246: string
joins, str.replace, str.split, the textbook edit distance) pinned to what the reference recorded in tests/golden/error_calc.npz
(tools/gen_error_calc_golden.py); the code-point tables the device path is built on; and the host checks of the two new C-ABI
entry points.  No GPU is used here; tests/test_gpu_error_calc.py runs the kernels and the models against this restatement."""
import ctypes
import os
from itertools import groupby

import numpy as np
import pytest

from conftest import ROOT, load_golden

LIB = os.path.join(ROOT, "espnet_amd", "csrc", "libespnet_amd_hip.so")
LISTS = ("char", "bpe")


def levenshtein(a, b):
    a, b = list(a), list(b)
    d = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(b) + 1):
            cur = min(d[j] + 1, d[j - 1] + 1, prev + (a[i - 1] != b[j - 1]))
            prev, d[j] = d[j], cur
    return d[-1]


def convert_to_char(tokens, space, blank, ys_hat, ys_pad):
    """e2e_asr_common.py:189-212 -> (hypothesis texts, reference texts)"""
    hats, trues = [], []
    for y_hat, y_true in zip(ys_hat, ys_pad):
        y_hat, y_true = [int(v) for v in y_hat], [int(v) for v in y_true]
        ymax = y_true.index(-1) if -1 in y_true else len(y_true)
        hat = "".join(tokens[i] for i in y_hat[:ymax]).replace(space, " ").replace(blank, "")
        true = "".join(tokens[i] for i in y_true if i != -1).replace(space, " ")
        hats.append(hat)
        trues.append(true)
    return hats, trues


def char_counts(hats, trues):
    """e2e_asr_common.py:214-229 -> per-utterance (distances, reference lengths)"""
    pairs = [(h.replace(" ", ""), t.replace(" ", "")) for h, t in zip(hats, trues)]
    return [levenshtein(h, t) for h, t in pairs], [len(t) for _, t in pairs]


def word_counts(hats, trues):
    """e2e_asr_common.py:231-246"""
    pairs = [(h.split(), t.split()) for h, t in zip(hats, trues)]
    return [levenshtein(h, t) for h, t in pairs], [len(t) for _, t in pairs]


def ctc_counts(tokens, space, blank, ys_hat, ys_pad):
    """e2e_asr_common.py:157-187 -> per-utterance (distances, reference lengths); 0 errors where the reference is empty"""
    idx_blank = tokens.index(blank)
    idx_space = tokens.index(space) if space in tokens else None
    eds, lens = [], []
    for y, y_true in zip(ys_hat, ys_pad):
        y_hat = [k for k, _ in groupby(int(v) for v in y)]
        hyp = "".join(tokens[i] for i in y_hat if i != -1 and i != idx_blank and i != idx_space)
        ref = "".join(tokens[int(i)] for i in y_true if int(i) != -1 and int(i) != idx_blank and int(i) != idx_space)
        eds.append(levenshtein(hyp, ref) if len(ref) > 0 else 0)
        lens.append(len(ref))
    return eds, lens


def rate(eds, lens):
    return float(sum(eds)) / sum(lens)


def golden_case(g, name):
    tokens = [str(t) for t in g[name + "_tokens"]]
    return tokens, str(g["sym_space"]), str(g["sym_blank"])


@pytest.fixture(scope="module")
def golden():
    return load_golden("error_calc.npz")


@pytest.mark.parametrize("name", LISTS)
def test_restatement_equals_the_reference(golden, name):
    g = golden
    tokens, space, blank = golden_case(g, name)
    assert (space in tokens) == (name == "char")
    hats, trues = convert_to_char(tokens, space, blank, g[name + "_att_hat"], g[name + "_ys_pad"])
    ce, cl = char_counts(hats, trues)
    we, wl = word_counts(hats, trues)
    te, tl = ctc_counts(tokens, space, blank, g[name + "_ctc_hat"], g[name + "_ys_pad"])
    assert ce == g[name + "_char_ed"].tolist() and cl == g[name + "_char_len"].tolist()
    assert we == g[name + "_word_ed"].tolist() and wl == g[name + "_word_len"].tolist()
    assert te == g[name + "_ctc_ed"].tolist() and tl == g[name + "_ctc_len"].tolist()
    assert rate(ce, cl) == float(g[name + "_cer"]) and rate(we, wl) == float(g[name + "_wer"])
    assert rate(te, tl) == float(g[name + "_cer_ctc"])


def test_fixture_covers_the_cases(golden):
    g = golden
    for name in LISTS:
        ys_pad = g[name + "_ys_pad"]
        assert (ys_pad[3] == -1).all() and g[name + "_char_len"][3] == 0 and (np.delete(g[name + "_char_len"], 3) > 0).all()
        assert g[name + "_att_hat"].shape[1] > ys_pad.shape[1]           # hypotheses longer than every ymax
        assert (g[name + "_att_hat"] == 0).any() and (g[name + "_ctc_hat"] == 0).any()          # blanks
        assert (g[name + "_ctc_hat"][:, 1:] == g[name + "_ctc_hat"][:, :-1]).any()               # repeats
    sp = [str(t) for t in g["char_tokens"]].index("<space>")
    y = g["char_ys_pad"]
    assert y[1, 0] == sp and y[2, 3] == sp and y[2, 2] == sp and y[2, 8] == sp          # leading, double, trailing
    assert sum(any(ord(c) > 127 for c in str(t)) for t in g["bpe_tokens"]) >= 2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "error_calc.npz")) < 16 * 1024


def test_tables():
    from espnet_amd.nets.e2e_asr_common import ErrorCalculator
    tokens = ["<blank>", "<unk>", "<space>", "a", "é", "日本", "<eos>"]
    ec = ErrorCalculator(tokens, "<space>", "<blank>", True, True)
    assert ec.idx_blank == 0 and ec.idx_space == 2

    def rows(table):
        off, cp, longest = table
        assert len(off) == len(tokens) + 1 and off[-1] == len(cp) and longest == max(b - a for a, b in zip(off, off[1:]))
        return [cp[a:b] for a, b in zip(off, off[1:])]
    hyp, ref, ctc = rows(ec.tables["hyp"]), rows(ec.tables["ref"]), rows(ec.tables["ctc"])
    assert hyp[0] == [] and hyp[2] == [0x20] and hyp[4] == [0xE9] and hyp[5] == [0x65E5, 0x672C]
    assert hyp[1] == [ord(c) for c in "<unk>"]
    assert ref[0] == [ord(c) for c in "<blank>"] and ref[2] == [0x20] and ref[1:] == hyp[1:]       # blank is not stripped
    assert ctc[0] == [] and ctc[2] == [] and ctc[3:] == hyp[3:] and ctc[1] == hyp[1]
    # no <space> in the list: idx_space is None and nothing maps to 0x20
    bpe = ErrorCalculator(["<blank>", "▁a", "b", "<eos>"], "<space>", "<blank>", True, False)
    assert bpe.idx_space is None
    assert all(0x20 not in r for t in bpe.tables.values() for r in rows_of(t))
    assert rows_of(bpe.tables["ctc"])[1] == [0x2581, ord("a")]


def rows_of(table):
    off, cp, _ = table
    return [cp[a:b] for a, b in zip(off, off[1:])]


@pytest.mark.parametrize("tokens", [
    ["<blank>", "a b", "<space>"],                   # whitespace inside a token
    ["<blank>", "a\t", "<space>"],
    ["<blank>", "x<space>", "<space>"],              # the symbol inside another token
    ["<blank>", "<blank>s", "<space>"],
    ["<blank>", "<", "space>", "<space>"],           # "<" + "space>" joins to the symbol
    ["<blank>", "a<bl", "ank>", "<space>"],
])
def test_unfaithful_token_lists_are_refused(tokens):
    from espnet_amd.nets.e2e_asr_common import ErrorCalculator
    with pytest.raises(ValueError):
        ErrorCalculator(tokens, "<space>", "<blank>", True, True)


def test_usual_token_lists_are_accepted(golden):
    from espnet_amd.nets.e2e_asr_common import ErrorCalculator
    for name in LISTS:
        tokens, space, blank = golden_case(golden, name)
        ErrorCalculator(tokens, space, blank, True, True)
    with pytest.raises(ValueError):                  # as in the reference: char_list.index(sym_blank)
        ErrorCalculator(["a", "b"], "<space>", "<blank>")


def test_calculator_without_flags_returns_none_and_needs_a_gpu_otherwise(golden):
    import torch
    from espnet_amd import _lib
    from espnet_amd.nets.e2e_asr_common import ErrorCalculator
    tokens, space, blank = golden_case(golden, "char")
    hat, pad = torch.from_numpy(golden["char_att_hat"]), torch.from_numpy(golden["char_ys_pad"])
    assert ErrorCalculator(tokens, space, blank)(hat, pad) == (None, None)
    with pytest.raises(_lib.EamdError):              # no CPU fallback
        ErrorCalculator(tokens, space, blank, True, True)(hat, pad)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("libespnet_amd_hip.so is not built")
    lib = ctypes.CDLL(LIB)
    lib.eamd_edit_distance_workspace_bytes.restype = ctypes.c_int64
    return lib


def test_symbols_bound(lib):
    from espnet_amd import _lib
    for s in ("eamd_text_units", "eamd_edit_distance", "eamd_edit_distance_workspace_bytes"):
        assert hasattr(lib, s) and s in _lib.SYMBOLS


def test_host_checks_without_a_gpu(lib):
    # two DP rows of max(lda, ldb) + 1 int32 per pair; no cap at 8192 symbols
    assert lib.eamd_edit_distance_workspace_bytes(3, 10, 7) == 3 * 2 * 11 * 4
    assert lib.eamd_edit_distance_workspace_bytes(1, 8192, 20000) == 2 * 20001 * 4
    i64 = ctypes.c_int64
    assert lib.eamd_edit_distance(None, 4, None, None, 4, None, None, None, i64(1 << 20), 2, None) == -1     # NULL operands
    buf = ctypes.create_string_buffer(64)            # a host buffer stands in for every pointer: refused before any launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.eamd_edit_distance(p, 4, p, p, 4, p, p, p, i64(8), 2, None) == -1                              # workspace too small
    assert lib.eamd_edit_distance(p, 0, p, p, 4, p, p, p, i64(1 << 20), 2, None) == -1
    assert lib.eamd_text_units(*([None] * 7), 2, 5, 10, 20, 0, -1, 0, None) == -1                              # NULL operands
    assert lib.eamd_text_units(p, None, p, p, p, p, p, 2, 5, 10, 20, 0, -1, 7, None) == -1                     # unknown mode
    assert lib.eamd_text_units(p, None, p, p, p, p, p, 2, 5, 10, 0, 0, -1, 0, None) == -1                      # cap == 0
