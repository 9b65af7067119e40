"""n-gram LM shallow fusion, host side (espnet_amd/nets/ngram.py): the ARPA parser and the flat tables against the
back-off definition written out in float64, literal values of the two reference fixtures, and the C ABI of eamd_ngram_score.
No kernel is launched here (tests/test_gpu_ngram.py does that); the helpers below are shared with it."""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

ARPA_TEST = os.path.join(GOLDEN, "ngram_test.arpa")
ARPA_BEAM = os.path.join(GOLDEN, "ngram_beam_search_test.arpa")


def f32(v):
    return float(np.float32(float(v)))


def arpa_dict(path):
    """{n-gram tuple of word strings: (log10 prob, back-off)}, every number rounded to fp32 -> (dict, order)"""
    grams, k = {}, 0
    for line in open(path, encoding="utf-8"):
        line = line.strip()
        if line.endswith("-grams:"):
            k = int(line[1:].split("-")[0])
        elif line and not line.startswith("\\") and k > 0:
            c = line.split()
            grams[tuple(c[1:k + 1])] = (f32(c[0]), f32(c[k + 1]) if len(c) > k + 1 else 0.0)
    grams.setdefault(("<unk>",), (-100.0, 0.0))
    return grams, max(len(g) for g in grams)


def definition(grams, order, hist, w):
    """log10 p(w | hist) of the back-off model in float64: the longest listed n-gram (suffix of hist + w) plus the back-offs of
    the longer contexts that exist.  hist: word strings, oldest first -> (value, sum of |terms|)"""
    known = lambda x: x if (x,) in grams else "<unk>"      # noqa: E731
    hist = tuple(known(x) for x in hist)[-(order - 1):] if order > 1 else ()
    w = known(w)
    for j in range(len(hist), -1, -1):
        g = hist[len(hist) - j:] + (w,)
        if g in grams:
            terms = [grams[g][0]] + [grams[hist[len(hist) - i:]][1] for i in range(j + 1, len(hist) + 1)
                                     if hist[len(hist) - i:] in grams]
            return sum(terms), sum(abs(t) for t in terms)
    raise AssertionError("no unigram for %r" % (w,))


def table_walk(lm, ctx):
    """the passes of eamd_ngram_score over ArpaLM's tables in numpy, fp32, in the kernel's order.  ctx: word ids, most recent
    first, -1 = empty -> row float32 [V]"""
    T = {k: getattr(lm, k).cpu().numpy() for k in ("uni_tok", "node_bo", "child_start", "child_word", "child_node", "succ_start",
                                                   "succ_tok", "succ_lp")}
    nodes = [0]
    for w in ctx:
        lo, hi = T["child_start"][nodes[-1]], T["child_start"][nodes[-1] + 1]
        p = lo + int(np.searchsorted(T["child_word"][lo:hi], w))
        if w < 0 or p >= hi or T["child_word"][p] != w:
            break
        nodes.append(int(T["child_node"][p]))
    D = len(nodes) - 1
    row = None
    for j in range(D + 1):
        acc = np.float32(0.0)
        for i in range(j + 1, D + 1):
            acc = np.float32(acc + T["node_bo"][nodes[i]])
        if j == 0:
            row = (T["uni_tok"] + acc).astype(np.float32)
        else:
            s, e = T["succ_start"][nodes[j]], T["succ_start"][nodes[j] + 1]
            row[T["succ_tok"][s:e]] = T["succ_lp"][s:e] + acc
    return row


def fixture_tokens(path):
    """a token list over a fixture's words: <eos> for </s>, one token the file does not list, and <s> left out"""
    words = [g[0] for g in arpa_dict(path)[0] if len(g) == 1 and g[0] not in ("<s>", "</s>")]
    return ["<blank>"] + words + ["zzz", "<eos>"]


def write_random_arpa(path, order, n_words, n_per_order, seed, n_tokens=None):
    """a seeded random well-formed ARPA file (every n-gram's context and its suffix are listed one order lower; <s> only first,
    </s> only last) -> token list of n_tokens entries: <blank>, <unk>, the words, tokens the file does not list, <eos>"""
    rnd = random.Random(seed)
    words = ["w%d" % i for i in range(n_words)]
    levels = [[("<unk>",), ("<s>",), ("</s>",)] + [(w,) for w in words]]
    ext = {(): words + ["</s>"]}                                    # (k-1)-gram minus its last word -> its listed last words
    for k in range(2, order + 1):
        ctxs = [g for g in levels[-1] if g[-1] != "</s>" and g[0] != "<unk>"]
        new = set()
        for _ in range(4 * n_per_order):
            if len(new) >= n_per_order or not ctxs:
                break
            g = rnd.choice(ctxs)
            cand = ext.get(g[1:], [])
            if cand:
                new.add(g + (rnd.choice(cand),))
        new = sorted(new)
        ext = {}
        for g in new:
            ext.setdefault(g[:-1], []).append(g[-1])
        levels.append(new)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n" + "".join("ngram %d=%d\n" % (k + 1, len(lv)) for k, lv in enumerate(levels)) + "\n")
        for k, lv in enumerate(levels):
            f.write("\\%d-grams:\n" % (k + 1))
            for g in lv:
                lp = "%.7f" % rnd.uniform(-3.0, -0.05)
                bo = "" if k + 1 == order else "\t%.7f" % rnd.uniform(-1.0, 0.0)
                f.write("%s\t%s%s\n" % (lp, " ".join(g), bo))
            f.write("\n")
        f.write("\\end\\\n")
    n_tokens = n_tokens or n_words + 4
    assert n_tokens >= n_words + 3
    return ["<blank>", "<unk>"] + words + ["x%d" % i for i in range(n_tokens - n_words - 3)] + ["<eos>"]


def check_contexts(lm, grams, rows, ctxs):
    """rows[i] (fp32 [V], however computed) for context ctxs[i] (word ids, most recent first, -1 = empty) against the float64
    definition: |got - want| <= (N - 1) 2^-24 sum|terms|, the rounding of at most N - 1 fp32 additions.  The definition is
    evaluated once per distinct context -> worst error / bound"""
    id2word = {i: w for w, i in lm.words.items()}
    tok_words = [id2word[int(w)] for w in lm.tok2word.cpu().numpy()]
    want, worst = {}, 0.0
    for row, ctx in zip(rows, ctxs):
        k = len(ctx) if -1 not in list(ctx) else list(ctx).index(-1)
        hist = tuple(id2word[int(w)] for w in ctx[:k])[::-1]
        if hist not in want:
            vals = [definition(grams, lm.order, hist, w) for w in tok_words]
            want[hist] = (np.asarray([v[0] for v in vals]), (lm.order - 1) * 2.0 ** -24 * np.asarray([v[1] for v in vals]))
        ref, bound = want[hist]
        err = np.abs(np.asarray(row, dtype=np.float64) - ref)
        v = int(np.argmax(err - bound))
        assert err[v] <= bound[v], (tuple(ctx), v, float(row[v]), ref[v], bound[v])
        worst = max(worst, float(np.max(err / bound)))
    return worst


def all_contexts(lm, depth):
    """every context of length 0 .. depth over every word id, padded with -1 to N - 1"""
    W, C = len(lm.words), lm.order - 1
    out = [()]
    for d in range(1, depth + 1):
        out += [tuple(int(x) for x in np.unravel_index(i, (W,) * d)) for i in range(W ** d)]
    return [c + (-1,) * (C - len(c)) for c in out]


# ---- the tables against the definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [ARPA_TEST, ARPA_BEAM])
def test_tables_follow_the_backoff_definition(path):
    from espnet_amd.nets.ngram import ArpaLM
    lm = ArpaLM(path, fixture_tokens(path))
    grams, order = arpa_dict(path)
    assert lm.order == order == 3 and lm.uni_tok.dtype.is_floating_point and lm.tok2word.numel() == len(fixture_tokens(path))
    ctxs = all_contexts(lm, 2)
    assert len(ctxs) == 1 + len(lm.words) + len(lm.words) ** 2 <= 1 + 9 + 81
    worst = check_contexts(lm, grams, [table_walk(lm, c) for c in ctxs], ctxs)
    print("[ngram] %s: %d contexts, worst error / bound %.3f" % (os.path.basename(path), len(ctxs), worst))


def test_random_four_gram_tables(tmp_path):
    from espnet_amd.nets.ngram import ArpaLM
    path = str(tmp_path / "r4.arpa")
    toks = write_random_arpa(path, 4, 12, 60, seed=3, n_tokens=20)
    lm = ArpaLM(path, toks)
    grams, order = arpa_dict(path)
    assert order == lm.order == 4
    rnd = random.Random(0)
    keys = [g for g in grams if 2 <= len(g) <= 3]
    ctxs = [tuple(lm.words[w] for w in g[::-1]) + (-1,) * (3 - len(g)) for g in rnd.sample(keys, 40)]
    ctxs += [tuple(rnd.randrange(len(lm.words)) for _ in range(3)) for _ in range(40)]
    check_contexts(lm, grams, [table_walk(lm, c) for c in ctxs], ctxs)


# ---- literal values of the reference's fixtures ---------------------------------------------------------------------------
def _sentence(lm, toks, words):
    """sum of the rows' entries along <s> w1 w2 ... (the scorer's history: <s>, then the prefix)"""
    ctx, total = [lm.bos] + [-1] * (lm.order - 2), 0.0
    for w in words:
        t = toks.index(w)
        total += float(table_walk(lm, ctx)[t])
        ctx = [int(lm.tok2word[t])] + ctx[:-1]
    return total


def test_reference_sentence_scores():
    """the sums the reference's test/test_ngram.py pins with kenlm.LanguageModel.score at -1.04 / -1.18 (rel 0.01)"""
    from espnet_amd.nets.ngram import NgramFullScorer
    toks = fixture_tokens(ARPA_TEST)
    lm = NgramFullScorer(ARPA_TEST, toks).lm
    assert abs(_sentence(lm, toks, ["I", "like", "apple", "<eos>"]) - -1.04778921) <= 1e-6
    assert abs(_sentence(lm, toks, ["you", "love", "coffee", "<eos>"]) - -1.18522948) <= 1e-6


def test_reference_beam_search_fixture_values():
    from espnet_amd.nets.ngram import ArpaLM
    toks = fixture_tokens(ARPA_BEAM)
    lm = ArpaLM(ARPA_BEAM, toks)
    row = table_walk(lm, [lm.words["a"], lm.bos])                       # history <s> a
    for tok, want in (("e", -0.17803444), ("i", -1.41239593), ("<eos>", -0.7859766), ("zzz", -1.748188)):
        assert abs(float(row[toks.index(tok)]) - want) <= 1e-6, (tok, float(row[toks.index(tok)]), want)
    row = table_walk(lm, [lm.unk, lm.words["a"]])                       # history a <unknown token>
    assert abs(float(row[toks.index("e")]) - -0.81033593) <= 1e-6


# ---- parser and tables ------------------------------------------------------------------------------------------------------
def _write(tmp_path, text, name="m.arpa"):
    p = tmp_path / name
    p.write_text(text, encoding="utf-8")
    return str(p)


SMALL = ("\\data\\\nngram 1=4\nngram 2=2\nngram 3=1\n\n\\1-grams:\n-1.0\t<s>\t-0.5\n-1.5\t</s>\n-0.7\ta\t-0.25   \n-0.9\tb\n\n"
         "\\2-grams:\n-0.3\ta </s>\t-0.125\n-0.4\t<s> a\n\n\n\\3-grams:\n-0.2\tb a </s>\n\n\\end\\\n")


def test_eos_reads_end_of_sentence_and_unlisted_tokens_are_unk():
    from espnet_amd.nets.ngram import ArpaLM
    toks = fixture_tokens(ARPA_TEST)
    lm = ArpaLM(ARPA_TEST, toks)
    assert int(lm.tok2word[toks.index("<eos>")]) == lm.words["</s>"]
    assert int(lm.tok2word[toks.index("zzz")]) == lm.unk == lm.words["<unk>"] and int(lm.tok2word[0]) == lm.unk
    assert lm.bos == lm.words["<s>"]
    assert float(lm.uni_tok[toks.index("I")]) == f32(-0.8305393) and float(lm.uni_tok[0]) == f32(-1.0598761)


def test_backoff_column_is_optional_and_missing_unk_is_minus_100(tmp_path):
    from espnet_amd.nets.ngram import ArpaLM
    toks = ["<blank>", "a", "b", "q", "<eos>"]
    lm = ArpaLM(_write(tmp_path, SMALL), toks)
    assert lm.order == 3 and "<unk>" in lm.words and lm.unk == 4
    assert float(lm.uni_tok[toks.index("q")]) == -100.0 and float(lm.uni_tok[0]) == -100.0
    row = table_walk(lm, [lm.words["b"], -1])           # b has no back-off column: 0
    assert float(row[toks.index("a")]) == f32(-0.7)
    row = table_walk(lm, [lm.words["a"], -1])           # a: back-off -0.25, bigram a </s>
    assert float(row[toks.index("b")]) == f32(f32(-0.9) + f32(-0.25)) and float(row[toks.index("<eos>")]) == f32(-0.3)


def test_context_inside_a_trigram_gets_a_zero_backoff_node(tmp_path):
    from espnet_amd.nets.ngram import ArpaLM
    toks = ["<blank>", "a", "b", "<eos>"]
    lm = ArpaLM(_write(tmp_path, SMALL), toks)
    # the trigram "b a </s>" has the context (a, b) most recent first; the bigram "b a" is not listed
    cs, cw, cn = lm.child_start.numpy(), lm.child_word.numpy(), lm.child_node.numpy()
    node = 0
    for w in (lm.words["a"], lm.words["b"]):
        lo, hi = cs[node], cs[node + 1]
        assert list(cw[lo:hi]) == sorted(cw[lo:hi])
        p = lo + list(cw[lo:hi]).index(w)
        node = int(cn[p])
    assert float(lm.node_bo[node]) == 0.0
    s, e = lm.succ_start[node], lm.succ_start[node + 1]
    assert lm.succ_tok[s:e].tolist() == [toks.index("<eos>")] and float(lm.succ_lp[s]) == f32(-0.2)
    row = table_walk(lm, [lm.words["a"], lm.words["b"]])
    assert float(row[toks.index("<eos>")]) == f32(-0.2)
    assert float(row[toks.index("b")]) == f32(f32(-0.9) + f32(-0.25))       # back-off of (a) only: (b a) carries none


def test_successor_word_shared_by_two_tokens_lands_on_both(tmp_path):
    from espnet_amd.nets.ngram import ArpaLM
    toks = ["<blank>", "a", "q1", "b", "q2", "<eos>"]       # q1, q2 and <blank> all read <unk>
    text = SMALL.replace("ngram 1=4", "ngram 1=5").replace("ngram 2=2", "ngram 2=3")
    text = text.replace("-0.9\tb\n", "-0.9\tb\n-2.0\t<unk>\n").replace("-0.4\t<s> a\n", "-0.4\t<s> a\n-0.6\ta <unk>\n")
    lm = ArpaLM(_write(tmp_path, text), toks)
    row = table_walk(lm, [lm.words["a"], -1])
    for t in ("<blank>", "q1", "q2"):
        assert float(row[toks.index(t)]) == f32(-0.6)
    assert float(row[toks.index("b")]) == f32(f32(-0.9) + f32(-0.25))
    # a word no token maps to (<s>) yields no successor entry
    assert not set(lm.succ_tok.tolist()) - set(range(len(toks)))
    assert int(lm.succ_start[-1]) == 3 + 1 + 1 + 1          # a <unk> on three tokens, a </s>, <s> a, b a </s>


def test_order_nine_is_not_implemented(tmp_path):
    from espnet_amd.nets.ngram import ArpaLM
    head = "\\data\\\n" + "".join("ngram %d=1\n" % k for k in range(1, 10)) + "\n\\1-grams:\n-1\t<s>\n\n\\end\\\n"
    with pytest.raises(NotImplementedError):
        ArpaLM(_write(tmp_path, head), ["a", "<eos>"])


def test_malformed_files_raise_value_error_with_the_line(tmp_path):
    from espnet_amd.nets.ngram import ArpaLM
    toks = ["<blank>", "a", "b", "<eos>"]
    cut = SMALL[:SMALL.index("\\3-grams:")]                  # truncated: no \end\
    with pytest.raises(ValueError, match=r":\d+: "):
        ArpaLM(_write(tmp_path, cut, "cut.arpa"), toks)
    with pytest.raises(ValueError, match=r":\d+: "):       # truncated inside a section
        ArpaLM(_write(tmp_path, SMALL[:SMALL.index("-0.4\t<s> a")] + "\\end\\\n", "cut2.arpa"), toks)
    with pytest.raises(ValueError, match=r":13: "):        # a bigram line with one word
        ArpaLM(_write(tmp_path, SMALL.replace("-0.3\ta </s>\t-0.125", "-0.3\ta"), "cols.arpa"), toks)
    with pytest.raises(ValueError, match=r":9: "):
        ArpaLM(_write(tmp_path, SMALL.replace("-0.7\ta", "abc\ta"), "num.arpa"), toks)


def test_build_ngram_scorer_kinds():
    import argparse
    from espnet_amd.nets.ngram import NgramFullScorer, NgramPartScorer, build_ngram_scorer
    from espnet_amd.nets.scorer_interface import BatchScorerInterface, PartialScorerInterface
    toks = fixture_tokens(ARPA_BEAM)
    assert build_ngram_scorer(argparse.Namespace(ngram_model=None), toks) is None
    full = build_ngram_scorer(argparse.Namespace(ngram_model=ARPA_BEAM, ngram_scorer="full"), toks)
    part = build_ngram_scorer(argparse.Namespace(ngram_model=ARPA_BEAM, ngram_scorer="part"), toks)
    assert type(full) is NgramFullScorer and isinstance(full, BatchScorerInterface) and not isinstance(full, PartialScorerInterface)
    assert type(part) is NgramPartScorer and isinstance(part, PartialScorerInterface)
    for m in ("init_state", "batch_init_state", "select_state", "score", "batch_score", "score_tree", "final_score", "final_tree"):
        assert callable(getattr(full, m)), m
    assert full.final_score(None) == 0.0 and full.final_tree(None) == 0.0


# ---- C ABI --------------------------------------------------------------------------------------------------------------
def test_entry_point_is_exported_declared_and_rejects_null():
    from espnet_amd import _lib
    assert "eamd_ngram_score" in _lib.SYMBOLS
    assert "eamd_ngram_score(" in open(os.path.join(ROOT, "include", "espnet_amd.h")).read()
    lib = _lib.lib()
    i64 = ctypes.c_int64
    none9 = [None] * 9
    assert lib.eamd_ngram_score(*none9, 1, 8, 3, 0, 0, None, i64(2), None, i64(1), 0, None, None, 1, None) < 0
    # valid-looking (never dereferenced) host addresses: n < 1 and N > 8 are refused before any launch
    buf = (ctypes.c_int32 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nine = [p] * 9
    assert lib.eamd_ngram_score(*nine, 1, 8, 3, 0, 0, p, i64(2), p, i64(1), 0, p, p, 0, None) == -1
    assert lib.eamd_ngram_score(*nine, 1, 8, 9, 0, 0, p, i64(8), p, i64(1), 0, p, p, 1, None) == _lib.EAMD_EUNSUPPORTED
    assert lib.eamd_ngram_score(*nine, 1, 8, 3, 0, 0, None, i64(2), p, i64(1), 0, p, p, 1, None) == -1      # N > 1 needs contexts
