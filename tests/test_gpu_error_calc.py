"""CER / WER scoring on the GPU: eamd_edit_distance and eamd_text_units against Python (the textbook DP; "".join / replace / split),
ErrorCalculator's device path against what the reference recorded (tests/golden/error_calc.npz), and the models' reported
cer_ctc / cer / wer against the restatement of tests/test_error_calc.py fed with the model's own argmax ids / n-best."""
import argparse
from itertools import groupby

import numpy as np
import pytest
import torch

from conftest import load_golden, seeded_weights
from test_error_calc import (LISTS, char_counts, convert_to_char, ctc_counts, golden_case, levenshtein, rate, word_counts)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- eamd_edit_distance ------------------------------------------------------------------------------------------------------
def run_edit_distance(pairs, lda, ldb, fill):
    """pairs: [(a, b)] lists of ints; rows padded to lda / ldb with fill(row, width) -> symbols that would match"""
    from espnet_amd import ops
    B = len(pairs)
    a = np.empty((B, lda), np.int64)
    b = np.empty((B, ldb), np.int64)
    for i, (x, y) in enumerate(pairs):
        a[i], b[i] = fill(i, lda), fill(i, ldb)
        a[i, :len(x)] = x
        b[i, :len(y)] = y
    alen = torch.tensor([len(x) for x, _ in pairs], dtype=torch.int32)
    blen = torch.tensor([len(y) for _, y in pairs], dtype=torch.int32)
    d = ops.edit_distance(torch.from_numpy(a).to(DEV), alen.to(DEV), torch.from_numpy(b).to(DEV), blen.to(DEV))
    torch.cuda.synchronize()
    return d.cpu().tolist()


def test_edit_distance_lengths_across_wave_chunk_and_tail():
    rng = np.random.default_rng(0)

    def seq(n):
        return rng.integers(0, 3, n).tolist()
    same64 = seq(64)
    pairs = [([], []), ([], seq(5)), (seq(5), []), ([1], [1]), ([1], [2]), (seq(63), seq(64)), (same64, list(same64)),
             ([0] * 64, [1] * 64), (seq(65), seq(63)), (seq(130), seq(257)), (seq(257), seq(130)), (seq(1000), seq(1)),
             (seq(1), seq(1000)), (seq(1031), seq(997))]
    assert len(pairs) == 14
    # padding that would match: the same symbol on both sides of a row, so reading past a length lowers the distance
    got = run_edit_distance(pairs, 1040, 1048, lambda i, w: np.full(w, i % 3, np.int64))
    want = [levenshtein(x, y) for x, y in pairs]
    assert got == want
    assert want[6] == 0 and want[7] == 64 and want[1] == 5 and want[2] == 5


def test_edit_distance_single_pair_and_upper_bits():
    rng = np.random.default_rng(1)
    x, y = rng.integers(0, 3, 70).tolist(), rng.integers(0, 3, 90).tolist()
    assert run_edit_distance([(x, y)], 96, 96, lambda i, w: np.zeros(w, np.int64)) == [levenshtein(x, y)]
    # symbols that differ only in their upper 32 bits are different symbols
    hi = 1 << 32
    x = [5, 5 + hi, 5 + 2 * hi, 7]
    y = [5 + hi, 5 + hi, 5, 7 + hi]
    assert levenshtein(x, y) == 3
    assert run_edit_distance([(x, y)], 8, 8, lambda i, w: np.full(w, 5, np.int64)) == [3]


def test_edit_distance_rows_in_the_workspace():
    """the DP rows leave LDS for the caller's workspace above 4096 entries (n + 1): columns 4094 .. 4097 straddle it, and a
    row of more than 8192 symbols has no cap of its own; a thread then owns up to 36 columns"""
    rng = np.random.default_rng(2)
    pairs = [(rng.integers(0, 3, 3).tolist(), rng.integers(0, 3, n).tolist()) for n in (4094, 4095, 4096, 4097)]
    pairs.append((rng.integers(0, 3, 9000).tolist(), rng.integers(0, 3, 5).tolist()))
    got = run_edit_distance(pairs, 9010, 9010, lambda i, w: np.full(w, i % 3, np.int64))
    assert got == [levenshtein(x, y) for x, y in pairs]


# ---- eamd_text_units ---------------------------------------------------------------------------------------------------------
def python_units(tokens, table_rows, ids, limit, collapse, drop_space, words):
    """what the reference's string handling gives for one id row under a token table (rows of code points per id)"""
    ids = [int(v) for v in ids]
    if limit is not None:
        ids = ids[:limit]
    if collapse:
        ids = [k for k, _ in groupby(ids)]
    text = "".join("".join(chr(c) for c in table_rows[i]) for i in ids if i != -1)
    if words:
        return text.split()
    return list(text.replace(" ", "") if drop_space else text)


def equality_pattern(seq):
    first = {}
    return [first.setdefault(s, len(first)) for s in seq]


@pytest.mark.parametrize("name", LISTS)
def test_text_units_against_python_strings(name):
    from espnet_amd import ops
    from espnet_amd.nets.e2e_asr_common import ErrorCalculator
    g = load_golden("error_calc.npz")
    tokens, space, blank = golden_case(g, name)
    ec = ErrorCalculator(tokens, space, blank, True, True)
    V = len(tokens)
    rng = np.random.default_rng(5)
    B, L = 9, 300                                  # more than one pass of 256 positions
    ids = rng.integers(0, V, (B, L)).astype(np.int32)
    rep = rng.random((B, L)) < 0.3
    for j in range(1, L):
        ids[rep[:, j], j] = ids[rep[:, j], j - 1]
    ids[rng.random((B, L)) < 0.1] = -1
    ids[0] = -1                                    # a row that is all -1
    ids[1] = 0                                     # only blanks: no characters and no words under the hyp table
    sp = ec.idx_space if ec.idx_space is not None else 0
    ids[2, :] = sp
    ids[2, 7] = -1                                 # spaces only (char list): zero words
    ids[3, :40] = ids[3, 40:80]                    # equal words / pieces in one row
    limit = rng.integers(0, L + 1, B).astype(np.int32)
    limit[4], limit[5] = 0, L
    ids_d, limit_d = torch.from_numpy(ids).to(DEV), torch.from_numpy(limit).to(DEV)
    for key in ("hyp", "ref", "ctc"):
        off, cp, longest = ec.tables[key]
        rows = [cp[a:b] for a, b in zip(off, off[1:])]
        off_d, cp_d = torch.tensor(off, dtype=torch.int32).to(DEV), torch.tensor(cp, dtype=torch.int32).to(DEV)
        cap = L * longest
        for words in (False, True):
            for collapse in (False, True):
                for lim in (None, limit):
                    for drop in ((False, True) if not words else (False,)):
                        out, n = ops.text_units(ids_d, off_d, cp_d, cap, limit=None if lim is None else limit_d,
                                                collapse=collapse, drop_cp=0x20 if drop else -1,
                                                mode=ops.TEXT_WORDS if words else ops.TEXT_CHARS)
                        torch.cuda.synchronize()
                        out, n = out.cpu().numpy(), n.cpu().tolist()
                        for b in range(B):
                            want = python_units(tokens, rows, ids[b], None if lim is None else int(lim[b]), collapse, drop,
                                                words)
                            got = out[b, :n[b]].tolist()
                            what = (key, words, collapse, lim is not None, drop, b)
                            assert n[b] == len(want), what
                            if words:      # 64-bit hashes: equal words <-> equal symbols
                                assert equality_pattern(got) == equality_pattern(want), what
                            else:
                                assert got == [ord(c) for c in want], what
        if key == "hyp":
            out, n = ops.text_units(ids_d, off_d, cp_d, cap, mode=ops.TEXT_WORDS)
            n = n.cpu().tolist()
            assert n[0] == 0 and n[1] == 0 and n[2] == 0 and n[3] > 0      # zero words: all -1, blanks only, spaces only


# ---- ErrorCalculator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LISTS)
def test_error_calculator_equals_the_reference(name):
    from espnet_amd.nets.e2e_asr_common import ErrorCalculator
    g = load_golden("error_calc.npz")
    tokens, space, blank = golden_case(g, name)
    ec = ErrorCalculator(tokens, space, blank, report_cer=True, report_wer=True)
    hat, pad = torch.from_numpy(g[name + "_att_hat"]).to(DEV), torch.from_numpy(g[name + "_ys_pad"]).to(DEV)
    ctc_hat = torch.from_numpy(g[name + "_ctc_hat"]).to(DEV)
    chars, words = ec.counts(hat, pad)
    ctc = ec.counts(ctc_hat, pad, is_ctc=True)
    for (e, n), key in ((chars, "char"), (words, "word"), (ctc, "ctc")):
        assert e.dtype == torch.int32 and n.dtype == torch.int32 and e.is_cuda and n.is_cuda
        assert e.cpu().tolist() == g[f"{name}_{key}_ed"].tolist() and n.cpu().tolist() == g[f"{name}_{key}_len"].tolist()
    assert ec(hat, pad) == (float(g[name + "_cer"]), float(g[name + "_wer"]))
    assert ec(ctc_hat, pad, is_ctc=True) == float(g[name + "_cer_ctc"])
    # the reference's None cases and its ZeroDivisionError on a batch of empty references
    only_cer = ErrorCalculator(tokens, space, blank, report_cer=True)
    assert only_cer(hat, pad) == (float(g[name + "_cer"]), None)
    assert ErrorCalculator(tokens, space, blank, report_wer=True)(hat, pad) == (None, float(g[name + "_wer"]))
    assert ErrorCalculator(tokens, space, blank)(hat, pad) == (None, None)
    empty = torch.full_like(pad[:2], -1)
    assert ec(ctc_hat[:2], empty, is_ctc=True) is None
    with pytest.raises(ZeroDivisionError):
        ec(hat[:2], empty)


# ---- models ------------------------------------------------------------------------------------------------------------------
CHARS50 = ["<blank>", "<unk>", "<space>"] + [chr(ord("a") + i) for i in range(26)] + [chr(ord("A") + i) for i in range(20)] + \
    ["<eos>"]
SP, BL = "<space>", "<blank>"


def expected_rates(tokens, ctc_ids, att_ids, ys):
    """the reference's three numbers from id arrays read back to the host"""
    ys = np.asarray(ys)
    out = {}
    if ctc_ids is not None:
        out["cer_ctc"] = rate(*ctc_counts(tokens, SP, BL, np.asarray(ctc_ids), ys))
    if att_ids is not None:
        hats, trues = convert_to_char(tokens, SP, BL, np.asarray(att_ids), ys)
        out["cer"], out["wer"] = rate(*char_counts(hats, trues)), rate(*word_counts(hats, trues))
    return out


def _espnet1(kind, **flags):
    from espnet_amd.nets import e2e_asr_conformer, e2e_asr_transformer
    ns = argparse.Namespace(adim=64, aheads=4, elayers=2, eunits=128, dlayers=1, dunits=128, mtlalpha=0.3, lsm_weight=0.1,
                            dropout_rate=0.0, transformer_length_normalized_loss=False, **flags)
    if kind == "conformer":
        cls = e2e_asr_conformer.E2E
        ns.transformer_encoder_pos_enc_layer_type, ns.transformer_encoder_selfattn_layer_type = "rel_pos", "rel_selfattn"
        ns.macaron_style, ns.use_cnn_module, ns.cnn_module_kernel = True, True, 15
    else:
        cls = e2e_asr_transformer.E2E
        ns.eunits = ns.dunits = 256
    return seeded_weights().fill_parameters(cls(20, 50, ns), salt=77).to(DEV)


def _batch50():
    g = load_golden("e2e_transformer.npz")
    ys = g["ys"].copy()
    ys[ys == 0] = 3                          # labels are never blank
    ys[0, 2] = 2                             # a space, so that references have two words
    return torch.from_numpy(g["xs"]).to(DEV), g["ilens"].tolist(), torch.from_numpy(ys).to(DEV), ys


@pytest.mark.parametrize("kind", ["transformer", "conformer"])
def test_espnet1_transformer_reports_error_rates(kind):
    xs, ilens, ys_d, ys = _batch50()
    model = _espnet1(kind, report_cer=True, report_wer=True, char_list=CHARS50).eval()
    assert model.error_calculator is not None
    with torch.no_grad():
        model(xs, ilens, ys_d)
        want = expected_rates(CHARS50, model.ctc.argmax(model.hs_pad).cpu().numpy(), model.pred_pad.argmax(-1).cpu().numpy(), ys)
    last = model.reporter.last
    print(kind, {k: last[k] for k in ("cer_ctc", "cer", "wer")}, want)
    assert {k: last[k] for k in ("cer_ctc", "cer", "wer")} == want
    # deferred report: forward launches only, _report() reads the counts with the other scalars
    model.sync_report = False
    model.reporter.last = {}
    with torch.no_grad():
        model(xs, ilens, ys_d)
    assert model.reporter.last == {} and model._cer_n[0].is_cuda and model._cer_ctc_n[0].dtype == torch.int32
    model._report()
    assert {k: model.reporter.last[k] for k in ("cer_ctc", "cer", "wer")} == want
    model.sync_report = True
    # training mode: nothing is scored
    model.train()
    model(xs, ilens, ys_d)
    assert [model.reporter.last[k] for k in ("cer_ctc", "cer", "wer")] == [None, None, None]
    # one flag only
    model = _espnet1(kind, report_wer=True, char_list=CHARS50).eval()
    with torch.no_grad():
        model(xs, ilens, ys_d)
    assert model.reporter.last["cer"] is None and model.reporter.last["wer"] == want["wer"]
    assert model.reporter.last["cer_ctc"] == want["cer_ctc"]


def test_default_flags_report_none():
    from espnet_amd.nets import e2e_asr_maskctc
    xs, ilens, ys_d, _ = _batch50()
    model = _espnet1("transformer").eval()
    assert model.error_calculator is None
    with torch.no_grad():
        model(xs, ilens, ys_d)
    assert [model.reporter.last[k] for k in ("cer_ctc", "cer", "wer")] == [None, None, None]
    assert model.reporter.last["loss"] is not None
    assert e2e_asr_maskctc.E2E.reports_errors is False


def test_espnet2_model_stats():
    from espnet_amd import ops
    from espnet_amd.espnet2 import CTC, ConformerEncoder, ESPnetASRModel, TransformerDecoder
    tokens = CHARS50[:29] + ["<eos>"]

    def build(**kw):
        enc = ConformerEncoder(20, output_size=64, attention_heads=4, linear_units=96, num_blocks=2, dropout_rate=0.0,
                               positional_dropout_rate=0.0, attention_dropout_rate=0.0, macaron_style=True, cnn_module_kernel=7)
        dec = TransformerDecoder(30, 64, attention_heads=4, linear_units=96, num_blocks=1, dropout_rate=0.0,
                                 positional_dropout_rate=0.0)
        m = ESPnetASRModel(vocab_size=30, token_list=tokens, encoder=enc, decoder=dec, ctc=CTC(30, 64, ctc_type="builtin"),
                           ctc_weight=0.3, lsm_weight=0.1, **kw)
        return seeded_weights().fill_parameters(m, salt=78).to(DEV)
    g = load_golden("espnet2_model.npz")
    speech, sl, tl = torch.from_numpy(g["speech"]).to(DEV), torch.from_numpy(g["speech_lengths"]), torch.from_numpy(g["text_lengths"])
    text = g["text"].copy()
    text[text == 0] = 3
    text[0, 1] = 2
    text_d = torch.from_numpy(text).to(DEV)
    model = build(report_cer=True, report_wer=True).eval()
    with torch.no_grad():
        loss, stats, _ = model(speech, sl, text_d, tl)
        enc_out, enc_lens = model.encode(speech, sl)
        tlist = tl.tolist()
        t = text_d[:, : max(tlist)].contiguous()
        ys_in, _, _ = ops.add_sos_eos(t, model.sos, model.eos, model.ignore_id)
        dec_out, _ = model.decoder(enc_out, enc_lens, ys_in, [v + 1 for v in tlist])
        want = expected_rates(tokens, model.ctc.argmax(enc_out).cpu().numpy(), dec_out.argmax(-1).cpu().numpy(),
                              t.cpu().numpy())
    for k in ("cer", "wer", "cer_ctc"):
        assert stats[k].shape == (1,) and stats[k].device == loss.device
        assert float(stats[k]) == float(np.float32(want[k])), (k, float(stats[k]), want[k])
    model.train()
    _, stats, _ = model(speech, sl, text_d, tl)
    assert stats["cer"] is None and stats["wer"] is None and stats["cer_ctc"] is None
    model = build().eval()
    assert model.error_calculator is None
    with torch.no_grad():
        _, stats, _ = model(speech, sl, text_d, tl)
    assert stats["cer"] is None and stats["wer"] is None and stats["cer_ctc"] is None


def test_rnn_e2e_reports_error_rates():
    from espnet_amd.nets.e2e_asr import E2E
    tokens = ["<blank>", "a", "b", "<space>", "d", "e", "<eos>"]
    d = dict(elayers=2, subsample="1_2_1", etype="blstmp", eunits=12, eprojs=10, dtype="lstm", dlayers=1, dunits=14,
             atype="location", aheads=1, awin=3, aconv_chans=3, aconv_filts=2, mtlalpha=0.5, lsm_type="", lsm_weight=0.0,
             sampling_probability=0.0, adim=9, dropout_rate=0.0, dropout_rate_decoder=0.0, verbose=0, char_list=tokens,
             outdir=None, ctc_type="builtin", sym_space=SP, sym_blank=BL, context_residual=False, use_frontend=False,
             replace_sos=False)
    beam = dict(report_cer=True, report_wer=True, beam_size=2, penalty=0.0, ctc_weight=0.3, maxlenratio=0.0, minlenratio=0.0,
                lm_weight=0.0, rnnlm=None, nbest=1)
    g = torch.Generator().manual_seed(4)
    xs = torch.nn.utils.rnn.pad_sequence([torch.randn(T, 12, generator=g) for T in (40, 33, 27)], batch_first=True).to(DEV)
    ilens = [40, 33, 27]
    ys = np.array([[1, 2, 3, 4, 5], [4, 4, 1, -1, -1], [-1, -1, -1, -1, -1]], np.int64)
    ys_d = torch.from_numpy(ys).to(DEV)

    def greedy_text_cer(m):
        ids = m.ctc.argmax(m.hs_pad).cpu().numpy()
        cers = []
        for y, y_true in zip(ids, ys):
            hyp = "".join(tokens[k] for k, _ in groupby(int(v) for v in y) if k != -1).replace(SP, " ").replace(BL, "")
            ref = "".join(tokens[int(i)] for i in y_true if int(i) != -1).replace(SP, " ")
            hyp, ref = hyp.replace(" ", ""), ref.replace(" ", "")
            if len(ref) > 0:
                cers.append(levenshtein(hyp, ref) / len(ref))
        return sum(cers) / len(cers)

    m = seeded_weights().fill_parameters(E2E(12, 7, argparse.Namespace(**d, **beam)), salt=79).to(DEV).eval()
    with torch.no_grad():
        m(xs, ilens, ys_d)
        assert m.cer_ctc == greedy_text_cer(m)
        lpz = m.ctc.log_softmax(m.hs_pad)
        nbest = m.dec.recognize_beam_batch(m.hs_pad, m.hlens, lpz, m.recog_args, tokens, None)
    hats, trues = [], []
    for hyp, y_true in zip(nbest, ys):
        hats.append("".join(tokens[int(i)] for i in hyp[0]["yseq"][1:-1] if int(i) != -1).replace(SP, " ").replace(BL, ""))
        trues.append("".join(tokens[int(i)] for i in y_true if int(i) != -1).replace(SP, " "))
    assert m.cer == rate(*char_counts(hats, trues)) and m.wer == rate(*word_counts(hats, trues))
    # training: cer / wer are 0.0, the greedy CTC rate is still there; without the flags as well
    m.train()
    m(xs, ilens, ys_d)
    assert (m.cer, m.wer) == (0.0, 0.0) and m.cer_ctc == greedy_text_cer(m)
    m = seeded_weights().fill_parameters(E2E(12, 7, argparse.Namespace(**d)), salt=79).to(DEV).eval()
    with torch.no_grad():
        m(xs, ilens, ys_d)
    assert (m.cer, m.wer) == (0.0, 0.0) and m.cer_ctc == greedy_text_cer(m)
    d["char_list"] = None
    m = E2E(12, 7, argparse.Namespace(**d)).to(DEV).eval()
    with torch.no_grad():
        m(xs, ilens, ys_d)
    assert m.error_calculator is None and m.cer_ctc is None


def test_transducer_e2e_reports_error_rates():
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    from espnet_amd.nets.e2e_asr_transducer import E2E
    tokens = ["<blank>", "a", "b", "<space>", "d", "<eos>"]
    d = dict(etype="blstmp", elayers=1, subsample="1_1", eunits=10, eprojs=8, dtype="lstm", dlayers=2, dunits=12,
             dec_embed_dim=6, dropout_rate=0.0, dropout_rate_decoder=0.0, dropout_rate_embed_decoder=0.0, joint_dim=7,
             joint_activation_type="tanh", rnnt_mode="rnnt", trans_type="warp-transducer", sym_space=SP, sym_blank=BL,
             transformer_init="pytorch")
    g = torch.Generator().manual_seed(8)
    xs = torch.nn.utils.rnn.pad_sequence([torch.randn(T, 12, generator=g) for T in (30, 22)], batch_first=True).to(DEV)
    ilens = [30, 22]
    ys = np.array([[1, 3, 2, 4], [2, 1, -1, -1]], np.int64)
    ys_d = torch.from_numpy(ys).to(DEV)
    m = E2E(12, 6, argparse.Namespace(**d, report_cer=True, report_wer=True, char_list=tokens))
    m = seeded_weights().fill_parameters(m, salt=80).to(DEV).eval()
    with torch.no_grad():
        m(xs, ilens, ys_d)
        search = BeamSearchTransducer(m.dec, beam_size=1)
        ys_hat = [list(search(m.hs_pad[b]).yseq[1:]) for b in range(2)]
    hats, trues = [], []
    for y_hat, y_true in zip(ys_hat, ys):
        y_true = [int(v) for v in y_true]
        ymax = y_true.index(-1) if -1 in y_true else len(y_true)
        hats.append("".join(tokens[i] for i in y_hat[:ymax]).replace(SP, " ").replace(BL, ""))
        trues.append("".join(tokens[i] for i in y_true if i != -1).replace(SP, " "))
    assert (m.cer, m.wer) == (rate(*char_counts(hats, trues)), rate(*word_counts(hats, trues)))
    m.train()
    m(xs, ilens, ys_d)
    assert m.cer is None and m.wer is None
    m = E2E(12, 6, argparse.Namespace(**d)).to(DEV).eval()
    assert m.error_calculator is None
