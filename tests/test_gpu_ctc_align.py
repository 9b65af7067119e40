"""CTC forced alignment on the GPU (eamd_ctc_forced_align, ops.ctc_forced_align, CTC.forced_align / forced_align_batch,
nets.ctc_align.ctc_align_batch): token paths pinned to the reference's CTC.forced_align (tests/golden/ctc_align.npz) and to the
float32 restatement of tests/test_ctc_align.py on random batches, ties, edge cases and long transcripts."""
from itertools import groupby

import numpy as np
import pytest
import torch

from conftest import load_golden, seeded_weights
from test_ctc_align import FIXTURE_CASES, extend, log_softmax64, segments, viterbi_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_align(acts, ilens, ys, normalized=False, time_major=False):
    from espnet_amd import ops
    a = torch.from_numpy(np.ascontiguousarray(acts)).to(DEV)
    out = ops.ctc_forced_align(a, torch.as_tensor(ilens, dtype=torch.int32).to(DEV), torch.from_numpy(ys).to(DEV),
                               normalized=normalized, time_major=time_major)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def pad_labels(labels, L=None):
    L = max([len(y) for y in labels] + [1]) if L is None else L
    ys = np.full((len(labels), L), -1, np.int64)
    for b, y in enumerate(labels):
        ys[b, :len(y)] = y
    return ys


def check_utterance(out, b, em, y, T, exact_score):
    """one utterance of a batch result against the restatement on emissions em [Tb, S]"""
    score, states, tokens, start, end = out
    ext = extend(y)
    Tb = em.shape[0]
    rs, rp = viterbi_ref(em, ext)
    if rp is None:
        assert score[b] == -np.inf and (states[b] == -1).all() and (tokens[b] == -1).all()
        assert (start[b] == -1).all() and (end[b] == -1).all()
        return
    assert states[b, :Tb].tolist() == rp.tolist(), b
    assert tokens[b, :Tb].tolist() == ext[rp].tolist(), b
    assert (states[b, Tb:] == -1).all() and (tokens[b, Tb:] == -1).all()
    rstart, rend = segments(rp, len(y))
    assert start[b, :len(y)].tolist() == rstart.tolist() and end[b, :len(y)].tolist() == rend.tolist()
    assert (start[b, len(y):] == -1).all() and (end[b, len(y):] == -1).all()
    if exact_score:
        assert np.float32(score[b]) == rs, (b, score[b], rs)
    else:
        assert abs(float(score[b]) - float(rs)) <= 1e-5 * max(1.0, abs(float(rs))), (b, score[b], rs)


# ---- 1. the reference's own log-posteriors through the normalized mode: its paths exactly ----------------------------------
@pytest.mark.parametrize("u,kind", FIXTURE_CASES)
def test_align_reference_lpz_exact(u, kind):
    g = load_golden("ctc_align.npz")
    tag = "u%d_%s" % (u, kind)
    ids, lpz, y = g[tag + "_ids"], g[tag + "_lpz"], g[tag + "_label"]
    col = {int(v): i for i, v in enumerate(ids)}
    yc = np.asarray([col[int(v)] for v in y], np.int64)        # labels as columns of the compact [T', K] matrix
    T = lpz.shape[0]
    out = run_align(lpz[None], [T], yc[None], normalized=True)
    assert ids[out[2][0]].tolist() == g[tag + "_align"].tolist()
    ext = extend(yc)
    check_utterance(out, 0, lpz[:, ext], yc, T, exact_score=True)
    print(f"[parity] ctc align {tag}: T'={T} L={len(y)} path exact, score {out[0][0]:.4f}")


# ---- 2. model level: our Conformer's CTC layer on the reference encoder outputs, on our encoder outputs, and batched -------
_MODEL = {}


def r4_model():
    if not _MODEL:
        from espnet_amd.nets.e2e_asr_conformer import E2E
        SW = seeded_weights()
        _MODEL.update(SW=SW, model=SW.decode_r4_model(E2E).to(DEV).eval())
    return _MODEL["SW"], _MODEL["model"]


def test_align_model_level_against_reference():
    SW, model = r4_model()
    g = load_golden("ctc_align.npz")
    encs = [model.encode(x) for x in SW.decode_r4_inputs()]
    for u in range(3):
        ref_enc = torch.from_numpy(g["u%d_enc" % u]).to(DEV)
        for kind in ("short", "repeats", "tight"):
            tag = "u%d_%s" % (u, kind)
            y, ref = g[tag + "_label"], g[tag + "_align"].tolist()
            assert model.ctc.forced_align(ref_enc.unsqueeze(0), y) == ref, (tag, "reference encoder output")
            assert model.ctc.forced_align(encs[u], torch.from_numpy(y)) == ref, (tag, "our encoder output")
    print("[parity] ctc align model level: 9 alignments exact on the reference's and on our encoder outputs")


def test_align_batch_helper_matches_single_utterances():
    from espnet_amd.nets.ctc_align import ctc_align_batch
    SW, model = r4_model()
    g = load_golden("ctc_align.npz")
    xs = SW.decode_r4_inputs()
    il = [x.shape[0] for x in xs]
    xs_pad = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True)
    ys = pad_labels([g["u%d_repeats_label" % u] for u in range(3)])
    single = ctc_align_batch(model, xs[0][None], [il[0]], ys[:1])
    batch = ctc_align_batch(model, xs_pad, il, ys)
    # the longest utterance has no padding: its path is the one it has alone, the reference's.  (The Conformer convolution
    # module has no mask - in the reference as here - so the shorter utterances' last frames see the padding.)
    assert batch.tokens[0].tolist() == single.tokens[0].tolist()
    assert batch.tokens[0].tolist() == g["u0_repeats_align"].tolist()
    # every utterance: one alignment pass over the batch = the alignment of that utterance's rows of the batch's encoder output
    # alone, over the valid frames of the reference's subsampled mask (a padded utterance keeps one frame more than the two
    # stride-2 convolutions give it unpadded: 160 vs 159 for 640 input frames, as in the reference's batches)
    from espnet_amd.nets.ctc_align import encode_batch
    from espnet_amd.nets.modules import embed_output_lengths
    hs, hl = encode_batch(model, xs_pad, il)
    assert hl == embed_output_lengths(model.encoder.embed, il, max(il))
    for u in range(3):
        Lu = len(g["u%d_repeats_label" % u])
        one = model.ctc.forced_align_batch(hs[u:u + 1, :hl[u]], [hl[u]], ys[u:u + 1, :Lu])
        assert batch.tokens[u, :hl[u]].tolist() == one.tokens[0].tolist(), u
        assert (batch.tokens[u, hl[u]:] == -1).all() and (batch.tokens[u, :hl[u]] != -1).all()
        assert batch.start[u, :Lu].tolist() == one.start[0].tolist() and batch.end[u, :Lu].tolist() == one.end[0].tolist()
        assert abs(float(batch.score[u]) - float(one.score[0])) <= 1e-5 * abs(float(one.score[0]))


# ---- 3. random ragged batches, both layouts, against the restatement -----------------------------------------------------
def random_batch(rng, B, T, V, Lmax):
    x = (rng.standard_normal((B, T, V)) * 3).astype(np.float32)
    ilens = rng.integers(T // 2, T + 1, B)
    ilens[0] = T
    labels = []
    for b in range(B):
        L = int(rng.integers(0, Lmax + 1))
        y = rng.integers(1, V, L)
        for i in range(1, L):
            if rng.random() < 0.3:
                y[i] = y[i - 1]
        labels.append(y)
    return x, ilens, labels


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("normalized", [False, True])
def test_align_random_batches(time_major, normalized):
    rng = np.random.default_rng(11 + 2 * time_major + normalized)
    B, T, V, Lmax = 8, 120, 5000, 40
    x, ilens, labels = random_batch(rng, B, T, V, Lmax)
    labels[1] = labels[1][:0]                                         # an empty transcript
    labels[2] = np.repeat(labels[2][:20], 2)[:40] if len(labels[2]) else labels[2]   # many adjacent repeats
    lp = log_softmax64(x).astype(np.float32)
    acts = lp if normalized else x
    ys = pad_labels(labels, Lmax + 3)
    out = run_align(acts.transpose(1, 0, 2) if time_major else acts, ilens, ys, normalized=normalized, time_major=time_major)
    for b in range(B):
        check_utterance(out, b, lp[b, :ilens[b]][:, extend(labels[b])], labels[b], T, exact_score=normalized)
    print(f"[parity] ctc align random B={B} T={T} V={V} time_major={time_major} normalized={normalized}: paths exact, "
          f"scores {np.round(out[0], 3).tolist()}")


# ---- 4. exact ties everywhere: the first-maximum path ---------------------------------------------------------------------
def test_align_ties_take_first_maximum():
    rng = np.random.default_rng(5)
    B, T, V = 4, 60, 300
    x = np.zeros((B, T, V), np.float32)
    labels = [rng.integers(1, V, L) for L in (7, 20, 1, 29)]
    labels[1][3] = labels[1][2]
    out = run_align(x, [T] * B, pad_labels(labels))
    lp = log_softmax64(x).astype(np.float32)
    for b in range(B):
        check_utterance(out, b, lp[b][:, extend(labels[b])], labels[b], T, exact_score=False)


# ---- 5. edge cases ---------------------------------------------------------------------------------------------------------
def test_align_edge_cases():
    from espnet_amd import _lib
    from espnet_amd.nets import modules as M
    rng = np.random.default_rng(9)
    V, T = 50, 30
    lp = log_softmax64(rng.standard_normal((4, T, V)) * 2).astype(np.float32)
    tight = np.array([3, 3, 5, 8, 8, 8, 2, 9, 4, 4, 6, 7, 1, 12, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22])  # 25 labels + 5 repeats
    assert len(tight) + int(np.sum(tight[1:] == tight[:-1])) == T
    labels = [np.zeros(0, np.int64), tight, np.concatenate([tight, [21]]), rng.integers(1, V, 3)]
    ilens = [T, T, T, 1]
    out = run_align(lp, ilens, pad_labels(labels), normalized=True)
    assert out[2][0].tolist() == [0] * T                                                   # L = 0: all blank
    for b in range(4):
        check_utterance(out, b, lp[b, :ilens[b]][:, extend(labels[b])], labels[b], T, exact_score=True)
    assert out[0][2] == -np.inf and (out[1][2] == -1).all() and (out[3][2] == -1).all()   # infeasible
    assert out[0][3] == -np.inf                                                            # 3 labels in 1 frame
    # T' = 1
    out = run_align(lp[:2, :1], [1, 1], pad_labels([[7], []]), normalized=True)
    assert out[2][:, 0].tolist() == [7, 0] and out[1][:, 0].tolist() == [1, 0] and out[3][0, 0] == 0 and out[4][0, 0] == 0
    # CTC.forced_align: ValueError for an infeasible pair, the reference's list otherwise
    ctc = M.CTC(V, 16, 0.0).to(DEV)
    h = torch.randn(5, 16, device=DEV)
    with pytest.raises(ValueError):
        ctc.forced_align(h, [1, 2, 3, 4, 5, 6])
    with pytest.raises(ValueError):
        ctc.forced_align(h, [1, 1, 1, 1])                           # 4 labels + 3 repeats > 5 frames
    got = ctc.forced_align(h.unsqueeze(0), [4, 4])
    assert isinstance(got, list) and len(got) == 5 and [k for k, _ in groupby(got) if k] == [4, 4]
    assert ctc.forced_align(h, []) == [0] * 5
    # the longest transcript a workgroup holds: Lmax = 2047 (S = 4095) over 4100 frames
    T2, L2 = 4100, 2047
    x = (rng.standard_normal((1, T2, 40)) * 2).astype(np.float32)
    y = rng.integers(1, 40, L2)
    out = run_align(x, [T2], y[None])
    check_utterance(out, 0, log_softmax64(x[0]).astype(np.float32)[:, extend(y)], y, T2, exact_score=False)
    # one more label is refused on the host, nothing launched
    with pytest.raises(_lib.EamdError, match="code -2"):
        run_align(x[:, :8], [8], rng.integers(1, 40, (1, 2048)))


# ---- 6. consistency with the CTC loss: the best path is at most the sum over all paths ----------------------------------------
def test_align_score_below_ctc_loglik():
    from espnet_amd import ops
    rng = np.random.default_rng(21)
    B, T, V, Lmax = 8, 90, 500, 30
    x, ilens, labels = random_batch(rng, B, T, V, Lmax)
    ys = pad_labels(labels)
    out = run_align(x, ilens, ys)
    nll, _ = ops.ctc_loss(torch.from_numpy(x).to(DEV), torch.from_numpy(ys).to(DEV),
                          torch.as_tensor(ilens, dtype=torch.int32).to(DEV), want_grad=False)
    nll = nll.cpu().numpy()
    for b in range(B):
        if np.isfinite(nll[b]):
            assert out[0][b] <= -nll[b] + 1e-4 * max(1.0, abs(nll[b])), (b, out[0][b], -nll[b])
        else:
            assert out[0][b] == -np.inf


# ---- 7. segments follow the states ------------------------------------------------------------------------------------------
def test_align_segments_follow_states():
    rng = np.random.default_rng(33)
    B, T, V, Lmax = 8, 150, 1000, 50
    x, ilens, labels = random_batch(rng, B, T, V, Lmax)
    score, states, tokens, start, end = run_align(x, ilens, pad_labels(labels))
    for b in range(B):
        L = len(labels[b])
        if score[b] == -np.inf:
            continue
        for i in range(L):
            frames = np.nonzero(states[b] == 2 * i + 1)[0]
            assert frames.size and frames[0] == start[b, i] and frames[-1] == end[b, i]
            assert (states[b, start[b, i]:end[b, i] + 1] == 2 * i + 1).all()
            assert (tokens[b, start[b, i]:end[b, i] + 1] == labels[b][i]).all()
        assert (np.diff(start[b, :L]) >= 0).all() and (end[b, :L - 1] < start[b, 1:L]).all()


# ---- the helper on the other model families: espnet1 RNN E2E (enc) and espnet2 ESPnetASRModel (encode) --------------------
def batch_vs_alone(model, xs, labels):
    """ctc_align_batch on the padded batch against each utterance alone (recurrent encoders over packed lengths: no padding
    reaches the valid frames), and the caller's train / eval mode left as it was"""
    from espnet_amd.nets.ctc_align import ctc_align_batch
    il = [x.shape[0] for x in xs]
    xs_pad = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True)
    ys = pad_labels(labels)
    model.train()
    batch = ctc_align_batch(model, xs_pad, il, ys)
    assert model.training
    for u, (x, y) in enumerate(zip(xs, labels)):
        one = ctc_align_batch(model, x[None], [il[u]], y[None])
        Tu = one.tokens.shape[1]
        assert batch.tokens[u, :Tu].tolist() == one.tokens[0].tolist(), u
        assert (batch.tokens[u, Tu:] == -1).all()
        assert batch.start[u, :len(y)].tolist() == one.start[0].tolist() and batch.end[u, :len(y)].tolist() == one.end[0].tolist()
        assert abs(float(batch.score[u]) - float(one.score[0])) <= 1e-5 * max(1.0, abs(float(one.score[0])))
        assert np.isfinite(float(one.score[0])) and [k for k, _ in groupby(one.tokens[0].tolist()) if k] == y.tolist()
    return batch


def test_align_batch_helper_rnn_e2e():
    import argparse
    from espnet_amd.nets.e2e_asr import E2E
    torch.manual_seed(3)
    args = argparse.Namespace(
        elayers=2, subsample="1_2_1", etype="blstmp", eunits=12, eprojs=10, dtype="lstm", dlayers=1, dunits=14, atype="location",
        aheads=1, awin=3, aconv_chans=3, aconv_filts=2, mtlalpha=0.5, lsm_type="", lsm_weight=0.0, sampling_probability=0.0,
        adim=9, dropout_rate=0.0, dropout_rate_decoder=0.0, verbose=0, char_list=["<blank>", "a", "b", "c", "d", "e", "<eos>"],
        outdir=None, ctc_type="builtin", sym_space="<space>", sym_blank="<blank>", context_residual=False, use_frontend=False,
        replace_sos=False)
    model = E2E(12, 7, args).to(DEV)
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(T, 12, generator=g) for T in (40, 27, 33)]
    batch_vs_alone(model, xs, [np.array([1, 2, 2, 3, 5]), np.array([4, 4, 1]), np.array([2, 5, 1, 3])])


def test_align_batch_helper_espnet2_model():
    from espnet_amd.espnet2 import CTC, ESPnetASRModel, RNNDecoder, RNNEncoder
    torch.manual_seed(5)
    model = ESPnetASRModel(vocab_size=30, encoder=RNNEncoder(20, num_layers=2, hidden_size=12, output_size=10, subsample=(2, 1)),
                           decoder=RNNDecoder(30, 10, hidden_size=12, rnn_type="lstm", num_layers=1,
                                              att_conf=dict(atype="location", adim=8, aconv_chans=3, aconv_filts=4)),
                           ctc=CTC(30, 10, ctc_type="builtin"), ctc_weight=0.3).to(DEV)
    g = torch.Generator().manual_seed(6)
    xs = [torch.randn(T, 20, generator=g) for T in (50, 36)]
    labels = [np.array([3, 7, 7, 12, 28]), np.array([9, 1, 14])]
    batch_vs_alone(model, xs, labels)
    # the espnet2 wrapper's own entry points
    with torch.no_grad():
        hs, hl = model.encode(xs[1][None].to(DEV), torch.tensor([36]))
    assert model.ctc.forced_align(hs[0], labels[1]) == model.ctc.forced_align_batch(hs, hl, labels[1][None]).tokens[0].tolist()


# ---- a label outside the vocabulary is never read: no path on the device, ValueError from the module -----------------------
def test_align_out_of_vocabulary_label():
    from espnet_amd.nets import modules as M
    rng = np.random.default_rng(13)
    V, T = 30, 20
    x = (rng.standard_normal((3, T, V)) * 2).astype(np.float32)
    labels = [np.array([3, 4]), np.array([3, V]), np.array([-5, 2])]     # (-1 would be padding: -5 is a negative id)
    for normalized in (False, True):
        acts = log_softmax64(x).astype(np.float32) if normalized else x
        out = run_align(acts, [T] * 3, pad_labels(labels), normalized=normalized)
        assert np.isfinite(out[0][0]) and (out[2][0] != -1).all()
        for b in (1, 2):
            assert out[0][b] == -np.inf and (out[1][b] == -1).all() and (out[2][b] == -1).all()
            assert (out[3][b] == -1).all() and (out[4][b] == -1).all()
    ctc = M.CTC(V, 16, 0.0).to(DEV)
    with pytest.raises(ValueError):
        ctc.forced_align(torch.randn(T, 16, device=DEV), [3, V])
