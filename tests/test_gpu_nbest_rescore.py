"""Second-pass n-best rescoring on the GPU: eamd_nbest_pack / eamd_nbest_rescore (csrc/rescore.hip) against the float64
restatement (tests/rescore_restatement.py), Decoder.forward_nbest against Decoder.forward, NBestRescorer against the
reference's own searches (decode_c2width.npz, decode_fusion.npz), and the public surface end to end.

Kernel bound (a priori, the rule of the project's float64 kernel tests; RR.term_bound / RR.f_bound): (U + tiles_n + 8) * 2^-24
times the sum of the magnitudes added.  Measured on an MI355X: see KERNEL_MEASURED below.  Order is compared only after the
restatement's own adjacent gaps of f (other than the planted exact ties) have been shown to exceed 10 x that bound."""
import argparse
import math

import numpy as np
import pytest
import torch

import rescore_restatement as RR
from test_gpu_ops import report

pytestmark = pytest.mark.gpu
DEV = "cuda"

# largest |device - float64| / bound over the kernel cases, terms and f, measured on an MI355X (0.045 at V = 37; largest
# absolute error 1.05e-5 on a term of -197.55 at V = 5000, bound 9.25e-4; the bound itself stays the a-priori one)
KERNEL_MEASURED = 0.045
# model-level tolerance: c2width_compare's and test_decode_fusion_golden's for the same quantities
TOL = 1e-4
# end to end, device score against the float64 restatement on the model's ordinary fp32 forward, relative to max(1, |f|): 4 x the
# largest difference measured on an MI355X, 2.15e-7 (720 hypotheses over 15 seeds of either end-to-end case)
E2E_TOL = 8.6e-7


@pytest.fixture(autouse=True)
def _fp32():
    import espnet_amd
    espnet_amd.set_precision("fp32")
    yield
    espnet_amd.set_precision("fp32")


def f32(w):
    return float(np.float32(w))


# ---- kernels against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [7, 40])
@pytest.mark.parametrize("N", [1, 5, 32])
def test_nbest_pack_is_exact(N, T):
    """B = 3; rows with L = -1, 0 and T among random lengths; U = T + 1, and U below the longest length (the clamp)"""
    from espnet_amd import ops
    B, V = 3, 50
    g = torch.Generator().manual_seed(100 * N + T)
    special = [-1, 0, T]
    hyps = []
    for b in range(B):
        row = []
        for n in range(N):
            k = b * N + n
            L = special[k % 3] if (k < 3 or k % 5 == 0) else int(torch.randint(0, T + 1, (), generator=g))
            row.append(None if L < 0 else (float(torch.randn((), generator=g)), torch.randint(1, V - 1, (L,), generator=g).tolist()))
        hyps.append(row)
    nbest = RR.make_nbest(hyps, T)
    assert {-1, 0, T} <= set(nbest[:, :, 1].reshape(-1).tolist())
    for U in (T + 1, T // 2 + 1):
        ys_in, col, ulen = ops.nbest_pack(nbest.to(DEV), U, V, V - 1, V - 1)
        want = RR.pack(nbest, U, V - 1, V - 1)
        assert ys_in.dtype == torch.int64 and col.dtype == torch.int32 and ulen.dtype == torch.int32
        assert torch.equal(ys_in.cpu(), want[0]) and torch.equal(col.cpu(), want[1]) and torch.equal(ulen.cpu(), want[2])


BAD = 3          # the token whose logit is -inf under scorer 1


def kernel_case(V, seed, S):
    """B = 3, N = 5, T = 12, D = 64: utterance 0 holds two identical hypotheses (1 and 3: bit-equal f), utterance 1 two absent
    ones (1 and 3) in front of present ones, utterance 2 a hypothesis (2) whose term under scorer 1 is -inf.  Lengths include 0
    and T.  -> (hyps, nbest, U, per scorer (hidden [B*N*U, D], W [V, D], bias [V]) fp32, weights rounded to fp32)"""
    B, N, T, D = 3, 5, 12, 64
    g = torch.Generator().manual_seed(seed)
    lens = [[4, 7, 0, 7, T], [5, -1, 9, -1, 2], [6, 3, 8, 1, 10]]
    hyps = [[None if L < 0 else (float(4.0 * torch.randn((), generator=g)), torch.randint(BAD + 1, V - 1, (L,), generator=g).tolist())
             for L in ls] for ls in lens]
    hyps[0][3] = hyps[0][1]
    hyps[2][2][1][5] = BAD
    nbest = RR.make_nbest(hyps, T)
    U = T + 1
    scorers = []
    for s in range(S):
        hidden = 0.5 * torch.randn(B, N, U, D, generator=g)
        hidden[0, 3] = hidden[0, 1]
        W = 0.5 * torch.randn(V, D, generator=g)
        bias = torch.randn(V, generator=g)
        if s == 0:
            bias[BAD] = -math.inf
        scorers.append((hidden.reshape(B * N * U, D).contiguous(), W, bias))
    return hyps, nbest, U, scorers, (f32(0.3), [f32(0.7), f32(0.6)][:S])


def check_gaps(res, bound, ties, label):
    """every adjacent gap of the restatement's f among the present hypotheses, other than the planted exact ties (pairs of
    first-pass indices), exceeds 10 x the bound: only then is the device's order comparable"""
    B, N = res["f"].shape
    for b in range(B):
        for k in range(N - 1):
            if not (res["here"][b, k] and res["here"][b, k + 1]):
                continue
            pair = (b, int(res["order"][b, k]), int(res["order"][b, k + 1]))
            gap = float(res["f"][b, k] - res["f"][b, k + 1])
            if pair in ties:
                assert gap == 0.0, (label, pair, gap)
                continue
            need = 10.0 * float(max(bound[b, k], bound[b, k + 1]))
            assert gap > need, "%s: gap %.3e of utterance %d ranks %d / %d below 10 x bound %.3e: choose another seed" % (
                label, gap, b, k, k + 1, need / 10)


KERNEL_SEED = 11          # chosen on the CPU (float64 logits through RR.tile_partials): the gap precondition holds for every case


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("V", [37, 150, 5000])
def test_nbest_rescore_against_float64(V, tile, S):
    """one tile (V = 37), a ragged last tile (150) and many tiles (5000), with the 64- and the 128-column GEMM tile; one and two
    scorers.  The partials come from eamd_gemm's row-statistics epilogue itself; the restatement merges THE SAME partials in
    float64, so the bound covers eamd_nbest_rescore alone."""
    from espnet_amd import ops
    hyps, nbest, U, scorers, (w0, ws) = kernel_case(V, KERNEL_SEED, S)
    B, N, _ = nbest.shape
    nb = nbest.to(DEV)
    ys_in, col, ulen = ops.nbest_pack(nb, U, V, V - 1, V - 1)
    dev_sc, host_sc, tiles = [], [], []
    for (hidden, W, bias), w in zip(scorers, ws):
        part, zcol, tn = ops.row_target_stats(hidden.to(DEV), W.to(DEV), bias.to(DEV), col, tile=tile)
        assert tn == (V + tile - 1) // tile and part.shape == (B * N * U, tn, 2)
        dev_sc.append((part, zcol, tn, w))
        host_sc.append((part.cpu(), zcol.cpu(), w))
        tiles.append(tn)
    res = RR.rescore(nbest, U, host_sc, w0)
    bound = RR.f_bound(res, ws, w0, U, tiles)
    label = "V %d tile %d S %d" % (V, tile, S)
    check_gaps(res, bound, {(0, 1, 3)}, label)
    out, terms, order = ops.nbest_rescore(nb, ulen, U, dev_sc, w0)
    again = ops.nbest_rescore(nb, ulen, U, dev_sc, w0)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((out, terms, order), again))      # same bits
    out, terms, order = out.cpu(), terms.cpu().double(), order.cpu().long()
    assert torch.equal(order, res["order"]), (label, order, res["order"])
    assert order[0].tolist().index(1) + 1 == order[0].tolist().index(3)             # the tie keeps its first-pass order
    assert order[1, 3:].tolist() == [1, 3]                                          # absent hypotheses last, in their order
    assert torch.equal(out[:, :, 1:], res["nbest_out"][:, :, 1:])
    f = torch.from_numpy(out[:, :, 0].contiguous().numpy().view(np.float32).astype(np.float64))
    worst = 0.0
    for b in range(B):
        for k in range(N):
            if not res["here"][b, k]:
                assert out[b, k, 0] == res["nbest_out"][b, k, 0] and float(terms[b, k, 1]) == 0.0      # passed through
                continue
            assert float(terms[b, k, 0]) == float(res["terms"][b, k, 0])                                # s1: the same fp32
            for s in range(S):
                got, want = float(terms[b, k, 1 + s]), float(res["terms"][b, k, 1 + s])
                tb = float(RR.term_bound(res["mags"][s][b, k], U, tiles[s]))
                print("[nbest rescore] %s (%d, %d) term %d: device %.7f float64 %.7f bound %.2e" % (label, b, k, s + 1, got, want, tb))
                assert got == want or abs(got - want) <= tb, (label, b, k, s, got, want, tb)
                worst = max(worst, 0.0 if got == want else abs(got - want) / tb)
            got, want, fb = float(f[b, k]), float(res["f"][b, k]), float(bound[b, k])
            print("[nbest rescore] %s (%d, %d) f: device %.7f float64 %.7f bound %.2e" % (label, b, k, got, want, fb))
            assert got == want or abs(got - want) <= fb, (label, b, k, got, want, fb)
            worst = max(worst, 0.0 if got == want else abs(got - want) / fb)
    k_inf = order[2].tolist().index(2)
    assert float(terms[2, k_inf, 1]) == -math.inf and float(f[2, k_inf]) == -math.inf and k_inf == N - 1
    print("[nbest rescore] %s: largest |device - float64| / bound %.3f" % (label, worst))


# ---- Decoder.forward_nbest ------------------------------------------------------------------------------------------------------
def test_forward_nbest_equals_forward():
    """the hidden rows at valid positions against Decoder.forward on the N-times replicated memory: d = 64, 2 layers, B = 3,
    N = 4, ragged ulen including 0 and 1, ragged hlens; tolerance: test_decoder_golden's 2e-5"""
    from espnet_amd.nets import modules as M
    torch.manual_seed(5)
    B, N, U, Tm, D, V = 3, 4, 6, 11, 64, 23
    dec = M.Decoder(odim=V, attention_dim=D, attention_heads=4, linear_units=96, num_blocks=2, dropout_rate=0.0,
                    positional_dropout_rate=0.0, use_output_layer=False).to(DEV).eval()
    g = torch.Generator().manual_seed(6)
    memory = torch.randn(B, Tm, D, generator=g).to(DEV)
    hlens = [11, 7, 9]
    mmask = M.make_non_pad_mask(hlens, Tm).unsqueeze(-2)
    ulen = torch.tensor([6, 0, 1, 3, 2, 6, 5, 1, 0, 4, 6, 2], dtype=torch.int32)
    ys_in = torch.randint(1, V - 1, (B, N, U), generator=g)
    ys_in[:, :, 0] = V - 1
    with torch.no_grad():
        got = dec.forward_nbest(ys_in.to(DEV), ulen.to(DEV), memory, mmask).view(B * N, U, D)
        tmask = M.subsequent_mask(U).unsqueeze(0).expand(B * N, U, U).contiguous()
        want, _ = dec(ys_in.view(B * N, U).to(DEV), tmask, memory.repeat_interleave(N, 0).contiguous(), mmask.repeat_interleave(N, 0))
    live = (torch.arange(U).view(1, U) < ulen.view(-1, 1)).to(DEV)
    assert int(live.sum()) == int(ulen.sum())
    report("forward_nbest hidden rows", got[live], want[live], 2e-5)


# ---- reference parity, decoder --------------------------------------------------------------------------------------------------
def _fixture_nbest(seqs, s1, T):
    """one utterance's hypotheses (with sos / eos) -> hyps row for RR.make_nbest"""
    return [(float(s), list(y[1:-1])) for y, s in zip(seqs, s1)]


@pytest.mark.parametrize("tag,w", [("beam_w03_r00", 0.3), ("beam_w00_r00", None)])
def test_rescorer_against_the_reference_search_decoder(tag, w):
    """the five hypotheses the reference's BeamSearch ended with for u0 - u2 at the benchmarked width, packed with s1 = sc_ctc
    (0 for the attention-only search, which has no CTC score), all three utterances in one call: the decoder term equals
    sc_decoder, f equals scores (w03), the order is the fixture's - 1e-4 relative, c2width_compare's tolerance"""
    from espnet_amd.nets.nbest_rescore import NBestRescorer
    from test_gpu_model import c2width_nbest, c2width_setup
    SW, model, g, encs = c2width_setup()
    seqs, scores, per = zip(*[c2width_nbest(g, "u%d_%s" % (u, tag)) for u in range(3)])
    T = max(len(y) for s in seqs for y in s)
    hyps = [_fixture_nbest(seqs[u], per[u]["ctc"] if w is not None else [0.0] * len(seqs[u]), T) for u in range(3)]
    nbest = RR.make_nbest(hyps, T).to(DEV)
    hs_pad = torch.nn.utils.rnn.pad_sequence(encs, batch_first=True)
    r = NBestRescorer(decoder=model.decoder, ctc_weight=w if w is not None else 0.3, sos=model.sos, eos=model.eos)
    out, terms, order = r.rescore_device(hs_pad, [e.shape[0] for e in encs], nbest)
    out, terms, order = out.cpu(), terms.cpu().double(), order.cpu().tolist()
    f = out[:, :, 0].contiguous().numpy().view(np.float32)
    for u in range(3):
        for k, j in enumerate(order[u]):
            want = per[u]["decoder"][j]
            got = float(terms[u, k, 1])
            assert abs(got - want) <= TOL * abs(want), (tag, u, k, got, want)
            if w is not None:
                assert abs(float(f[u, k]) - scores[u][j]) <= TOL * abs(scores[u][j]), (tag, u, k, float(f[u, k]), scores[u][j])
            if j != k:          # a swap: only between hypotheses the reference itself has closer than 2 TOL (c2width_compare)
                assert abs(scores[u][j] - scores[u][k]) <= 2 * TOL * max(1.0, abs(scores[u][j])), (tag, u, "order", order[u], scores[u])
        assert order[u][0] == 0 or abs(scores[u][0] - scores[u][1]) <= 2 * TOL * max(1.0, abs(scores[u][0]))
        print("[nbest rescore] c2width u%d %s: order %s, decoder terms %s" % (u, tag, order[u], [round(float(v), 4) for v in terms[u, :, 1]]))


def test_rescorer_in_bf16_mode_stays_within_the_loss_bar():
    """set_precision("bf16"): bf16 operands through the decoder and the row-statistics GEMM (no [rows, V] logits there either).
    The decoder term is a summed log-likelihood, i.e. a loss: it stays within the project's 1e-3 relative bar for bf16 losses
    (test_gpu_model) of the reference's sc_decoder, on the fp32 encoder outputs (measured on an MI355X: 8.3e-4 at worst, over
    sums of ~190 log-probabilities through two decoder layers)"""
    import espnet_amd
    from espnet_amd.nets.nbest_rescore import NBestRescorer
    from test_gpu_model import c2width_nbest, c2width_setup
    SW, model, g, encs = c2width_setup()
    seqs, scores, per = zip(*[c2width_nbest(g, "u%d_beam_w03_r00" % u) for u in range(3)])
    T = max(len(y) for s in seqs for y in s)
    nbest = RR.make_nbest([_fixture_nbest(seqs[u], per[u]["ctc"], T) for u in range(3)], T).to(DEV)
    hs_pad = torch.nn.utils.rnn.pad_sequence(encs, batch_first=True)
    espnet_amd.set_precision("bf16")
    r = NBestRescorer(decoder=model.decoder, ctc_weight=0.3, sos=model.sos, eos=model.eos)
    out, terms, order = r.rescore_device(hs_pad, [e.shape[0] for e in encs], nbest)
    terms, order = terms.cpu().double(), order.cpu().tolist()
    worst = 0.0
    for u in range(3):
        for k, j in enumerate(order[u]):
            want = per[u]["decoder"][j]
            worst = max(worst, abs(float(terms[u, k, 1]) - want) / abs(want))
    print("[nbest rescore] bf16 mode, c2width decoder terms: largest relative difference %.3e" % worst)
    assert worst <= 1e-3


# ---- reference parity, LM ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,lm", [("beam_tlm", "tlm"), ("beam_rlm", "rlm")])
def test_rescorer_against_the_reference_search_lm(tag, lm):
    """decoder + LM against the reference's fused search (decode_fusion.npz, weights ctc 0.3 / decoder 0.7 / lm 0.6 / length
    bonus 0.1): s1 = the float64 CTC log-likelihood of each yseq from the model's own CTC log-softmax; f plus the search's
    length bonus 0.1 * (len(yseq) - 1) equals the fixture's scores to 1e-4 relative.  That this recomposition holds for the
    reference alone is the CPU test test_rescore_restatement.test_lm_recomposition_holds_for_the_reference; as explained
    there, the reference's search ran all six hypotheses into maxlen: beam_tlm's three and beam_rlm's first are scored without
    the unscored second <eos> the search appended, beam_rlm's other two (no scored <eos> at all) are left out."""
    from espnet_amd.nets.nbest_rescore import NBestRescorer
    from test_gpu_model import _fusion_models, _nbest_from
    p, model, lms = _fusion_models()
    with torch.no_grad():
        enc, _ = model.encode(p["speech"].unsqueeze(0).to(DEV), torch.tensor([p["speech"].shape[0]]))
        logp = model.ctc.log_softmax(enc)[0].cpu()
    kept = RR.scored_hypotheses(*_nbest_from(p, tag), model.eos, enc.shape[1])
    assert len(kept) == {"beam_tlm": 3, "beam_rlm": 1}[tag]
    want, scores = [y for y, _ in kept], [s for _, s in kept]
    s1 = [RR.ctc_loglik(logp, y[1:-1]) for y in want]
    T = max(len(y) for y in want)
    nbest = RR.make_nbest([_fixture_nbest(want, s1, T)], T).to(DEV)
    r = NBestRescorer(decoder=model.decoder, lm=lms[lm], ctc_weight=0.3, lm_weight=0.6, sos=model.sos, eos=model.eos)
    hyps = r.rescore(enc, [enc.shape[1]], nbest)[0]
    assert len(hyps) == len(want)
    for h in hyps:
        j = want.index(h["yseq"])
        got = h["score"] + 0.1 * (len(h["yseq"]) - 1)
        print("[nbest rescore] fusion %s: %s f + bonus %.5f ref %.5f" % (tag, h["scores"], got, scores[j]))
        assert abs(got - scores[j]) <= TOL * abs(scores[j]), (tag, j, got, scores[j])
        assert set(h["scores"]) == {"ctc", "decoder", "lm"}
        assert abs(0.3 * h["scores"]["ctc"] + 0.7 * h["scores"]["decoder"] + 0.6 * h["scores"]["lm"] - h["score"]) <= 1e-5 * abs(h["score"])


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _e2e_model(mtlalpha, seed):
    """the e2e_conformer.npz-size model (test_gpu_model.CASES[0]) with seeded random weights"""
    from espnet_amd.nets.e2e_asr_conformer import E2E
    torch.manual_seed(seed)
    ns = argparse.Namespace(adim=64, aheads=4, elayers=2, eunits=128, dlayers=1, dunits=128, mtlalpha=mtlalpha, lsm_weight=0.1,
                            dropout_rate=0.0, transformer_length_normalized_loss=False,
                            transformer_encoder_pos_enc_layer_type="rel_pos", transformer_encoder_selfattn_layer_type="rel_selfattn",
                            macaron_style=True, use_cnn_module=True, cnn_module_kernel=15)
    return E2E(20, 50, ns).to(DEV).eval()


def _second_pass_float64(nbest, sos, eos, logits_of):
    """the restatement on full logits: logits_of(ys_in [R, U]) -> [R, U, V] from the model's ordinary forward; log_softmax and
    the sums in float64 -> (terms [B, N] float64, magnitude [B, N] = sum of |log p| added)"""
    B, N, W = nbest.shape
    U = int(nbest[:, :, 1].max()) + 1
    ys_in, col, ulen = RR.pack(nbest, U, sos, eos)
    lp = torch.log_softmax(logits_of(ys_in).double().cpu(), dim=-1).view(B * N * U, -1)
    live = col >= 0
    tok = torch.gather(lp, 1, col.long().clamp(min=0).view(-1, 1)).view(-1)
    tok = torch.where(live, tok, torch.zeros_like(tok)).view(B * N, U)
    return tok.sum(1).view(B, N), tok.abs().sum(1).view(B, N)


def _expected_nbest(nbest, terms, weights, w0, tol):
    """f, ranking and the gap precondition (10 x tol * max(1, |f|)) of the restatement -> per utterance [(f, yseq body)]"""
    worst = math.inf
    B, N, W = nbest.shape
    here = nbest[:, :, 1] >= 0
    s1 = torch.from_numpy(nbest[:, :, 0].contiguous().numpy().view(np.float32).astype(np.float64))
    f = RR.combine(s1, terms, weights, w0)
    order = RR.rank(f, here)
    res = []
    for b in range(B):
        rows = [(float(f[b, n]), nbest[b, n, 2:2 + int(nbest[b, n, 1])].tolist()) for n in order[b].tolist() if here[b, n]]
        for (fa, _), (fb, _) in zip(rows, rows[1:]):
            worst = min(worst, (fa - fb) / max(1.0, abs(fa)))
        res.append(rows)
    print("[nbest rescore] smallest gap of the restatement's f / max(1, |f|): %.3e (tolerance %.1e)" % (worst, tol))
    assert worst > 10 * tol, "smallest relative gap %.3e below 10 x tolerance %.1e: choose another seed" % (worst, tol)
    return res


def _first_pass(model, xs, beam):
    from espnet_amd.nets.ctc_prefix_beam import CTCPrefixBeamSearch
    encs = [model.encode(x) for x in xs]
    hs_pad = torch.nn.utils.rnn.pad_sequence(encs, batch_first=True)
    hlens = [e.shape[0] for e in encs]
    with torch.no_grad():
        nbest = CTCPrefixBeamSearch(beam, nbest=beam).search_device(model.ctc.log_softmax(hs_pad.contiguous()), hlens)
    return hs_pad, hlens, nbest.cpu()


def _check_hyps(got, want, sos, eos, keep, label):
    assert len(got) == min(keep, len(want)), (label, len(got), len(want))
    for h, (f, body) in zip(got, want):
        print("[nbest rescore] %s: device %.6f float64 %.6f rel %.2e" % (label, h["score"], f, abs(h["score"] - f) / max(1.0, abs(f))))
        assert h["yseq"] == [sos] + body + [eos], (label, h["yseq"], body)
        assert abs(h["score"] - f) <= E2E_TOL * max(1.0, abs(f)), (label, h["score"], f)


# chosen on an MI355X among seeds 21 .. 35: smallest relative gap of the restatement's f 1.1e-2 / 8.7e-4, against 10 x E2E_TOL = 8.6e-6
E2E_SEED, E2E_LM_SEED = 29, 27


def test_recognize_rescore_with_the_decoder():
    """recognize / recognize_batch(ctc_search="rescore") on the e2e_conformer.npz-size model, B = 3 ragged, beam 5: the batch
    gives every utterance the n-best it gets alone, and both equal "prefix beam search, then the restatement on
    Decoder.forward + log_softmax in float64" (scores to E2E_TOL * max(1, |f|); the restatement's gaps are asserted to
    exceed 10 x that first)"""
    from espnet_amd.nets import modules as M
    model = _e2e_model(0.3, E2E_SEED)
    g = torch.Generator().manual_seed(E2E_SEED)
    xs = [torch.randn(n, 20, generator=g) for n in (83, 60, 47)]
    ra = argparse.Namespace(ctc_weight=0.3, beam_size=5, nbest=3, penalty=0.0, ctc_search="rescore")
    hs_pad, hlens, nbest = _first_pass(model, xs, 5)
    B, N, _ = nbest.shape

    def logits_of(ys_in):
        U = ys_in.shape[1]
        tmask = M.subsequent_mask(U).unsqueeze(0).expand(B * N, U, U).contiguous()
        mmask = M.make_non_pad_mask(hlens, hs_pad.shape[1]).unsqueeze(-2).repeat_interleave(N, 0)
        with torch.no_grad():
            return model.decoder(ys_in.to(DEV), tmask, hs_pad.repeat_interleave(N, 0).contiguous(), mmask)[0]

    att, _ = _second_pass_float64(nbest, model.sos, model.eos, logits_of)
    want = _expected_nbest(nbest, [att], [0.7], 0.3, E2E_TOL)
    batch = model.recognize_batch(xs, ra)
    assert len(batch) == 3
    for b, x in enumerate(xs):
        _check_hyps(batch[b], want[b], model.sos, model.eos, 3, "batch %d" % b)
        alone = model.recognize(x, ra)
        _check_hyps(alone, want[b], model.sos, model.eos, 3, "alone %d" % b)
        assert [h["yseq"] for h in alone] == [h["yseq"] for h in batch[b]]
        assert set(alone[0]["scores"]) == {"ctc", "decoder"}
    print("[nbest rescore] e2e decoder: best %s" % [round(h[0]["score"], 4) for h in batch])


def test_recognize_rescore_with_an_lm_on_a_ctc_only_model():
    """mtlalpha = 1.0: f = s1 + lm_weight * lm with a SequentialRNNLM (2-layer LSTM), against the LM's own forward in float64"""
    from espnet_amd.espnet2 import SequentialRNNLM
    model = _e2e_model(1.0, E2E_LM_SEED)
    torch.manual_seed(E2E_LM_SEED)
    lm = SequentialRNNLM(50, unit=32, nlayers=2, rnn_type="lstm").to(DEV).eval()
    g = torch.Generator().manual_seed(E2E_LM_SEED)
    xs = [torch.randn(n, 20, generator=g) for n in (83, 60, 47)]
    ra = argparse.Namespace(ctc_weight=0.5, beam_size=5, nbest=5, penalty=0.0, lm_weight=0.8, ctc_search="rescore")
    hs_pad, hlens, nbest = _first_pass(model, xs, 5)

    def logits_of(ys_in):
        with torch.no_grad():
            return lm(ys_in.to(DEV), None)[0]

    term, _ = _second_pass_float64(nbest, model.sos, model.eos, logits_of)
    want = _expected_nbest(nbest, [term], [f32(0.8)], 1.0, E2E_TOL)
    batch = model.recognize_batch(xs, ra, rnnlm=lm)
    for b, x in enumerate(xs):
        _check_hyps(batch[b], want[b], model.sos, model.eos, 5, "batch %d" % b)
        _check_hyps(model.recognize(x, ra, rnnlm=lm), want[b], model.sos, model.eos, 5, "alone %d" % b)
        assert set(batch[b][0]["scores"]) == {"ctc", "lm"}
    print("[nbest rescore] e2e ctc-only + lm: best %s" % [round(h[0]["score"], 4) for h in batch])


def test_lm_whose_hidden_width_is_no_multiple_of_eight():
    """a 30-unit GRU LM (the reference's default LSTM LM has 650 units): the row-statistics GEMM gets zero-padded operands and
    the LM term still is the LM's own forward in float64 (terms compared in first-pass order, so no gap is needed)"""
    from espnet_amd.espnet2 import SequentialRNNLM
    from espnet_amd.nets.nbest_rescore import NBestRescorer
    V, T = 50, 9
    torch.manual_seed(31)
    lm = SequentialRNNLM(V, unit=30, nlayers=1, rnn_type="gru").to(DEV).eval()
    g = torch.Generator().manual_seed(32)
    hyps = [[(float(torch.randn((), generator=g)), torch.randint(1, V - 1, (L,), generator=g).tolist()) for L in ls] for ls in ([9, 2, 5], [0, 7, 4])]
    nbest = RR.make_nbest(hyps, T)

    def logits_of(ys_in):
        with torch.no_grad():
            return lm(ys_in.to(DEV), None)[0]

    want, _ = _second_pass_float64(nbest, V - 1, V - 1, logits_of)
    out, terms, order = NBestRescorer(lm=lm, lm_weight=0.5, sos=V - 1, eos=V - 1).rescore_device(None, None, nbest.to(DEV))
    terms, order = terms.cpu().double(), order.cpu().long()
    for b in range(2):
        for k in range(3):
            got, ref = float(terms[b, k, 1]), float(want[b, int(order[b, k])])
            print("[nbest rescore] 30-unit LM (%d, %d): device %.6f float64 %.6f" % (b, k, got, ref))
            assert abs(got - ref) <= E2E_TOL * max(1.0, abs(ref)), (b, k, got, ref)


def test_speech2text_rescore():
    """Speech2Text(ctc_search="rescore") returns the best hypothesis of "first pass, then the restatement on the decoder's
    ordinary forward", as Hypothesis objects whose scores carry the terms"""
    from espnet_amd.espnet2 import CTC, ConformerEncoder, ESPnetASRModel, Speech2Text, TransformerDecoder
    from espnet_amd.nets import modules as M
    from espnet_amd.nets.beam_search import Hypothesis
    from espnet_amd.nets.ctc_prefix_beam import CTCPrefixBeamSearch
    torch.manual_seed(2)
    enc = ConformerEncoder(20, output_size=64, attention_heads=4, linear_units=96, num_blocks=2, dropout_rate=0.0,
                           positional_dropout_rate=0.0, attention_dropout_rate=0.0, macaron_style=True, cnn_module_kernel=7)
    dec = TransformerDecoder(30, 64, attention_heads=4, linear_units=96, num_blocks=1, dropout_rate=0.0, positional_dropout_rate=0.0)
    model = ESPnetASRModel(vocab_size=30, encoder=enc, decoder=dec, ctc=CTC(30, 64, ctc_type="builtin"), ctc_weight=0.3)
    s2t = Speech2Text(model, device=DEV, beam_size=5, ctc_weight=0.3, nbest=2, ctc_search="rescore")
    speech = torch.randn(90, 20, generator=torch.Generator().manual_seed(3))
    res = s2t(speech.numpy())
    with torch.no_grad():
        enc_out, _ = model.encode(speech.unsqueeze(0).to(DEV), torch.full([1], 90, dtype=torch.long))
        nbest = CTCPrefixBeamSearch(5, nbest=5).search_device(model.ctc.log_softmax(enc_out), [enc_out.shape[1]]).cpu()
    N = nbest.shape[1]

    def logits_of(ys_in):
        U = ys_in.shape[1]
        tmask = M.subsequent_mask(U).unsqueeze(0).expand(N, U, U).contiguous()
        with torch.no_grad():
            return dec._dec[0](ys_in.to(DEV), tmask, enc_out.repeat_interleave(N, 0).contiguous(), None)[0]

    att, _ = _second_pass_float64(nbest, model.sos, model.eos, logits_of)
    want = _expected_nbest(nbest, [att], [0.7], 0.3, E2E_TOL)[0]
    assert len(res) == 2
    for (text, token, token_int, hyp), (f, body) in zip(res, want):
        assert isinstance(hyp, Hypothesis) and hyp.yseq.tolist() == [model.sos] + body + [model.eos]
        assert abs(float(hyp.score) - f) <= E2E_TOL * max(1.0, abs(f)) and set(hyp.scores) == {"ctc", "decoder"}
        assert token_int == [t for t in body if t != 0]


# ---- host reads and memory ---------------------------------------------------------------------------------------------------------
def test_rescore_mode_makes_at_most_three_host_reads(monkeypatch):
    """counted as test_transducer_search_one_host_read_per_pass counts them: the first pass's one read (here none: its n-best
    stays on the device) plus the longest length and the result"""
    model = _e2e_model(0.3, E2E_SEED)
    g = torch.Generator().manual_seed(E2E_SEED)
    xs = [torch.randn(n, 20, generator=g) for n in (83, 60, 47)]
    ra = argparse.Namespace(ctc_weight=0.3, beam_size=5, nbest=3, penalty=0.0, ctc_search="rescore")
    model.recognize_batch(xs, ra)
    reads = [0]
    for meth in ("tolist", "item", "cpu", "numpy"):
        orig = getattr(torch.Tensor, meth)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                reads[0] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, meth, counted)
    got = model.recognize_batch(xs, ra)
    monkeypatch.undo()
    print("[nbest rescore] recognize_batch(ctc_search='rescore'): %d host reads" % reads[0])
    assert len(got) == 3 and 1 <= reads[0] <= 3


def test_no_rows_by_vocabulary_buffer():
    """d = 64, V = 20000, B = 4, N = 8, U = 33: the pass allocates less than ONE [rows, V] fp32 matrix (84 MB) at its peak"""
    from espnet_amd.nets import modules as M
    from espnet_amd.nets.nbest_rescore import NBestRescorer
    B, N, T, V, D = 4, 8, 40, 20000, 64
    torch.manual_seed(7)
    dec = M.Decoder(odim=V, attention_dim=D, attention_heads=4, linear_units=96, num_blocks=1, dropout_rate=0.0,
                    positional_dropout_rate=0.0).to(DEV).eval()
    g = torch.Generator().manual_seed(8)
    hyps = [[(float(torch.randn((), generator=g)), torch.randint(1, V - 1, (32 if (b, n) == (0, 0) else int(torch.randint(0, 33, (), generator=g)),),
                                                                  generator=g).tolist()) for n in range(N)] for b in range(B)]
    nbest = RR.make_nbest(hyps, T).to(DEV)
    memory = torch.randn(B, 20, D, generator=g).to(DEV)
    r = NBestRescorer(decoder=dec, ctc_weight=0.3, sos=V - 1, eos=V - 1)
    r.rescore_device(memory, [20, 17, 20, 9], nbest)                   # warm-up: positional table, library handles
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, terms, order = r.rescore_device(memory, [20, 17, 20, 9], nbest)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    rows = B * N * 33
    print("[nbest rescore] peak allocation of the pass: %.2f MB, one [rows, V] fp32 matrix: %.2f MB" % (peak / 1e6, rows * V * 4 / 1e6))
    assert peak < rows * V * 4
    assert torch.isfinite(terms).all()
