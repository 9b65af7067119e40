"""Batched greedy transducer decoding on the GPU: the fused joint + argmax kernels (csrc/rnnt_greedy.hip) and
BeamSearchTransducer.greedy_batch / E2E.recognize_batch against
  * tests/rnnt_greedy_restatement.py - float64, pinned to the reference by tests/test_rnnt_greedy_restatement.py,
  * the per-utterance greedy search of the same package, and
  * the greedy hypotheses the reference recorded in tests/golden/transducer_*.npz.
Tokens, live flags and appended sequences are compared exactly; that is meaningful where float32 cannot flip a decision, so
every compared decision must have a float64 top-2 logit gap >= 1e-4 (the float32 error of these logits is of order 1e-6).
This precondition is ASSERTED: the seeds below were chosen on the CPU (each case takes the first seed of its own sequence whose
float64 run meets the precondition and has both blank and emit decisions; the choice never looks at a GPU result).
Scores: 1e-4 * max(1, |reference|), the bound of the existing transducer decoding tests."""
import numpy as np
import pytest
import torch

from conftest import load_golden, split_golden
from rnnt_greedy_restatement import frame_decision, greedy_batch64, seeded_weights, weights_from_state_dict

DEV = "cuda"
GAP = 1e-4
ACTS = ("tanh", "relu", "swish")
T_K = 5                                   # frames of a kernel case


@pytest.fixture(autouse=True)
def _fp32():
    import espnet_amd
    espnet_amd.set_precision("fp32")
    yield
    espnet_amd.set_precision("fp32")


def _blank_bias(V):
    """bias on b_out[blank] that puts blank near the largest of the V - 1 other logits (standard deviation about 1.4)"""
    return {2: 0.0, 6: 2.0}.get(V, 4.0)


# ---- 1. kernels vs float64 ---------------------------------------------------------------------------------------------
def kernel_case(B, V, J, act, seed):
    """seeded operands of T_K frames: enc_proj [B, T, J], one d [B, J] per frame, W_out, b_out (blank biased), hlens"""
    r = np.random.default_rng(seed)
    f = lambda *s, scale=1.0: (r.standard_normal(s) * scale).astype(np.float32)      # noqa: E731
    c = dict(enc=f(B, T_K, J), d=f(T_K, B, J, scale=0.7), w=f(V, J, scale=2.0 / np.sqrt(J)), b=f(V, scale=0.5),
             hlens=r.integers(1, T_K + 1, B).astype(np.int32))
    c["b"][0] += np.float32(_blank_bias(V))
    return c


def kernel_case_reference(c, act):
    """float64 decisions of every frame: [(token, logp, gap, on)] with on = t < hlens"""
    return [frame_decision(c["enc"][:, t], c["d"][t], c["w"], c["b"], act)[:3] + (t < c["hlens"],) for t in range(T_K)]


def kernel_case_ok(c, act):
    ref = kernel_case_reference(c, act)
    gap = min(float(g[on].min()) for _tok, _lp, g, on in ref if on.any())
    n_blank = sum(int((on & (tok == 0)).sum()) for tok, _lp, _g, on in ref)
    n_emit = sum(int((on & (tok != 0)).sum()) for tok, _lp, _g, on in ref)
    return gap >= GAP and (n_blank > 0 and n_emit > 0 or c["enc"].shape[0] == 1)


def kernel_seed(B, V, J, act):
    """the case's seed: the first of its sequence whose float64 run meets the precondition (CPU only)"""
    base = 1000 * B + 10 * V + J + 100000 * ACTS.index(act)
    for i in range(64):
        if kernel_case_ok(kernel_case(B, V, J, act, base + 7919 * i), act):
            return base + 7919 * i
    raise AssertionError("no seed meets the gap precondition")


class _Dev:
    """device buffers of one kernel case"""

    def __init__(self, c, score0=0.0):
        from espnet_amd import ops
        B, V = c["enc"].shape[0], c["w"].shape[0]
        self.B, self.V, self.ycap = B, V, T_K + 1
        self.enc, self.w, self.b = (torch.from_numpy(c[k]).to(DEV) for k in ("enc", "w", "b"))
        self.d = [torch.from_numpy(c["d"][t]).to(DEV) for t in range(T_K)]
        self.hlens = torch.from_numpy(c["hlens"]).to(DEV)
        self.part = ops.rnnt_greedy_part(B, V, DEV)
        self.yseq = torch.zeros(B, self.ycap, dtype=torch.int32, device=DEV)
        self.ylen = torch.ones(B, dtype=torch.int32, device=DEV)
        self.score = torch.full((B,), score0, dtype=torch.float32, device=DEV)
        self.tok = torch.full((B,), -7, dtype=torch.int64, device=DEV)
        self.live = torch.full((B,), 9, dtype=torch.uint8, device=DEV)

    def frame(self, t, act, t_arg=None, t_dev=None, hlens=True):
        from espnet_amd import ops
        from espnet_amd.nets.transducer.joint_network import _ACTS
        t_arg = t if t_arg is None else t_arg
        ops.rnnt_greedy_joint(self.enc, self.d[t], self.w, self.b, self.part, _ACTS[act], t_arg, t_dev)
        ops.rnnt_greedy_pick(self.part, self.hlens if hlens else None, self.yseq, self.ylen, self.score, self.tok, self.live,
                             T_K, self.V, 0, t_arg, t_dev)

    def host(self):
        return (self.yseq.cpu().numpy().copy(), self.ylen.cpu().numpy().copy(), self.score.cpu().numpy().astype(np.float64),
                self.tok.cpu().numpy().copy(), self.live.cpu().numpy().copy())


def _check_frames(c, act, dev, run_frame, score0=0.0):
    """steps the device through the T_K frames and compares every frame's decision with float64"""
    B = c["enc"].shape[0]
    ref = kernel_case_reference(c, act)
    yseq = np.zeros((B, T_K + 1), np.int64)
    ylen = np.ones(B, np.int64)
    score = np.full(B, score0, np.float64)
    worst = 0.0
    for t, (tok, logp, gap, on) in enumerate(ref):
        assert not on.any() or gap[on].min() >= GAP, ("precondition: float64 top-2 gap", t, gap[on].min())
        live = on & (tok != 0)
        for b in np.nonzero(live)[0]:
            yseq[b, ylen[b]] = tok[b]
            ylen[b] += 1
            score[b] += logp[b]
        run_frame(t)
        g_yseq, g_ylen, g_score, g_tok, g_live = dev.host()
        assert np.array_equal(g_live, live.astype(np.uint8)), (t, g_live, live)
        assert np.array_equal(g_tok, np.where(live, tok, 0)), (t, g_tok, tok)
        assert np.array_equal(g_ylen, ylen) and np.array_equal(g_yseq, yseq), t
        err = np.abs(g_score - score) / np.maximum(1.0, np.abs(score))
        worst = max(worst, float(err.max()))
        assert err.max() <= 1e-4, (t, g_score, score)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("J", [7, 52, 64])
@pytest.mark.parametrize("V", [2, 6, 256, 257])
@pytest.mark.parametrize("B", [1, 3, 17, 33])
def test_joint_and_pick_kernels_vs_float64(B, V, J):
    """one joint + pick call per frame against the restatement's decision for that frame from the same d: token, live flag and
    the appended yseq / ylen equal, score within 1e-4 * max(1, |ref|); every activation; random hlens, blank biased"""
    for act in ACTS:
        c = kernel_case(B, V, J, act, kernel_seed(B, V, J, act))
        dev = _Dev(c)
        worst = _check_frames(c, act, dev, lambda t: dev.frame(t, act))
        print("[parity] rnnt greedy kernels B=%d V=%d J=%d %s: decisions equal, score rel err %.2e" % (B, V, J, act, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("J", [7, 52])
@pytest.mark.parametrize("V,pair", [(257, (3, 4)), (257, (63, 64)), (257, (255, 256)), (257, (1, 256)), (256, (1, 255)),
                                    (6, (3, 4)), (6, (1, 5))])
def test_equal_logits_lowest_id_wins(V, pair, J):
    """two tokens with identical rows of W_out and entries of b_out are the row maximum: the lower id is emitted - inside a
    tile, across a tile boundary (63 | 64, 255 | 256) and against the ragged last tile (1 | V - 1)"""
    lo, hi = pair
    B = 17
    c = kernel_case(B, V, J, "tanh", 4242 + V + J)
    c["w"][hi] = c["w"][lo]
    c["b"][lo] = c["b"][hi] = np.float32(60.0)              # |other logits| < 2 sqrt(J) + a few units: these two are the maximum
    c["hlens"][:] = T_K
    tok, _lp, gap, _ = frame_decision(c["enc"][:, 0], c["d"][0], c["w"], c["b"], "tanh")
    assert (tok == lo).all() and (gap == 0).all()           # float64 sees the tie too, and numpy's argmax takes the first
    dev = _Dev(c)
    dev.frame(0, "tanh")
    yseq, ylen, _score, g_tok, live = dev.host()
    assert (g_tok == lo).all() and (live == 1).all() and (ylen == 2).all() and (yseq[:, 1] == lo).all()


@pytest.mark.gpu
def test_blank_best_and_frames_past_the_length_append_nothing():
    B, V, J = 17, 257, 52
    c = kernel_case(B, V, J, "tanh", 77)
    c["b"][0] += np.float32(60.0)                            # blank best on every row
    c["hlens"][:] = T_K
    dev = _Dev(c, score0=1.5)
    dev.frame(0, "tanh")
    yseq, ylen, score, tok, live = dev.host()
    assert (tok == 0).all() and (live == 0).all() and (ylen == 1).all() and (yseq == 0).all() and (score == 1.5).all()
    c = kernel_case(B, V, J, "tanh", 78)
    c["b"][5] += np.float32(60.0)                            # a non-blank maximum, on frames at and past every row's length
    c["hlens"][:] = np.arange(B) % 3                         # 0, 1, 2
    dev = _Dev(c, score0=1.5)
    for t in (2, 3, 4):
        dev.frame(t, "tanh")
        yseq, ylen, score, tok, live = dev.host()
        assert (tok == 0).all() and (live == 0).all() and (ylen == 1).all() and (yseq == 0).all() and (score == 1.5).all()
    dev.frame(1, "tanh")                                     # ... and the rows of length 2 do emit on frame 1
    yseq, ylen, score, tok, live = dev.host()
    want = (c["hlens"] == 2)
    assert np.array_equal(live, want.astype(np.uint8)) and np.array_equal(tok, np.where(want, 5, 0))
    assert np.array_equal(ylen, 1 + want) and np.array_equal(yseq[:, 1], np.where(want, 5, 0)) and (score[~want] == 1.5).all()
    dev2 = _Dev(c)                                           # hlens = NULL: every row runs all T frames
    dev2.frame(4, "tanh", hlens=False)
    assert (dev2.host()[4] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("B,V,J", [(3, 6, 7), (33, 257, 52)])
def test_frame_counter_on_the_device(B, V, J):
    """t = 0 with the counter on the device: the same results as the host-side frame index, and the counter advances by one per
    pick"""
    act = "tanh"
    c = kernel_case(B, V, J, act, kernel_seed(B, V, J, act))
    dev = _Dev(c)
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)

    def run(t):
        assert int(t_dev.cpu()[0]) == t
        dev.frame(t, act, t_arg=0, t_dev=t_dev)
    _check_frames(c, act, dev, run)
    assert int(t_dev.cpu()[0]) == T_K


# ---- 2. search vs float64 ----------------------------------------------------------------------------------------------
T_S, E_S, D_S = 12, 6, 8
SEARCH_CASES = [(dtype, L, H, J, V, B) for dtype in ("lstm", "gru") for L in (1, 2) for H in (12, 64) for (J, V) in ((7, 6), (52, 257))
                for B in (3, 33)]


def search_case(dtype, L, H, J, V, B, seed):
    sd = seeded_weights(seed, dtype, L, H, E_S, J, V, D_S, _blank_bias(V))
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((B, T_S, D_S)).astype(np.float32)
    hlens = r.integers(T_S // 2, T_S + 1, B)
    hlens[0] = T_S
    return sd, hs, hlens


def search_case_ok(ref):
    n = int(ref["n_blank"].sum() + ref["n_emit"].sum())
    return ref["min_gap"] >= GAP and 4 * int(ref["n_blank"].sum()) >= n and 4 * int(ref["n_emit"].sum()) >= n


def search_seed(dtype, L, H, J, V, B):
    base = 31 * H + 7 * J + V + 1000 * L + 100000 * (dtype == "gru") + 17 * B
    for i in range(64):
        sd, hs, hlens = search_case(dtype, L, H, J, V, B, base + 104729 * i)
        if search_case_ok(greedy_batch64(weights_from_state_dict(sd), hs, hlens)):
            return base + 104729 * i
    raise AssertionError("no seed meets the preconditions")


def _decoder(sd, dtype, L, H, E, J, V, D_enc, act="tanh"):
    from espnet_amd.nets.transducer.rnn_decoder import DecoderRNNT
    dec = DecoderRNNT(D_enc, V, dtype, L, H, 0, E, J, act)
    dec.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in sd.items()})
    return dec.to(DEV).eval()


def _same_hyps(got, want_yseq, want_score, what):
    assert len(got) == len(want_yseq), what
    worst = 0.0
    for b, (h, y, s) in enumerate(zip(got, want_yseq, want_score)):
        assert list(h.yseq) == [int(v) for v in y], (what, b, h.yseq, y)
        err = abs(h.score - float(s)) / max(1.0, abs(float(s)))
        worst = max(worst, err)
        assert err <= 1e-4, (what, b, h.score, s)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,L,H,J,V,B", SEARCH_CASES)
def test_greedy_batch_vs_float64(dtype, L, H, J, V, B):
    """greedy_batch on a seeded DecoderRNNT (H = 12: GEMM + cell kernel, H = 64: the one-launch LSTM step) against the restatement:
    tokens equal, scores within 1e-4 relative; blank and emit each make up >= 25 % of the live decisions; gap precondition"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    sd, hs, hlens = search_case(dtype, L, H, J, V, B, search_seed(dtype, L, H, J, V, B))
    ref = greedy_batch64(weights_from_state_dict(sd), hs, hlens)
    n = int(ref["n_blank"].sum() + ref["n_emit"].sum())
    assert ref["min_gap"] >= GAP, ("precondition: float64 top-2 gap", ref["min_gap"])
    assert 4 * int(ref["n_blank"].sum()) >= n and 4 * int(ref["n_emit"].sum()) >= n, (ref["n_blank"].sum(), ref["n_emit"].sum())
    bs = BeamSearchTransducer(decoder=_decoder(sd, dtype, L, H, E_S, J, V, D_S), beam_size=1)
    got = bs.greedy_batch(torch.from_numpy(hs).to(DEV), [int(v) for v in hlens])
    worst = _same_hyps(got, ref["yseq"], ref["score"], "greedy_batch vs float64")
    assert all(h.yseq[0] == 0 for h in got)
    print("[parity] greedy_batch %s x%d H=%d J=%d V=%d B=%d: %d blank / %d emit decisions equal, min gap %.1e, score rel err %.2e"
          % (dtype, L, H, J, V, B, ref["n_blank"].sum(), ref["n_emit"].sum(), ref["min_gap"], worst))


@pytest.mark.gpu
def test_greedy_batch_in_chunks_of_64_rows():
    """more rows than one frame loop takes: chunks, the same hypotheses, still one host read (test below counts it)"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    dtype, L, H, J, V, B = "lstm", 1, 64, 52, 257, 33
    sd, hs, hlens = search_case(dtype, L, H, J, V, B, search_seed(dtype, L, H, J, V, B))
    hs3, hl3 = np.concatenate([hs, hs[::-1], hs]), np.concatenate([hlens, hlens[::-1], hlens])          # 99 rows: 64 + 35
    ref = greedy_batch64(weights_from_state_dict(sd), hs, hlens)
    bs = BeamSearchTransducer(decoder=_decoder(sd, dtype, L, H, E_S, J, V, D_S), beam_size=1)
    got = bs.greedy_batch(torch.from_numpy(hs3).to(DEV), torch.from_numpy(hl3).to(DEV))
    _same_hyps(got[:B], ref["yseq"], ref["score"], "chunk 0")
    _same_hyps(got[B:2 * B], ref["yseq"][::-1], ref["score"][::-1], "across the chunk boundary")
    _same_hyps(got[2 * B:], ref["yseq"], ref["score"], "chunk 1")


# ---- 3. search vs the per-utterance path and the reference's record ----------------------------------------------------
def _golden_model(name):
    from test_gpu_model import load_sd
    from test_gpu_rnn import _trn_case_args
    from espnet_amd.nets.e2e_asr_transducer import E2E
    p, sd, _ = split_golden(load_golden(name))
    m = load_sd(E2E(12, 6, _trn_case_args(name)), sd)
    m.train()
    m(p["xs"].to(DEV), p["ilens"], p["ys"].to(DEV))      # as in the fixture: BatchNorm running stats see one training batch
    m.eval()
    with torch.no_grad():
        m(p["xs"].to(DEV), p["ilens"], p["ys"].to(DEV))  # m.hs_pad: the padded encoder states of the batch in eval mode
    return p, m


def _valid_lengths(m, p):
    from espnet_amd.nets.modules import subsampled_lengths
    il = [int(v) for v in p["ilens"]]
    if "transformer" in m.etype:
        return [int(v) for v in subsampled_lengths(il, int(p["xs"].shape[1]))]
    with torch.no_grad():
        _h, hl, _ = m.enc(p["xs"].to(DEV), il)
    return [int(v) for v in (hl.tolist() if torch.is_tensor(hl) else hl)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["transducer_rnn.npz", "transducer_gru.npz", "transducer_conformer.npz"])
def test_greedy_batch_vs_per_utterance_search_and_reference(name):
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    p, m = _golden_model(name)
    search = BeamSearchTransducer(decoder=m.dec, beam_size=1)
    hs_pad = m.hs_pad.detach()
    hlens = _valid_lengths(m, p)
    assert max(hlens) == hs_pad.shape[1] and min(hlens) < max(hlens)
    one = [search(hs_pad[b, : hlens[b]]) for b in range(len(hlens))]
    _same_hyps(search.greedy_batch(hs_pad, hlens), [h.yseq for h in one], [h.score for h in one], "ragged")
    _same_hyps(search.greedy_batch(hs_pad, torch.tensor(hlens).to(DEV)), [h.yseq for h in one], [h.score for h in one], "tensor hlens")
    whole = [search(hs_pad[b]) for b in range(len(hlens))]
    _same_hyps(search.greedy_batch(hs_pad), [h.yseq for h in whole], [h.score for h in whole], "hlens=None: whole padded rows")
    xs = [p["xs"][b, : int(p["ilens"][b])].numpy() for b in range(3)]
    nb = m.recognize_batch(xs, search)
    assert len(nb) == 3
    n = int(p["dec_greedy_lens"][0])
    want_s = float(p["dec_greedy_scores"][0])
    assert nb[0]["yseq"] == [int(v) for v in p["dec_greedy_yseq"][:n]]           # the reference's record: bit exact
    assert abs(nb[0]["score"] - want_s) <= 1e-4 * max(1.0, abs(want_s)), (nb[0]["score"], want_s)
    # beam_size > 1: the configured search per utterance on its valid frames, in recognize's format
    beam = BeamSearchTransducer(decoder=m.dec, beam_size=2)
    nb2 = m.recognize_batch(xs, beam)
    assert len(nb2) == 3 and all(isinstance(r, list) and r and "yseq" in r[0] for r in nb2)
    assert nb2[0][0]["yseq"] == m.recognize(xs[0], beam)[0]["yseq"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["transducer_att.npz", "transducer_tt.npz"])
def test_other_prediction_networks_loop_over_the_per_utterance_search(name):
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    p, m = _golden_model(name)
    search = BeamSearchTransducer(decoder=m.decoder if hasattr(m, "decoder") else m.dec, beam_size=1)
    hs_pad = m.hs_pad.detach()
    hlens = _valid_lengths(m, p)
    one = [search(hs_pad[b, : hlens[b]]) for b in range(len(hlens))]
    got = search.greedy_batch(hs_pad, hlens)
    assert [h.yseq for h in got] == [h.yseq for h in one] and [h.score for h in got] == [h.score for h in one]


# ---- 4. one host read ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(3, 12), (33, 40), (70, 12)])
def test_greedy_batch_reads_the_host_once(B, T, monkeypatch):
    """blocking device-to-host reads counted as test_transducer_search_one_host_read_per_pass counts them: exactly one per call,
    whatever B and T (70 rows: two chunks)"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    sd = seeded_weights(5, "lstm", 1, 64, E_S, 52, 257, D_S, 4.0)
    bs = BeamSearchTransducer(decoder=_decoder(sd, "lstm", 1, 64, E_S, 52, 257, D_S), beam_size=1)
    hs = torch.randn(B, T, D_S, generator=torch.Generator().manual_seed(B)).to(DEV)
    hl = torch.full((B,), T, dtype=torch.int32).to(DEV)
    reads = [0]
    for meth in ("tolist", "item", "cpu", "numpy"):
        orig = getattr(torch.Tensor, meth)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                reads[0] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, meth, counted)
    counts = []
    for hlens in (None, [T] * B, hl):
        reads[0] = 0
        got = bs.greedy_batch(hs, hlens)
        counts.append(reads[0])
    monkeypatch.undo()
    assert len(got) == B and counts == [1, 1, 1], counts


# ---- 5. graph steps -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,H", [("lstm", 64), ("lstm", 12), ("gru", 12)])
def test_graph_steps_replay_bit_identical(dtype, H):
    """graph_steps: the first call of a signature runs eagerly, the second captures the frame pair and replays it, the third only
    replays - tokens and scores bit-identical to the eager call; another B has its own signature (and an odd T its spare frame)"""
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    L, J, V, B, T = 2, 52, 257, 5, 11
    sd = seeded_weights(11, dtype, L, H, E_S, J, V, D_S, 4.0)
    dec = _decoder(sd, dtype, L, H, E_S, J, V, D_S)
    g = torch.Generator().manual_seed(3)
    hs = torch.randn(B, T, D_S, generator=g).to(DEV)
    hlens = [11, 7, 10, 1, 9]
    eager = BeamSearchTransducer(decoder=dec, beam_size=1).greedy_batch(hs, hlens)
    assert any(len(h.yseq) > 1 for h in eager)
    bs = BeamSearchTransducer(decoder=dec, beam_size=1)
    bs.graph_steps = True
    runs = [bs.greedy_batch(hs, hlens) for _ in range(3)]
    assert bs.graph_steps and len(bs._greedy_graphs) == 1
    ws = next(iter(bs._greedy_graphs.values()))
    assert ws["graph"] is not None and ws["calls"] == 3
    for r in runs:
        assert [h.yseq for h in r] == [h.yseq for h in eager]
        assert [np.float32(h.score).tobytes() for h in r] == [np.float32(h.score).tobytes() for h in eager]
    hs2 = torch.randn(B + 2, T, D_S, generator=g).to(DEV)           # other inputs through the captured step, and another B
    other = bs.greedy_batch(hs2[:B], hlens)
    want = BeamSearchTransducer(decoder=dec, beam_size=1).greedy_batch(hs2[:B], hlens)
    assert [h.yseq for h in other] == [h.yseq for h in want]
    assert [np.float32(h.score).tobytes() for h in other] == [np.float32(h.score).tobytes() for h in want]
    bs.greedy_batch(hs2, hlens + [11, 11])
    assert len(bs._greedy_graphs) == 2                                # B + 2 rows did not reuse the captured step
    assert [w["graph"] is not None for w in bs._greedy_graphs.values()] == [True, False]
