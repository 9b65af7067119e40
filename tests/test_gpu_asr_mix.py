"""Multi-speaker Transformer ASR on the GPU (nets/e2e_asr_mix_transformer.py, eamd_ctc_pit_loss): the PIT kernel against a float64
CTC plus the PIT restatement of tests/test_asr_mix.py and against eamd_ctc_loss, CTC(reduce=False), training against the
reference's recorded losses, permutations and gradients (tests/golden/asr_mix.npz, tools/gen_golden_asr_mix.py), the bucketed
graph step, decoding against the reference's n-best lists, batches against single utterances, and the host syncs of a step."""
import argparse

import numpy as np
import pytest
import torch

from conftest import load_golden, seeded_weights
from test_asr_mix import ALPHAS, SPKRS, pit_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _fp32():
    import espnet_amd
    espnet_amd.set_precision("fp32")
    yield
    espnet_amd.set_precision("fp32")


@pytest.fixture(scope="module")
def golden():
    return load_golden("asr_mix.npz")


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------
def pit_batch(S, B, T, V, L, seed, kinds=()):
    """acts [S,B,T,V], ys [B,S,L] (padded -1), ilens [B]: ragged lengths; kinds[b] in {"empty", "tie", "short"}"""
    g = torch.Generator().manual_seed(seed)
    acts = torch.randn(S, B, T, V, generator=g) * 2
    ilens = torch.randint(max(1, T // 2), T + 1, (B,), generator=g)
    ilens[0] = T
    ys = torch.full((B, S, L), -1, dtype=torch.int64)
    for b in range(B):
        for s in range(S):
            n = int(torch.randint(max(0, L // 3), L + 1, (1,), generator=g))
            n = min(n, max(0, int(ilens[b]) // 2 - 1))
            ys[b, s, :n] = torch.randint(1, V, (n,), generator=g)
    for b, kind in enumerate(kinds):
        if kind == "empty":
            ys[b, S - 1] = -1
        elif kind == "tie":
            ys[b, 1] = ys[b, 0]
        elif kind == "short":                    # more labels than frames for every speaker: no permutation is feasible
            ilens[b] = 3
            ys[b, :, :min(L, 5)] = torch.randint(1, V, (S, min(L, 5)), generator=g)
    return acts, ys, ilens.to(torch.int32)


def nll_pair_f64(acts, ys, ilens):
    """[B, S, S] float64 -log p of hypothesis i against reference j (torch CTC on float64 log-softmax; +inf where infeasible)"""
    S, B, T, V = acts.shape
    lp = torch.log_softmax(acts.double(), -1)
    tl = (ys != -1).sum(-1)
    out = torch.empty(B, S, S, dtype=torch.float64, device=acts.device)
    for i in range(S):
        for j in range(S):
            out[:, i, j] = torch.nn.functional.ctc_loss(lp[i].transpose(0, 1), ys[:, j].clamp_min(0), ilens.long(), tl[:, j],
                                                        blank=0, reduction="none", zero_infinity=False)
    return out


def run_pit(acts, ys, ilens, scale):
    from espnet_amd import ops
    return ops.ctc_pit_loss(acts.to(DEV).contiguous(), ys.to(DEV).contiguous(), ilens.to(DEV), 0, -1, scale, want_grad=True)


CASES = [  # S, B, T', L, V
    (2, 4, 50, 12, 52), (3, 5, 60, 10, 52), (2, 32, 1000, 150, 52), (3, 16, 400, 100, 52), (2, 3, 120, 30, 5000),
    (3, 2, 80, 20, 5000),
]


@pytest.mark.parametrize("S,B,T,L,V", CASES)
def test_pit_kernel_matches_float64(S, B, T, L, V):
    kinds = ["empty", "tie"] + [""] * B
    acts, ys, il = pit_batch(S, B, T, V, L, seed=S * 1000 + B + T, kinds=kinds[:B])
    scale = 1.0 / (S * B * B)
    nll, perm, pit, grad = run_pit(acts, ys, il, scale)
    ref = nll_pair_f64(acts.to(DEV), ys.to(DEV), il.to(DEV))
    err = ((nll.double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
    print(f"[pit] S={S} B={B} T'={T} L={L} V={V}: nll_pair rel err {err:.2e}")
    assert err < 2e-5
    # the choice from the kernel's own pair matrix, in the reference's float32 arithmetic
    pair = (nll.cpu().numpy() / np.float32(B)).reshape(B, S * S)
    p_ref, pit_r = pit_ref(pair)
    assert perm.cpu().tolist() == p_ref.tolist()
    assert np.array_equal(pit.cpu().numpy(), pit_r)
    # gradient of scale * sum_b sum_i nll[b, i, perm] against float64 autograd
    a = acts.to(DEV).double().requires_grad_(True)
    r = nll_pair_f64(a, ys.to(DEV), il.to(DEV))
    pm = perm.to(DEV)
    sel = torch.gather(r, 2, pm.unsqueeze(-1)).sum() * scale
    sel.backward()
    # fp32 carries the log-space lattice to ~1e-7 of its magnitude (-log p grows with T'), so the occupancies of a lattice are
    # compared relative to grad_scale * max(1, its -log p), as the eamd_ctc_loss tests do (test_gpu_row_kernels.ctc_ref)
    nsel = torch.gather(nll.double(), 2, pm.unsqueeze(-1)).squeeze(-1).clamp_min(1.0)          # [B, S]
    gerr = ((grad.double() - a.grad).abs() / (scale * nsel.t().reshape(S, B, 1, 1))).max().item()
    print(f"[pit]   grad err / (scale * nll) {gerr:.2e}")
    assert gerr < 1e-5
    t = torch.arange(T, device=DEV).view(1, 1, T, 1)
    assert (grad.masked_select(t >= il.to(DEV).view(1, B, 1, 1)) == 0).all()


def test_pit_kernel_tie_takes_the_first_permutation():
    S, B = 2, 3
    acts, ys, il = pit_batch(S, B, 40, 52, 8, seed=5, kinds=["tie", "tie", "tie"])
    acts[1] = acts[0]                   # both hypotheses identical as well: every permutation scores the same
    nll, perm, pit, _ = run_pit(acts, ys, il, 1.0)
    assert (nll[:, :, 0] == nll[:, :, 1]).all()
    assert perm.cpu().tolist() == [[0, 1]] * B
    for S in (2, 3):
        acts = torch.zeros(S, 1, 10, 6)
        ys = torch.tensor([[[1, 2]] * S])
        _, perm, _, _ = run_pit(acts, ys, torch.tensor([10], dtype=torch.int32), 1.0)
        assert perm.cpu().tolist() == [list(range(S))]


def test_pit_kernel_infeasible_utterance():
    """the speakers of an utterance share its frames, so an infeasible pair makes its reference infeasible for every hypothesis:
    every permutation scores +inf, the first is kept; the other utterances are unaffected"""
    S, B = 2, 3
    acts, ys, il = pit_batch(S, B, 40, 52, 8, seed=9, kinds=["", "short", ""])
    from espnet_amd import ops
    nll, perm, pit, _ = ops.ctc_pit_loss(acts.to(DEV), ys.to(DEV), il.to(DEV), 0, -1, 1.0, want_grad=False)
    assert torch.isinf(nll[1]).all() and torch.isinf(pit[1]) and perm[1].tolist() == [0, 1]
    assert torch.isfinite(pit[[0, 2]]).all()


def test_pit_kernel_rejects_other_speaker_counts():
    from espnet_amd import ops
    from espnet_amd._lib import EamdError
    for S in (1, 4):
        acts, ys, il = pit_batch(S, 2, 20, 8, 4, seed=1) if S > 1 else pit_batch(2, 2, 20, 8, 4, seed=1)
        if S == 1:
            acts, ys = acts[:1].contiguous(), ys[:, :1].contiguous()
        with pytest.raises(EamdError):
            ops.ctc_pit_loss(acts.to(DEV), ys.to(DEV), il.to(DEV), 0, -1, 1.0)


@pytest.mark.parametrize("S", [2, 3])
def test_pit_pairs_equal_ctc_loss_calls(S):
    """nll_pair[b, i, j] = eamd_ctc_loss on speaker i's rows with speaker j's labels (the reference's S^2 CTC calls)"""
    from espnet_amd import ops
    B, T, V, L = 6, 90, 52, 20
    acts, ys, il = pit_batch(S, B, T, V, L, seed=21 + S, kinds=["empty", "tie"])
    nll, _, _, _ = run_pit(acts, ys, il, 1.0)
    a, y, ild = acts.to(DEV), ys.to(DEV), il.to(DEV)
    for i in range(S):
        for j in range(S):
            ref, _ = ops.ctc_loss(a[i].contiguous(), y[:, j].contiguous(), ild, want_grad=False)
            assert torch.equal(nll[:, i, j], ref), (i, j)


def test_ctc_reduce_false_matches_reference_semantics():
    """CTC(reduce=False): the vector -log p_b / B (ctc.py:53-61, reduction "none") with a per-utterance backward"""
    from espnet_amd.nets.modules import CTC
    B, T, D, V = 5, 70, 16, 30
    torch.manual_seed(3)
    ctc = CTC(V, D, 0.0, reduce=False).to(DEV)
    hs = torch.randn(B, T, D, device=DEV, requires_grad=True)
    hl = torch.tensor([70, 60, 55, 40, 70], dtype=torch.int32)
    ys = torch.randint(1, V, (B, 12))
    ys[1, 8:] = -1
    ys[2, :] = -1
    loss = ctc(hs, hl, ys)
    assert loss.shape == (B,)
    g = torch.rand(B, device=DEV) + 0.5
    loss.backward(g)
    h64 = hs.detach().double().requires_grad_(True)
    lp = torch.log_softmax(torch.nn.functional.linear(h64, ctc.ctc_lo.weight.double(), ctc.ctc_lo.bias.double()), -1)
    tl = (ys != -1).sum(-1)
    ref = torch.nn.functional.ctc_loss(lp.transpose(0, 1), ys.clamp_min(0).to(DEV), hl.long().to(DEV), tl.to(DEV), reduction="none") / B
    assert ((loss.double() - ref).abs() / ref.abs()).max().item() < 1e-5
    (ref * g.double()).sum().backward()
    assert ((hs.grad.double() - h64.grad).abs().max() / h64.grad.abs().max()).item() < 1e-4


# ---- 2. training -----------------------------------------------------------------------------------------------------------
def train_model(S, alpha):
    from espnet_amd.nets.e2e_asr_mix_transformer import E2E
    from tools.gen_golden_asr_mix import TRAIN_IDIM, TRAIN_ODIM, TRAIN_SALT, train_ns
    m = E2E(TRAIN_IDIM, TRAIN_ODIM, argparse.Namespace(**train_ns(S, alpha)))
    return seeded_weights().fill_parameters(m, salt=TRAIN_SALT).to(DEV).train()


def batch(golden, S):
    return (torch.from_numpy(golden["tr_s%d_xs" % S]), torch.from_numpy(golden["tr_s%d_ilens" % S]),
            torch.from_numpy(golden["tr_s%d_ys" % S]))


@pytest.mark.parametrize("S", SPKRS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_training_matches_reference_fp32(golden, S, alpha):
    from test_gpu_model import _check_seeded
    tag = "tr_s%d_a%g" % (S, alpha)
    model = train_model(S, alpha)
    xs, il, ys = batch(golden, S)
    loss = model(xs.to(DEV), il, ys)
    loss.backward()
    B = xs.shape[0]
    checks = [("loss", loss), ("loss_ctc", model._loss_ctc_t)]
    if alpha < 1:
        checks.append(("loss_att", model._loss_att_t))
        assert abs(model.acc - float(golden[tag + "_acc"])) < 1e-6
    for name, got in checks:
        ref = float(golden[tag + "_" + name])
        got = float(got.detach())
        rel = abs(got - ref) / abs(ref)
        print(f"[parity] asr_mix {tag} {name} hip={got:.6f} ref={ref:.6f} rel={rel:.2e}")
        assert rel < 1e-5, name
    assert model.min_perm.cpu().tolist() == golden[tag + "_perm"].tolist()
    pair = (model.pit_record["nll_pair"] / B).reshape(B, S * S).cpu().numpy()
    ref = golden[tag + "_pair"]
    assert np.abs(pair - ref).max() <= 1e-5 * np.abs(ref).max()
    _check_seeded(model, golden, 1e-3, prefix=tag + "/")


@pytest.mark.parametrize("S", SPKRS)
def test_reference_state_dict_loads_strictly(golden, S):
    SW = seeded_weights()
    model = train_model(S, 0.2)
    sd = {}
    for k, shp in zip(golden["keys_s%d" % S].tolist(), golden["shapes_s%d" % S].tolist()):
        sd[k] = SW.seeded_value(k, [int(v) for v in shp if v], salt=5)
    model.load_state_dict(sd, strict=True)
    assert len(model.encoder.encoders_sd) == S


def test_bucketed_graph_step_matches_eager_step(golden):
    """train.BucketedGraphStep on a padded batch (eager first sight, capture, replay) against the eager step on the exact shapes;
    the caller passes olens, the longest label per utterance over its speakers; learning rate 0 keeps every call the same step"""
    from espnet_amd import train
    S = 2
    xs, il, ys = batch(golden, S)
    il = il.tolist()
    olens = (ys != -1).sum(-1).max(-1).values.tolist()
    steps = []
    for _ in range(2):
        m = train_model(S, 0.2)
        m.sync_report = False
        flat = train.FlatParams(m)
        steps.append((m, flat, train.NoamAdam(flat, mode="const", base_lr=0.0, max_grad_norm=0.0)))
    m, flat, opt = steps[1]
    ref = float(train.train_step(m, flat, opt, m.prepare(xs, il, ys)).detach())
    bstep = train.BucketedGraphStep(*steps[0], t_edge=64, l_edge=8)
    assert bstep.bucket(xs, il, ys, olens) == (3, 128, 16)
    for mode in ("eager", "capture", "replay"):
        got = float(bstep(xs, il, ys, olens).detach())
        print(f"[parity] asr_mix bucketed step ({mode}): {got:.6f} eager exact-shape {ref:.6f}")
        assert abs(got - ref) <= 1e-5 * abs(ref), mode
    assert bstep.stats()["captures"] == 1 and bstep.stats()["hits"] == 1


def test_forward_core_has_no_host_sync(golden):
    """forward_core launches kernels only: it captures into a graph, and a replay gives the eager loss"""
    S = 3
    model = train_model(S, 0.2)
    model.sync_report = False
    xs, il, ys = batch(golden, S)
    b = model.prepare(xs, il, ys)
    eager = float(model.forward_core(b).detach())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad():
        with torch.cuda.graph(g):
            loss = model.forward_core(b)
    g.replay()
    torch.cuda.synchronize()
    assert abs(float(loss) - eager) <= 1e-6 * abs(eager)
    assert model.min_perm.cpu().tolist() == golden["tr_s3_a0.2_perm"].tolist()


# ---- 3. decoding -----------------------------------------------------------------------------------------------------------
def decode_model():
    from espnet_amd.nets.e2e_asr_mix_transformer import E2E
    from tools.gen_golden_asr_mix import DECODE
    return seeded_weights().decode_r4_model(E2E, DECODE).to(DEV)


def dec_x(golden, u):
    from tools.gen_golden_asr_mix import decode_inputs
    return decode_inputs(int(golden["dec_u%d_seed" % u]))[u]


def ra(c):
    from tools.gen_golden_asr_mix import CTCW, recog_args
    return recog_args(CTCW[c])


def check_nbest(golden, tag, hyps):
    ids, sc, ln = golden[tag + "_ids"], golden[tag + "_scores"], golden[tag + "_len"]
    assert len(hyps) == len(sc), tag
    for k, h in enumerate(hyps):
        assert h["yseq"] == ids[k, :ln[k]].tolist(), (tag, k)
        assert abs(h["score"] - sc[k]) <= 1e-4 * max(1.0, abs(sc[k])), (tag, k, h["score"], sc[k])


@pytest.mark.parametrize("c", [0, 1])
def test_recognize_matches_reference(golden, c):
    model = decode_model()
    for u in range(3):
        nb = model.recognize(dec_x(golden, u).numpy(), ra(c))
        assert len(nb) == 2
        for s in range(2):
            check_nbest(golden, "dec_c%d_u%d_s%d" % (c, u, s), nb[s])


@pytest.mark.parametrize("c", [0, 1])
def test_recognize_batch_equals_single(golden, c):
    model = decode_model()
    xs = [dec_x(golden, u) for u in range(3)]
    got = model.recognize_batch(xs, ra(c))
    assert len(got) == 3
    for u in range(3):
        single = model.recognize(xs[u].numpy(), ra(c))
        for s in range(2):
            assert [h["yseq"] for h in got[u][s]] == [h["yseq"] for h in single[s]]
            for a, b in zip(got[u][s], single[s]):
                assert abs(a["score"] - b["score"]) <= 1e-4 * max(1.0, abs(b["score"]))
            check_nbest(golden, "dec_c%d_u%d_s%d" % (c, u, s), got[u][s])
