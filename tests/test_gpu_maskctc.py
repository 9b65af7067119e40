"""Mask-CTC on the GPU (nets/e2e_asr_maskctc.py, eamd_maskctc_seed / eamd_maskctc_update): training against the reference's
recorded losses and gradients (tests/golden/maskctc.npz, tools/gen_golden_maskctc.py), the two decode kernels against the numpy
restatement of tests/test_maskctc.py, decoding against the reference's hypotheses, batches against single utterances, and the
two host reads of a batched decode."""
import argparse

import numpy as np
import pytest
import torch

from conftest import load_golden, seeded_weights
from test_maskctc import KS, seed_ref, update_ref

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
    return load_golden("maskctc.npz")


def train_model(enc):
    from espnet_amd.nets.e2e_asr_maskctc import E2E
    from tools.gen_golden_maskctc import TRAIN_IDIM, TRAIN_ODIM, TRAIN_SALT, train_ns
    m = E2E(TRAIN_IDIM, TRAIN_ODIM, argparse.Namespace(**train_ns(enc)))
    return seeded_weights().fill_parameters(m, salt=TRAIN_SALT[enc]).to(DEV).train()


def train_forward(model, golden, seed):
    np.random.seed(seed)
    xs = torch.from_numpy(golden["tr_xs"]).to(DEV)
    return model(xs, torch.from_numpy(golden["tr_ilens"]), torch.from_numpy(golden["tr_ys"]))


# ---- 1. training ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["transformer", "conformer"])
@pytest.mark.parametrize("seed", [0, 1])
def test_training_matches_reference_fp32(golden, enc, seed):
    from test_gpu_model import _check_seeded
    tag = "tr_%s_s%d" % (enc, seed)
    model = train_model(enc)
    loss = train_forward(model, golden, seed)
    loss.backward()
    for name, got in (("loss", loss), ("loss_ctc", model.ctc.loss), ("loss_att", model._loss_att_t)):
        ref = float(golden[tag + "_" + name])
        rel = abs(float(got) - ref) / abs(ref)
        print(f"[parity] maskctc {tag} {name} hip={float(got):.6f} ref={ref:.6f} rel={rel:.2e}")
        assert rel < 1e-5, name
    assert abs(model.acc - float(golden[tag + "_acc"])) < 1e-6
    _check_seeded(model, golden, 1e-3, prefix=tag + "/")


@pytest.mark.parametrize("enc", ["transformer", "conformer"])
def test_training_matches_reference_bf16(golden, enc):
    import espnet_amd
    tag = "tr_%s_s0" % enc
    model = train_model(enc)
    espnet_amd.set_precision("bf16")
    loss = train_forward(model, golden, 0)
    loss.backward()
    espnet_amd.set_precision("fp32")
    rel = abs(float(loss) - float(golden[tag + "_loss"])) / abs(float(golden[tag + "_loss"]))
    print(f"[parity] maskctc {tag} bf16 loss rel={rel:.2e}")
    assert rel < 1e-3


@pytest.mark.parametrize("enc", ["transformer", "conformer"])
def test_reference_state_dict_loads_strictly(golden, enc):
    SW = seeded_weights()
    model = train_model(enc)
    sd = {}
    for k, shp in zip(golden["keys_" + enc].tolist(), golden["shapes_" + enc].tolist()):
        shape = [int(v) for v in shp if v]
        own = model.state_dict()[k] if k in model.state_dict() else None
        sd[k] = SW.seeded_value(k, shape, salt=5) if own is None or own.is_floating_point() else own.clone()
    model.load_state_dict(sd, strict=True)
    assert model.decoder.output_layer.weight.shape[0] == 13 and model.ctc.ctc_lo.weight.shape[0] == 13
    assert (model.mask_token, model.sos, model.eos) == (12, 11, 11)


def test_bucketed_graph_step_matches_eager_step(golden):
    """train.BucketedGraphStep on a padded batch (eager first sight, capture, replay) against the eager step on the exact
    shapes, same numpy masking draws each time; an optimizer with learning rate 0 keeps every call the same step"""
    from espnet_amd import train
    xs, il, ys = torch.from_numpy(golden["tr_xs"]), golden["tr_ilens"].tolist(), torch.from_numpy(golden["tr_ys"])
    steps = []
    for _ in range(2):
        m = train_model("transformer")
        flat = train.FlatParams(m)
        steps.append((m, flat, train.NoamAdam(flat, mode="const", base_lr=0.0, max_grad_norm=0.0)))
    m, flat, opt = steps[1]
    np.random.seed(3)
    ref = float(train.train_step(m, flat, opt, m.prepare(xs, il, ys)))
    bstep = train.BucketedGraphStep(*steps[0], t_edge=64, l_edge=8)
    assert bstep.bucket(xs, il, ys) == (3, 128, 16)
    for mode in ("eager", "capture", "replay"):
        np.random.seed(3)
        got = float(bstep(xs, il, ys))
        print(f"[parity] maskctc bucketed step ({mode}): {got:.6f} eager exact-shape {ref:.6f}")
        assert abs(got - ref) <= 1e-5 * abs(ref), mode
    assert bstep.stats()["captures"] == 1 and bstep.stats()["hits"] == 1


# ---- 2. seed kernel ------------------------------------------------------------------------------------------------------
def seed_batch(B, T, V, seed, kinds):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g) * 3
    hl = [T] * B
    for b, kind in enumerate(kinds):
        if kind == "short":
            hl[b] = 1
        elif kind == "ragged":
            hl[b] = max(1, T // 3 + b)
        elif kind == "blank":
            x[b, :, 0] += 50.0
        elif kind == "long_run":
            x[b, :, min(3, V - 1)] += 50.0
        elif kind == "alternate":
            for t in range(T):
                x[b, t, 1 + (t // 2) % 2] += 30.0
                if t % 5 == 4:
                    x[b, t, 0] += 60.0
        elif kind == "ties":
            top = x[b].max(-1).values + 1.0
            x[b, :, V - 1] = top
            x[b, :, V // 2] = top            # equal p: the lower index wins
        elif kind == "sharp":
            x[b] *= 8.0
    return x, hl


def check_seed(x, hl, thr, K, mask_token, eos):
    from espnet_amd import ops
    B, T, V = x.shape
    xd = x.to(DEV).contiguous()
    out = ops.maskctc_seed(xd, torch.tensor(hl, dtype=torch.int32, device=DEV), thr, K, mask_token, eos, Lcap=max(hl))
    fid, fp = out["frame_id"].cpu().numpy(), out["frame_p"].cpu().numpy()
    lp = torch.log_softmax(x.double(), -1)
    p64 = lp.exp()
    top2 = p64.topk(2, -1)
    for b in range(B):
        n = hl[b]
        assert np.allclose(fp[b, :n], top2.values[b, :n, 0].numpy(), rtol=1e-5, atol=1e-7), b
        clear = (top2.values[b, :n, 0] - top2.values[b, :n, 1] > 1e-5 * top2.values[b, :n, 0]).numpy()
        ref_id = np.argmax(p64[b, :n].numpy(), -1)
        assert (fid[b, :n][clear] == ref_id[clear]).all(), b
    y, tp = out["y_in"].cpu().numpy(), out["tok_p"].cpu().numpy()
    host = {k: out[k].cpu().numpy() for k in ("len", "nmask", "niter", "kper")}
    for b in range(B):
        ry, rp, M, nit, kp = seed_ref(fid[b, :hl[b]], fp[b, :hl[b]], thr, K, mask_token)
        L = len(ry)
        assert (host["len"][b], host["nmask"][b], host["niter"][b], host["kper"][b]) == (L, M, nit, kp), b
        assert y[b, :L].tolist() == ry.tolist() and (y[b, L:] == eos).all(), b
        assert tp[b, :L].tobytes() == rp.tobytes(), b
    return out


@pytest.mark.parametrize("T,V", [(4096, 6), (37, 6), (700, 5001), (300, 16384)])
def test_seed_kernel_matches_restatement(T, V):
    kinds = ["ragged", "short", "blank", "long_run", "alternate", "ties", "sharp", "plain"]
    x, hl = seed_batch(len(kinds), T, V, T + V, kinds)
    mask_token, eos = V - 1, V - 2
    for thr, K in ((0.999, 10), (0.5, 0), (0.0, 3), (2.0, 1)):
        out = check_seed(x, hl, thr, K, mask_token, eos)
    assert (out["frame_id"][5, :hl[5]] == V // 2).all()          # equal p: the first index
    # thresholds exactly at a token's probability: that token is kept
    tp, ln = out["tok_p"].cpu().numpy(), out["len"].cpu().numpy()
    b = int(np.argmax(ln))
    if ln[b]:
        thr = float(tp[b, ln[b] // 2])
        o = check_seed(x, hl, thr, 3, mask_token, eos)        # (the restatement keeps a token at p == thr)
        assert o["tok_p"][b, ln[b] // 2].item() == thr


def test_seed_kernel_edge_utterances():
    """all-blank utterance (no token: len 0, nothing masked) and an utterance of one frame"""
    x, hl = seed_batch(3, 50, 40, 1, ["blank", "short", "plain"])
    out = check_seed(x, hl, 0.9, 10, 39, 38)
    assert out["len"][0].item() == 0 and out["niter"][0].item() == 0 and out["len"][1].item() <= 1


# ---- 3. update kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [7, 5001])
def test_update_kernel_matches_restatement(V):
    from espnet_amd import ops
    g = torch.Generator().manual_seed(V)
    B, ldy, mt = 6, 40, V - 1
    lens = [40, 23, 0, 11, 30, 5]
    niter = [10, 3, 0, 1, 30, 2]
    y = torch.randint(1, V - 2, (B, ldy), generator=g)
    for b in range(B):
        sel = torch.rand(ldy, generator=g) < 0.6
        y[b][sel] = mt
        y[b, lens[b]:] = V - 2
    y[1, 2] = mt
    M = [int((y[b, :lens[b]] == mt).sum()) for b in range(B)]
    niter = [min(n, m) for n, m in zip(niter, M)]
    kper = [m // n if n else 0 for m, n in zip(M, niter)]
    yd = y.to(DEV).contiguous()
    Ld = max(lens)
    dl = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    yh = y.numpy().copy()
    for p in range(max(niter) + 2):                  # two passes beyond the last: every utterance frozen
        x = torch.randn(B, Ld, V, generator=g)
        x[0, :, 3] = 100.0                           # utterance 0: all scores tie (lower positions first), argmax 3
        x[1, 2, mt] = 100.0                          # <mask> predicted at a masked position: it stays masked
        x[4, :, : V // 2] = x[4, :, : V // 2].round()   # ties in scores and in the argmax
        ops.maskctc_update(p, x.to(DEV).contiguous(), yd, dl(lens), dl(niter), dl(kper), mt)
        xs = x.numpy()
        for b in range(B):
            L = lens[b]
            yh[b, :L] = update_ref(yh[b, :L], xs[b, :L].max(-1) if L else [], xs[b, :L].argmax(-1) if L else [], p, niter[b],
                                   kper[b], mt)
        assert yd.cpu().numpy().tolist() == yh.tolist(), p
    assert yd[1, 2].item() == mt


# ---- 4. decoding against the reference -----------------------------------------------------------------------------------
_models = {}


def decode_model(enc):
    if enc not in _models:
        from espnet_amd.nets.e2e_asr_maskctc import E2E
        from tools.gen_golden_maskctc import decode_spec
        _models[enc] = seeded_weights().decode_r4_model(E2E, decode_spec(enc)).to(DEV)
    return _models[enc]


def dec_x(golden, enc, u):
    from tools.gen_golden_maskctc import decode_inputs
    return decode_inputs(int(golden["dec_%s_u%d_seed" % (enc, u)]))[u].numpy()


def ra(thr, K):
    return argparse.Namespace(maskctc_probability_threshold=float(thr), maskctc_n_iterations=K)


@pytest.mark.parametrize("enc", ["transformer", "conformer"])
def test_recognize_matches_reference(golden, enc):
    model = decode_model(enc)
    bad = []
    for u in range(3):
        tag = "dec_%s_u%d" % (enc, u)
        x = dec_x(golden, enc, u)
        for ti, thr in enumerate(golden[tag + "_thr"].tolist()):
            for K in KS:
                hyp = model.recognize(x, ra(thr, K))
                want = golden["%s_t%d_k%d_yseq" % (tag, ti, K)].tolist()
                if hyp[0]["yseq"] != want or hyp[0]["score"] != 0.0:
                    bad.append((tag, ti, K))
    assert not bad, bad


# ---- 5. batches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["transformer", "conformer"])
def test_recognize_batch_equals_single_utterances(golden, enc):
    model = decode_model(enc)
    xs = [dec_x(golden, enc, u) for u in range(3)]
    if enc == "conformer":     # the convolution module sees a padded utterance's padding: an equal-length batch
        n = min(len(x) for x in xs)
        xs = [x[:n] for x in xs]
    thr = float(golden["dec_%s_u0_thr" % enc][0])
    for t, K in ((thr, 3), (thr, 0), (2.0, 10), (0.0, 10)):
        batch = model.recognize_batch(xs, ra(t, K))
        assert len(batch) == len(xs)
        for x, nb in zip(xs, batch):
            assert nb == model.recognize(x, ra(t, K)), (t, K)


@pytest.mark.parametrize("K", [0, 3, 10])
def test_batched_decode_two_host_reads(golden, monkeypatch, K):
    model = decode_model("transformer")
    xs = [dec_x(golden, "transformer", u) for u in range(3)]
    reads = [0]
    for meth in ("tolist", "item", "cpu", "numpy"):
        orig = getattr(torch.Tensor, meth)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda:
                reads[0] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, meth, counted)
    nb = model.recognize_batch(xs, ra(2.0, K))
    monkeypatch.undo()
    print("[passes] K=%d: %d host reads" % (K, reads[0]))
    assert len(nb) == 3 and reads[0] == 2 == model.host_reads
