"""E-Branchformer on the GPU: the gating-unit kernels of csrc/cgmlp.hip (eamd_csgu_fwd / eamd_csgu_bwd) and the encoder built
on them (espnet_amd.espnet2.EBranchformerEncoder) against the float64 restatement of tests/branchformer_restatement.py.

Every error is the largest absolute difference to float64 over the tensor, divided by the largest |float64 value| of that
tensor.  Each bound is 4x the largest error observed under its name on an MI355X (noted beside it); the kernel checks
also compute the same formulas with torch in float32 on the device and require the kernel's error to stay within 4x of
torch's.  Output buffers and the workspace are filled with NaN before the launch, accumulated gradients start from non-zero
values.  The time tile of the kernels is 64 frames, the channel slab 64 channels; the last kernel case makes a workgroup
of the backward tile kernel walk two tiles."""
import pytest
import torch

import branchformer_restatement as br

pytestmark = pytest.mark.gpu

DEV = "cuda"
# observed maxima over the cases below: y 2.48e-7, da 2.63e-7, dw 2.10e-7, dbias 1.66e-7, dgamma 2.67e-7, dbeta 2.44e-7
# (torch float32 on the same inputs: 1.41e-7, 1.42e-7, 3.49e-7, 1.42e-7, 7.89e-7, 2.13e-7)
CSGU_TOL = dict(y=9.9e-7, da=1.05e-6, dw=8.4e-7, dbias=6.6e-7, dgamma=1.07e-6, dbeta=9.8e-7)
ENC_OUT_TOL = 1.03e-6     # output; observed 2.56e-7 (two blocks, relative positions)
ENC_GRAD_TOL = 6.7e-6     # any parameter gradient; observed 1.68e-6 (two blocks, relative positions)


def rel_err(got, ref):
    d = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return float(d.max() / ref.abs().max().clamp_min(1e-30))


def csgu_call(lib, a, gamma, beta, w, bias, dy, acc0):
    """the two entry points on NaN-filled outputs; acc0 = starting values of (dw, dbias, dgamma, dbeta)"""
    B, T, C2 = a.shape
    Ch, K = C2 // 2, w.shape[-1]
    L, p = lib.lib(), lib.ptr
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    y, stats, da = nan(B, T, Ch), nan(B * T, 2), nan(B, T, C2)
    ws = nan(L.eamd_csgu_bwd_workspace(B, T, Ch, K))
    acc = [t.clone() for t in acc0]
    lib.check(L.eamd_csgu_fwd(p(a), p(gamma), p(beta), p(w), p(bias), br.EPS, p(y), p(stats), B, T, Ch, K, lib.stream_ptr()), "fwd")
    lib.check(L.eamd_csgu_bwd(p(dy), p(a), p(stats), p(gamma), p(beta), p(w), p(bias), p(da), *[p(t) for t in acc], p(ws),
                              B, T, Ch, K, lib.stream_ptr()), "bwd")
    return [y, da] + acc


def formulas(args, dy, acc0):
    """br.csgu and its autograd in the dtype / on the device of args -> the same six outputs"""
    a, gamma, beta, w, bias = [t.detach().clone().requires_grad_(True) for t in args]
    y = br.csgu(a, gamma, beta, w, bias)
    y.backward(dy)
    return [y, a.grad] + [s + g for s, g in zip(acc0, (w.grad, bias.grad, gamma.grad, beta.grad))]


@pytest.mark.parametrize("B,T,Ch,K", [(1, 1, 8, 31), (1, 7, 72, 31), (3, 7, 8, 15), (3, 65, 72, 15), (1, 65, 1024, 3),
                                      (1, 130, 8, 3), (3, 130, 1024, 31), (12, 130, 1024, 31)])
def test_csgu_kernels(B, T, Ch, K):
    from espnet_amd import _lib
    g = torch.Generator().manual_seed(B * 1000 + T + Ch + K)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    args = [rn(B, T, 2 * Ch), 1 + 0.1 * rn(Ch), 0.1 * rn(Ch), rn(Ch, 1, K) / K ** 0.5, 1 + 0.1 * rn(Ch)]
    dy, acc0 = rn(B, T, Ch), [rn(Ch, 1, K), rn(Ch), rn(Ch), rn(Ch)]
    ref = formulas([t.double() for t in args], dy.double(), [t.double() for t in acc0])
    dev = [t.to(DEV) for t in args]
    f32 = formulas(dev, dy.to(DEV), [t.to(DEV) for t in acc0])
    got = csgu_call(_lib, *dev, dy.to(DEV), [t.to(DEV) for t in acc0])
    for name, k, t, r in zip(CSGU_TOL, got, f32, ref):
        ek, et = rel_err(k, r), rel_err(t, r)
        print(f"[branchformer] csgu {name} B{B} T{T} Ch{Ch} K{K}: kernel {ek:.3e} torch-fp32 {et:.3e} (tol {CSGU_TOL[name]:g})")
        assert ek <= CSGU_TOL[name], f"{name}: {ek:.3e} > {CSGU_TOL[name]:g}"
        assert ek <= 4 * et, f"{name}: kernel error {ek:.3e} above 4x torch float32's {et:.3e}"
    if B > 1:      # the halo must not read the neighbouring utterance: each one alone gives the same bits
        for b in range(B):
            alone = csgu_call(_lib, dev[0][b:b + 1].contiguous(), *dev[1:], dy[b:b + 1].to(DEV), [t.to(DEV) for t in acc0])[0]
            assert torch.equal(alone[0], got[0][b]), f"utterance {b} differs from its B = 1 call"


@pytest.mark.parametrize("kw,what", [(dict(cgmlp_conv_kernel=8), "odd"), (dict(cgmlp_linear_units=2 * 2056), "2048"),
                                     (dict(cgmlp_linear_units=24), "multiple of 8")])
def test_unsupported_shapes_are_refused(kw, what):
    from espnet_amd import _lib, ops
    from espnet_amd.espnet2 import EBranchformerEncoder
    with pytest.raises(NotImplementedError, match=what):
        EBranchformerEncoder(20, 32, 2, **kw)
    Ch, K = kw.get("cgmlp_linear_units", 64) // 2, kw.get("cgmlp_conv_kernel", 31)
    z = torch.zeros(5, 2 * Ch, device=DEV)
    with pytest.raises(_lib.EamdError, match=what):
        ops.csgu_fwd(z, z[0, :Ch], z[0, :Ch], torch.zeros(Ch, K, device=DEV), z[0, :Ch], br.EPS, 1, 5, Ch, K)


def tiny(rel, num_blocks, seed=0):
    """the float64 restatement with non-trivial gating parameters, and the product encoder loaded from its state dict"""
    from espnet_amd.espnet2 import EBranchformerEncoder
    torch.manual_seed(seed)
    ref = br.EBranchformerEncoder(20, rel=rel, num_blocks=num_blocks)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "csgu.conv.weight" in n:
                p.normal_(0, 7 ** -0.5)
            elif "norm" in n or "csgu.conv.bias" in n:
                p.copy_((1.0 if n.endswith("weight") or "conv" in n else 0.0) + 0.1 * torch.randn_like(p))
    names = ("rel_selfattn", "rel_pos") if rel else ("selfattn", "abs_pos")
    enc = EBranchformerEncoder(20, 32, 2, *names, cgmlp_linear_units=64, cgmlp_conv_kernel=7, num_blocks=num_blocks,
                               dropout_rate=0.0, positional_dropout_rate=0.0, attention_dropout_rate=0.0, input_layer="linear",
                               use_ffn=True, macaron_ffn=True, linear_units=64, merge_conv_kernel=3)
    enc.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return ref.double(), enc.to(DEV)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("num_blocks", [1, 2])
@pytest.mark.parametrize("rel", [False, True])
def test_encoder_matches_restatement(rel, num_blocks, train):
    import espnet_amd
    espnet_amd.set_precision("fp32")
    ref, enc = tiny(rel, num_blocks)
    enc.train(train)
    g = torch.Generator().manual_seed(1)
    xs, lens, R = torch.randn(2, 11, 20, generator=g), [11, 7], torch.randn(2, 11, 32, generator=g)
    want = ref(xs.double(), lens)
    (want * R.double()).sum().backward()
    out, olens, _ = enc(xs.to(DEV), torch.tensor(lens))
    (out * R.to(DEV)).sum().backward()
    assert olens.tolist() == lens and not torch.isnan(out).any()
    eo = rel_err(out, want.detach())
    # a gradient that cancels to (nearly) nothing, such as the key bias's under the softmax, is judged against the largest
    # gradient of the model: its rounding noise scales with what flows through backward, not with the sum that is left
    rg = {n: p.grad for n, p in ref.named_parameters()}
    floor = 1e-3 * max(float(v.abs().max()) for v in rg.values())
    eg = max(rel_err(p.grad, rg[n]) * float(rg[n].abs().max()) / max(float(rg[n].abs().max()), floor)
             for n, p in enc.named_parameters())
    print(f"[branchformer] encoder rel={rel} blocks={num_blocks} train={train}: out {eo:.3e} grads {eg:.3e}")
    assert eo <= ENC_OUT_TOL and eg <= ENC_GRAD_TOL


def test_five_training_steps_reduce_the_loss():
    from espnet_amd.espnet2 import CTC, ESPnetASRModel, TransformerDecoder
    _, enc = tiny(True, 2)
    torch.manual_seed(2)
    dec = TransformerDecoder(30, 32, attention_heads=2, linear_units=64, num_blocks=1, dropout_rate=0.0, positional_dropout_rate=0.0)
    model = ESPnetASRModel(vocab_size=30, encoder=enc, decoder=dec, ctc=CTC(30, 32, ctc_type="builtin"), ctc_weight=0.3).to(DEV).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    g = torch.Generator().manual_seed(3)
    speech, slen = torch.randn(2, 11, 20, generator=g).to(DEV), torch.tensor([11, 7])
    text, tlen = torch.randint(1, 29, (2, 4), generator=g), torch.tensor([4, 3])
    text[1, 3] = -1
    text = text.to(DEV)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = model(speech, slen, text, tlen)[0]
        loss.sum().backward()
        opt.step()
        losses.append(float(loss))
    print("[branchformer] losses", losses)
    assert all(x == x for x in losses) and losses[-1] < losses[0]
