"""branchformer_restatement.py checked on its own (CPU): its parameter names are the E-Branchformer's, and its float64
gating unit is differentiable as written."""
import torch

import branchformer_restatement as br

LAYER_KEYS = [f"{m}.{p}" for p in ("weight", "bias") for m in (
    "attn.linear_q", "attn.linear_k", "attn.linear_v", "attn.linear_out", "cgmlp.channel_proj1.0", "cgmlp.csgu.norm",
    "cgmlp.csgu.conv", "cgmlp.channel_proj2", "feed_forward.w_1", "feed_forward.w_2", "feed_forward_macaron.w_1",
    "feed_forward_macaron.w_2", "norm_ff", "norm_ff_macaron", "norm_mha", "norm_mlp", "norm_final", "depthwise_conv_fusion",
    "merge_proj")]
REL_KEYS = ["attn.linear_pos.weight", "attn.pos_bias_u", "attn.pos_bias_v"]
OUTER_KEYS = ["embed.0.weight", "embed.0.bias", "embed.1.weight", "embed.1.bias", "after_norm.weight", "after_norm.bias"]


def test_state_dict_keys():
    for rel in (False, True):
        want = OUTER_KEYS + [f"encoders.{i}.{k}" for i in range(2) for k in LAYER_KEYS + (REL_KEYS if rel else [])]
        assert sorted(br.EBranchformerEncoder(20, rel=rel).state_dict()) == sorted(want)


def test_csgu_gradcheck():
    g = torch.Generator().manual_seed(0)
    B, T, Ch, K = 1, 5, 8, 3
    args = [torch.randn(B, T, 2 * Ch, generator=g), 1 + 0.1 * torch.randn(Ch, generator=g), 0.1 * torch.randn(Ch, generator=g),
            torch.randn(Ch, 1, K, generator=g) / K ** 0.5, 1 + 0.1 * torch.randn(Ch, generator=g)]
    assert torch.autograd.gradcheck(br.csgu, [t.double().requires_grad_(True) for t in args])
