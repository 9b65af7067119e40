"""E-Branchformer encoder (Kim et al., "E-Branchformer: Branchformer with enhanced merging for speech recognition",
SLT 2022): each layer runs self-attention and a convolutional gating MLP (cgMLP) side by side on the same input and
merges the two with a depthwise convolution over their concatenation.

reference classes mirrored (ESPnet, espnet2/asr/...): layers/cgmlp.py (ConvolutionalSpatialGatingUnit,
ConvolutionalGatingMLP), encoder/e_branchformer_encoder.py (EBranchformerEncoderLayer, EBranchformerEncoder) - same
constructor arguments and parameter names, so a checkpoint of the same configuration loads with load_state_dict.
The torch.nn.Linear / Conv1d / LayerNorm objects are parameter containers; the arithmetic runs on the HIP kernels:
the gating unit is csrc/cgmlp.hip (F_.CSGUFn), the merge convolution the generic depthwise kernels (F_.DepthwiseConvFn),
attention / feed-forward / LayerNorm / dropout the modules of nets/modules.py.
"""
import torch

from .. import functional as F_
from .. import ops
from . import modules as M


class ConvolutionalSpatialGatingUnit(torch.nn.Module):
    """reference: layers/cgmlp.py - x [B, T, size] -> x_r * conv(norm(x_g)) [B, T, size // 2], then dropout.
    Its input here is channel_proj1's PRE-activation: the GELU in front of the unit is applied inside the kernel."""

    def __init__(self, size, kernel_size, dropout_rate, use_linear_after_conv=False, gate_activation="identity"):
        super().__init__()
        if use_linear_after_conv:
            raise NotImplementedError("use_linear_after_conv=True is not on the HIP path (the fused gating kernel has no Linear)")
        if gate_activation != "identity":
            raise NotImplementedError("gate_activation=%r: only 'identity' is on the HIP path" % (gate_activation,))
        n_channels = size // 2
        if size % 2 or not ops.csgu_supported(n_channels, kernel_size):
            raise NotImplementedError(f"cgMLP with kernel_size {kernel_size}, size // 2 = {n_channels} has no HIP kernel "
                                      f"(supported: {ops.CSGU_LIMITS})")
        self.norm = M.LayerNorm(n_channels)
        self.conv = torch.nn.Conv1d(n_channels, n_channels, kernel_size, 1, (kernel_size - 1) // 2, groups=n_channels)
        self.linear = None
        self.dropout_rate = dropout_rate
        self.salt = ops.new_salt()
        self.espnet_initialization_fn()

    def espnet_initialization_fn(self):
        torch.nn.init.normal_(self.conv.weight, std=1e-6)
        torch.nn.init.ones_(self.conv.bias)

    def forward(self, a):
        y = F_.run(F_.CSGUFn, a, self.norm.weight, self.norm.bias, self.conv.weight, self.conv.bias, self.norm.eps)
        return F_.dropout(y, self.dropout_rate, self.salt, self.training)


class ConvolutionalGatingMLP(torch.nn.Module):
    """reference: layers/cgmlp.py - channel_proj1 (Linear + GELU), the gating unit, channel_proj2"""

    def __init__(self, size, linear_units, kernel_size, dropout_rate, use_linear_after_conv=False, gate_activation="identity"):
        super().__init__()
        self.channel_proj1 = torch.nn.Sequential(torch.nn.Linear(size, linear_units), torch.nn.GELU())
        self.csgu = ConvolutionalSpatialGatingUnit(linear_units, kernel_size, dropout_rate, use_linear_after_conv,
                                                   gate_activation)
        self.channel_proj2 = torch.nn.Linear(linear_units // 2, size)

    def forward(self, x, mask=None):
        p1, p2 = self.channel_proj1[0], self.channel_proj2
        a = F_.LinearFn.apply(x, p1.weight, p1.bias)          # GELU(a) is formed inside the gating kernels
        return F_.LinearFn.apply(self.csgu(a), p2.weight, p2.bias)


class EBranchformerEncoderLayer(torch.nn.Module):
    """reference: encoder/e_branchformer_encoder.py (EBranchformerEncoderLayer)"""

    def __init__(self, size, attn, cgmlp, feed_forward, feed_forward_macaron, dropout_rate, merge_conv_kernel=3):
        super().__init__()
        self.size = size
        self.attn = attn
        self.cgmlp = cgmlp
        self.feed_forward = feed_forward
        self.feed_forward_macaron = feed_forward_macaron
        self.ff_scale = 1.0
        if feed_forward is not None:
            self.norm_ff = M.LayerNorm(size)
        if feed_forward_macaron is not None:
            self.ff_scale = 0.5
            self.norm_ff_macaron = M.LayerNorm(size)
        self.norm_mha = M.LayerNorm(size)
        self.norm_mlp = M.LayerNorm(size)
        self.norm_final = M.LayerNorm(size)
        self.dropout_rate = dropout_rate
        if merge_conv_kernel % 2 == 0 or not 1 <= merge_conv_kernel <= 31:
            raise NotImplementedError("merge_conv_kernel must be odd and at most 31 (the depthwise HIP kernels)")
        self.depthwise_conv_fusion = torch.nn.Conv1d(2 * size, 2 * size, merge_conv_kernel, 1, (merge_conv_kernel - 1) // 2,
                                                     groups=2 * size, bias=True)
        self.merge_proj = torch.nn.Linear(2 * size, size)
        self.salts = [ops.new_salt() for _ in range(3)]

    def forward(self, x_input, mask, cache=None):
        assert cache is None, "encoder-side cache is not used on the ASR path"
        x, pos_emb = x_input if isinstance(x_input, tuple) else (x_input, None)
        p, tr = self.dropout_rate, self.training
        if self.feed_forward_macaron is not None:
            x = M.ffn_block(self.norm_ff_macaron, self.feed_forward_macaron, x, self.ff_scale, p)
        # the two branches have no residual of their own: the modules' bare forwards
        x1 = self.norm_mha(x)
        x1 = self.attn(x1, x1, x1, pos_emb, mask) if pos_emb is not None else self.attn(x1, x1, x1, mask)
        x1 = F_.dropout(x1, p, self.salts[0], tr)
        x2 = F_.dropout(self.cgmlp(self.norm_mlp(x)), p, self.salts[1], tr)
        xc = torch.cat([x1, x2], dim=-1)
        dw = self.depthwise_conv_fusion
        xm = xc + F_.DepthwiseConvFn.apply(xc, dw.weight, dw.bias)
        x = x + F_.dropout(F_.LinearFn.apply(xm, self.merge_proj.weight, self.merge_proj.bias), p, self.salts[2], tr)
        if self.feed_forward is not None:
            x = M.ffn_block(self.norm_ff, self.feed_forward, x, self.ff_scale, p)
        x = self.norm_final(x)
        return ((x, pos_emb), mask) if pos_emb is not None else (x, mask)


class _LinearInput(M._LinearInput):
    """input_layer="linear" of the espnet2 Conformer-family encoders: Linear -> torch.nn.LayerNorm (eps 1e-5) -> Dropout ->
    pos_enc, without the ReLU of the espnet1 form; state_dict keys embed.0.* / embed.1.*"""

    def __init__(self, idim, odim, dropout_rate, pos_enc):
        torch.nn.Sequential.__init__(self, torch.nn.Linear(idim, odim), torch.nn.LayerNorm(odim),
                                     torch.nn.Dropout(dropout_rate), pos_enc)
        self.salt = ops.new_salt()

    def forward(self, x):
        y = F_.LinearFn.apply(x, self[0].weight, self[0].bias)
        y = F_.run(F_.LayerNormFn, y, self[1].weight, self[1].bias, self[1].eps)
        y, pos = F_.dropout(y, self[2].p, self.salt, self.training), self[3]
        if not isinstance(pos, M.RelPositionalEncoding):
            return pos(y)
        pe = pos.pos_emb(y.size(1), y.device).unsqueeze(0)      # x * sqrt(d) on the tape: the input layer has parameters
        return (F_.dropout(F_.ScaleFn.apply(y, pos.xscale), pos.dropout_rate, pos.salt, pos.training),
                F_.dropout(pe, pos.dropout_rate, pos.salt2, pos.training))


_REL_ALIASES = {"legacy_rel_selfattn": "rel_selfattn", "legacy_rel_pos": "rel_pos"}


class EBranchformerEncoder(torch.nn.Module):
    """reference: encoder/e_branchformer_encoder.py (EBranchformerEncoder).  Relative positions are this project's form (the
    one its Conformer uses, ESPnet's legacy_rel_pos / legacy_rel_selfattn): rel_pos_type="legacy"."""

    def __init__(self, idim, attention_dim=256, attention_heads=4, attention_layer_type="rel_selfattn",
                 pos_enc_layer_type="rel_pos", rel_pos_type="legacy", cgmlp_linear_units=2048, cgmlp_conv_kernel=31,
                 use_linear_after_conv=False, gate_activation="identity", num_blocks=12, dropout_rate=0.1,
                 positional_dropout_rate=0.1, attention_dropout_rate=0.0, input_layer="conv2d", padding_idx=-1,
                 layer_drop_rate=0.0, use_ffn=True, macaron_ffn=True, ffn_activation_type="swish", linear_units=2048,
                 positionwise_layer_type="linear", merge_conv_kernel=3, interctc_layer_idx=None,
                 interctc_use_conditioning=False):
        super().__init__()
        if rel_pos_type != "legacy":
            raise NotImplementedError(
                "rel_pos_type=%r: the newer relative positional encoding (2T-1 positions) has no HIP kernel here; only the "
                "legacy form (rel_pos_type='legacy', ESPnet's legacy_rel_pos / legacy_rel_selfattn) is implemented, and "
                "checkpoints trained with the newer form do not transfer" % (rel_pos_type,))
        if layer_drop_rate != 0.0:
            raise NotImplementedError("layer_drop_rate other than 0 (stochastic depth) is not on the HIP path")
        if interctc_layer_idx or interctc_use_conditioning:
            raise NotImplementedError("intermediate CTC (interctc_layer_idx / interctc_use_conditioning) is not on the HIP path")
        att = _REL_ALIASES.get(attention_layer_type, attention_layer_type)
        pos = _REL_ALIASES.get(pos_enc_layer_type, pos_enc_layer_type)
        if (att, pos) == ("selfattn", "abs_pos"):
            attn_class, pos_enc_class = M.MultiHeadedAttention, M.PositionalEncoding
        elif (att, pos) == ("rel_selfattn", "rel_pos"):
            attn_class, pos_enc_class = M.RelPositionMultiHeadedAttention, M.RelPositionalEncoding
        else:
            raise NotImplementedError("attention_layer_type=%r with pos_enc_layer_type=%r: (selfattn, abs_pos) and "
                                      "(rel_selfattn, rel_pos) are on the HIP path" % (attention_layer_type, pos_enc_layer_type))
        pos_enc = pos_enc_class(attention_dim, positional_dropout_rate)
        conv2d = {"conv2d": M.Conv2dSubsampling, "conv2d6": M.Conv2dSubsampling6, "conv2d8": M.Conv2dSubsampling8}
        if input_layer in conv2d:
            self.embed = conv2d[input_layer](idim, attention_dim, dropout_rate, pos_enc)
        elif input_layer == "linear":
            self.embed = _LinearInput(idim, attention_dim, dropout_rate, pos_enc)
        else:
            raise NotImplementedError("input_layer=%r: conv2d / conv2d6 / conv2d8 / linear are on the HIP path" % (input_layer,))

        def pw():
            return M.positionwise_layer(positionwise_layer_type, attention_dim, linear_units, dropout_rate, 3,
                                        M.get_activation(ffn_activation_type))
        self.encoders = M.repeat(
            num_blocks,
            lambda lnum: EBranchformerEncoderLayer(
                attention_dim, attn_class(attention_heads, attention_dim, attention_dropout_rate),
                ConvolutionalGatingMLP(attention_dim, cgmlp_linear_units, cgmlp_conv_kernel, dropout_rate,
                                       use_linear_after_conv, gate_activation),
                pw() if use_ffn else None, pw() if use_ffn and macaron_ffn else None, dropout_rate, merge_conv_kernel))
        self.after_norm = M.LayerNorm(attention_dim)

    def forward(self, xs, masks):
        if isinstance(self.embed, M.Conv2dSubsampling):
            xs, masks = self.embed(xs, masks)
        else:
            xs = self.embed(xs)
        xs, masks = self.encoders(xs, masks)
        if isinstance(xs, tuple):
            xs = xs[0]
        return self.after_norm(xs), masks
