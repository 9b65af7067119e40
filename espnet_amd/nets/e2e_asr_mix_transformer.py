"""espnet1 model surface: multi-speaker Transformer ASR (single-channel mixtures) on the HIP kernels.

Plug-in slot: ``--model-module espnet_amd.nets.e2e_asr_mix_transformer:E2E``
(reference: espnet/nets/pytorch_backend/e2e_asr_mix_transformer.py:42-462, transformer/encoder_mix.py:20-128,
e2e_asr_mix.py:48-166 for PIT and the encoder option).

The encoder has three stages: the input layer (Enc_mix), one stack of `elayers_sd` layers per speaker (Enc_SD) and the shared
stack of `elayers` layers (Enc_rec).  The shared stack runs once on the S B rows of all speakers.  Training runs the
permutation-invariant CTC in one eamd_ctc_pit_loss call, permutes the labels on the device with a gather, runs one decoder pass
over the S B rows and weights the per-speaker attention losses and accuracies by the permuted label lengths, as the reference
does.  Nothing in forward_core() waits for the host.

Departures from the reference:
  - dropout in front of the CTC output layer draws one mask per speaker; the reference draws one for each of its S^2 CTC calls
    (identical at dropout 0);
  - the reference logs float(loss_ctc) inside forward, a host synchronisation; it is dropped (sync_report still reports the
    losses as the Transformer E2E does).
"""
import numpy as np
import torch

from .. import functional as F_
from .. import ops
from .e2e_asr_transformer import E2E as E2ETransformer
from .modules import (CTC, MultiHeadedAttention, TransformerEncoder, TransformerEncoderLayer, positionwise_layer, repeat,
                      subsequent_mask)


def pit_permutations(num_spkrs):
    """reference: PIT.permutationDFS (e2e_asr_mix.py:110-128): the swap-based depth-first order, not lexicographic"""
    out = []

    def dfs(src, start):
        if start == len(src) - 1:
            out.append(list(src))
        for i in range(start, len(src)):
            src[start], src[i] = src[i], src[start]
            dfs(src, start + 1)
            src[start], src[i] = src[i], src[start]
    dfs(list(range(num_spkrs)), 0)
    return out


class EncoderMix(TransformerEncoder):
    """reference: transformer/encoder_mix.py:20-128 (state_dict: embed.*, encoders_sd.{s}.{l}.*, encoders.{l}.*, after_norm.*)"""

    def __init__(self, idim, attention_dim=256, attention_heads=4, linear_units=2048, num_blocks_sd=4, num_blocks_rec=8,
                 dropout_rate=0.1, positional_dropout_rate=0.1, attention_dropout_rate=0.0, input_layer="conv2d",
                 normalize_before=True, concat_after=False, positionwise_layer_type="linear", positionwise_conv_kernel_size=1,
                 padding_idx=-1, num_spkrs=2):
        super().__init__(idim, attention_dim=attention_dim, attention_heads=attention_heads, linear_units=linear_units,
                         num_blocks=num_blocks_rec, dropout_rate=dropout_rate, positional_dropout_rate=positional_dropout_rate,
                         attention_dropout_rate=attention_dropout_rate, input_layer=input_layer,
                         normalize_before=normalize_before, concat_after=concat_after,
                         positionwise_layer_type=positionwise_layer_type,
                         positionwise_conv_kernel_size=positionwise_conv_kernel_size, padding_idx=padding_idx)
        self.num_spkrs = num_spkrs
        self.encoders_sd = torch.nn.ModuleList([
            repeat(num_blocks_sd, lambda lnum: TransformerEncoderLayer(
                attention_dim, MultiHeadedAttention(attention_heads, attention_dim, attention_dropout_rate),
                positionwise_layer(positionwise_layer_type, attention_dim, linear_units, dropout_rate,
                                   positionwise_conv_kernel_size), dropout_rate, normalize_before, concat_after))
            for _ in range(num_spkrs)])

    def forward_stacked(self, xs, masks):
        """-> (hs (S B, T', D): speaker-major rows, masks (S B, 1, T') or None).  The per-speaker stacks run on the input
        layer's output; the shared stack and the final LayerNorm run once on the S B rows (its weights are shared)."""
        xs, masks = self._embed(xs, masks)
        S = self.num_spkrs
        xs = torch.cat([self.encoders_sd[ns](xs, masks)[0] for ns in range(S)], 0)
        masks = None if masks is None else masks.repeat(S, 1, 1)
        xs, masks = self.encoders(xs, masks)
        if self.normalize_before:
            xs = self.after_norm(xs)
        return xs, masks

    def forward(self, xs, masks):
        """reference: encoder_mix.py:104-128 -> (list of S (B, T', D), list of S masks)"""
        B = xs.shape[0]
        hs, m = self.forward_stacked(xs, masks)
        S = self.num_spkrs
        masks = [None] * S if m is None else list(m.view(S, B, *m.shape[1:]).unbind(0))
        return list(hs.view(S, B, *hs.shape[1:]).unbind(0)), masks


class E2E(E2ETransformer):
    """E2E module (reference: e2e_asr_mix_transformer.py:42-462)."""

    @staticmethod
    def add_arguments(parser):
        E2ETransformer.add_arguments(parser)
        E2E.encoder_mix_add_arguments(parser)
        return parser

    @staticmethod
    def encoder_mix_add_arguments(parser):
        """reference: e2e_asr_mix.py:149-166 (without --spa, which only the RNN mixture model reads)"""
        group = parser.add_argument_group("E2E encoder setting for multi-speaker")
        group.add_argument("--elayers-sd", default=4, type=int,
                           help="Number of speaker differentiate encoder layers for multi-speaker speech recognition task.")
        return parser

    reports_errors = False     # error_calculator stays None here (CER / WER reporting)

    def __init__(self, idim, odim, args, ignore_id=-1):
        from .e2e_asr_transformer import fill_missing_args
        super().__init__(idim, odim, args, ignore_id)
        args = fill_missing_args(args, self.add_arguments)
        if args.transformer_attn_dropout_rate is None:
            args.transformer_attn_dropout_rate = args.dropout_rate
        self.num_spkrs = int(getattr(args, "num_spkrs", 2))
        # built after the Transformer E2E's modules and in their slots, as the reference does (same names, same init order)
        self.encoder = EncoderMix(
            idim=idim, attention_dim=args.adim, attention_heads=args.aheads, linear_units=args.eunits,
            num_blocks_sd=args.elayers_sd, num_blocks_rec=args.elayers, input_layer=args.transformer_input_layer,
            dropout_rate=args.dropout_rate, positional_dropout_rate=args.dropout_rate,
            attention_dropout_rate=args.transformer_attn_dropout_rate, num_spkrs=self.num_spkrs)
        if args.mtlalpha > 0.0:
            self.ctc = CTC(odim, args.adim, args.dropout_rate, ctc_type=args.ctc_type, reduce=False)
        else:
            self.ctc = None
        self.pit_record = {}          # nll_pair [B, S, S] and pit [B] of the last training forward (device tensors)
        self.min_perm = None          # perm [B, S] of the last training forward (device)
        self._mix_L = None

    # ---- training forward ---------------------------------------------------------------------------------------------
    def prepare(self, xs_pad, ilens, ys_pad, pad_to=None):
        """Transformer E2E prepare() on labels ys_pad (B, S, L) padded with ignore_id (asr_mix.py:112-121).  pad_to = (T, L):
        frames and every speaker's labels padded to these sizes (train.BucketedGraphStep passes L = the longest label of any
        speaker).  The labels travel as (B, S L) rows; forward_core() views them as (B, S, L)."""
        ys_pad = torch.as_tensor(ys_pad)
        B, S, L = ys_pad.shape
        assert S == self.num_spkrs, (S, self.num_spkrs)
        if pad_to is not None:
            Tb, Lb = pad_to
            yp = ys_pad.new_full((B, S, Lb), self.ignore_id)
            n = min(Lb, L)
            yp[:, :, :n] = ys_pad[:, :, :n]
            ys_pad, L, pad_to = yp, Lb, (Tb, S * Lb)
        self._mix_L = L
        try:
            return super().prepare(xs_pad, ilens, ys_pad.reshape(B, S * L), pad_to=pad_to)
        finally:
            self._mix_L = None

    def decoder_inputs(self, ys_host, ys_pad, dev):
        """the causal mask of the decoder's S B rows (the labels themselves are permuted on the device in forward_core)"""
        S, U = self.num_spkrs, self._mix_L + 1
        ys_mask = subsequent_mask(U).unsqueeze(0).expand(S * ys_pad.size(0), U, U).to(torch.uint8).contiguous()
        return dict(ys_mask=ops.h2d_async(ys_mask, dev))

    def forward_core(self, batch):
        """Kernel-only part of forward (reference: e2e_asr_mix_transformer.py:89-214): no host synchronisation."""
        S, B, D = self.num_spkrs, batch["B"], self.adim
        ops.set_time_bound(batch.get("tbound"))
        try:
            hs, hs_mask = self.encoder.forward_stacked(batch["xs_pad"], batch["src_mask"])
        finally:
            ops.set_time_bound(None)
        self.hs_pad = hs
        if hs_mask is not None and not hs_mask.is_contiguous():
            hs_mask = hs_mask.contiguous()
        ys = batch["ys_pad"].view(B, S, -1)
        L = ys.shape[2]
        assert self.mtlalpha > 0.0
        loss_ctc, perm = self.ctc.pit_loss(hs.view(S, B, -1, D), batch["hs_len"], ys, record=self.pit_record)
        self.min_perm = perm
        # permuted labels, speaker-major rows like the encoder output: ys_perm[i, b] = ys[b, perm[b, i]] (:129-131)
        ys_perm = torch.gather(ys, 1, perm.unsqueeze(-1).expand(B, S, L)).transpose(0, 1).reshape(S * B, L).contiguous()
        loss_att = None
        self._acc_t = None
        if self.decoder is not None:
            ys_in, ys_out, _ = ops.add_sos_eos(ys_perm, self.sos, self.eos, self.ignore_id)
            pred_pad, _ = self.decoder(ys_in, batch["ys_mask"], hs, hs_mask)
            self.pred_pad = pred_pad
            n_lab = (ys_perm != self.ignore_id).view(S, B * L).sum(1).float()        # ys_out_len (:133-135)
            n_out = (ys_out != self.ignore_id).view(S, -1).sum(1).float()          # tokens + <eos> of each speaker
            denom = n_out if self.criterion.normalize_length else torch.full_like(n_out, float(B))
            loss_att, correct = _MixLabelSmoothingFn.apply(pred_pad, ys_out, self.criterion.smoothing, self.ignore_id,
                                                           n_lab / (denom * n_lab.sum()))
            self._acc_t = (correct / n_out * n_lab).sum() / n_lab.sum()            # (:160-180)
        alpha = self.mtlalpha
        if alpha == 1:
            self.loss = loss_ctc
        else:
            self.loss = F_.WeightedSumFn.apply(loss_ctc, loss_att, alpha)
        self._loss_ctc_t, self._loss_att_t = loss_ctc, loss_att
        return self.loss

    # ---- inference ----------------------------------------------------------------------------------------------------
    def encode(self, x):
        """x: (T, idim) -> list of the S speakers' (T', adim) encoder outputs (e2e_asr_mix_transformer.py:222-232)"""
        self.eval()
        dev = next(self.parameters()).device
        x = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x, dtype=torch.float32)
        with torch.no_grad():
            hs, _ = self.encoder(x.to(dev).unsqueeze(0), None)
        return [h.squeeze(0) for h in hs]

    @ops.inference_call
    def recognize(self, x, recog_args, char_list=None, rnnlm=None, use_jit=False, ngram=None):
        """reference: e2e_asr_mix_transformer.py:438-462 -> one n-best list per speaker (the reference's recog for each)"""
        from .beam_search import recognize_beam
        return [recognize_beam(self, h, recog_args, char_list, rnnlm, ngram=ngram) for h in self.encode(x)]

    @ops.inference_call
    def recognize_batch(self, xs, recog_args, char_list=None, rnnlm=None, ngram=None):
        """xs: list of (T_b, idim) features -> [B][S] n-best lists, each what recognize() gives for that utterance: the padded batch
        is encoded once (every utterance keeps its single-utterance encoder output, nets.ctc_align.encode_batch(alone=True)) and
        the S B searches run in one BeamSearch.forward_batch"""
        from .beam_search import recognize_beam_batch
        from .ctc_align import encode_batch
        xs = [torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x, dtype=torch.float32) for x in xs]
        ilens = [int(x.shape[0]) for x in xs]
        xs_pad = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True)
        hs, hl = encode_batch(self, xs_pad, ilens, alone=True)
        S = self.num_spkrs
        encs = [hs[s][b, :hl[b]] for b in range(len(xs)) for s in range(S)]
        out = recognize_beam_batch(self, encs, recog_args, char_list, rnnlm, ngram=ngram)
        return [out[b * S:(b + 1) * S] for b in range(len(xs))]


class _MixLabelSmoothingFn(torch.autograd.Function):
    """sum_i w[i] * (label-smoothing loss sum over speaker i's rows) for the S speaker-major row blocks of one decoder pass
    (reference: the per-speaker criterion calls and their length-weighted mean, e2e_asr_mix_transformer.py:160-180) ->
    (loss, correct [S] = argmax-correct rows per speaker).  w [S] is a device tensor: no host synchronisation."""

    @staticmethod
    def forward(ctx, logits, target, smoothing, ignore_id, w):
        S = w.numel()
        V = logits.shape[-1]
        loss_rows, correct, grad = ops.lsm_loss(logits.reshape(-1, V).contiguous(), target.reshape(-1).contiguous(), smoothing,
                                                1.0, ignore_id, want_grad=logits.requires_grad)
        ctx.save_for_backward(grad, w)
        ctx.shp = logits.shape
        correct = correct.view(S, -1).sum(1)
        ctx.mark_non_differentiable(correct)
        return (loss_rows.view(S, -1).sum(1) * w).sum(), correct

    @staticmethod
    def backward(ctx, g, _gc):
        grad, w = ctx.saved_tensors
        S = w.numel()
        gs = (w * g).contiguous()
        gv = grad.view(S, -1)
        for i in range(S):       # speaker-major rows: one scale per contiguous block
            ops.scale_dev(gv[i], gs[i:i + 1], 1.0, out=gv[i])
        return grad.view(ctx.shp), None, None, None, None
