"""espnet1 model surface: Mask-CTC non-autoregressive ASR on the HIP kernels.

Plug-in slot: ``--model-module espnet_amd.nets.e2e_asr_maskctc:E2E``
(reference: espnet/nets/pytorch_backend/e2e_asr_maskctc.py:31-249, maskctc/add_mask_token.py:13-39, maskctc/mask.py:11-28).

Training is the Transformer E2E's prepare() / forward_core() split with one more output class (<mask>) and the decoder fed the
masked labels under a padding-only square mask.  Decoding runs a whole padded batch on the device: the CTC seed
(eamd_maskctc_seed), then a fixed number of decoder passes, each followed by eamd_maskctc_update; the host reads the device twice
per batch (the lengths / pass counts after the seed, the hypotheses at the end).

Departure from the reference: with --maskctc-use-conformer-encoder and no --transformer-attn-dropout-rate the reference reads
args.conformer_dropout_rate, which no parser defines; the attention dropout rate falls back to --dropout-rate instead, as in the
Transformer and Conformer E2E.
"""
import numpy as np
import torch

from .. import ops
from .ctc_align import encode_batch
from .e2e_asr_conformer import E2E as E2EConformer
from .e2e_asr_conformer import add_arguments_conformer_common
from .e2e_asr_transformer import E2E as E2ETransformer
from .e2e_asr_transformer import strtobool
from .modules import make_non_pad_mask


def mask_uniform(ys_pad, mask_token, eos, ignore_id):
    """reference: maskctc/add_mask_token.py:13-39, on the host.  ys_pad (B, L) labels padded with ignore_id (tensor or array)
    -> (ys_in, ys_out) int64 CPU tensors (B, Lmax), Lmax the longest label sequence.  For each utterance in batch order, from the
    global numpy RNG: n = randint(1, len + 1), then n positions drawn WITH replacement (choice(len, n)); ys_in has <mask> there
    and is padded with eos, ys_out has the label there and ignore_id elsewhere."""
    ys_pad = ys_pad.cpu().numpy() if isinstance(ys_pad, torch.Tensor) else np.asarray(ys_pad)
    ys = [y[y != ignore_id] for y in ys_pad]
    Lmax = max(len(y) for y in ys)
    ys_in = np.full((len(ys), Lmax), eos, np.int64)
    ys_out = np.full((len(ys), Lmax), ignore_id, np.int64)
    for i, y in enumerate(ys):
        n = np.random.randint(1, len(y) + 1)
        idx = np.random.choice(len(y), n)
        ys_in[i, :len(y)] = y
        ys_in[i, idx] = mask_token
        ys_out[i, idx] = y[idx]
    return torch.from_numpy(ys_in), torch.from_numpy(ys_out)


def square_mask(ys_in_pad, pad_id):
    """reference: maskctc/mask.py:11-28.  (B, L) -> (B, L, L) bool: query and key both not padding"""
    m = ys_in_pad != pad_id
    return m.unsqueeze(-1) & m.unsqueeze(-2)


def length_square_mask(lens, L):
    """(B, L, L) bool mask of positions < lens[b] on both axes (square_mask of a batch padded after lens[b] tokens)"""
    m = make_non_pad_mask(lens, L) if L > 0 else torch.zeros(len(lens), 0, dtype=torch.bool)
    return m.unsqueeze(-1) & m.unsqueeze(-2)


class E2E(E2ETransformer):
    """E2E module (reference: e2e_asr_maskctc.py:31-249)."""

    @staticmethod
    def add_arguments(parser):
        E2ETransformer.add_arguments(parser)
        E2E.add_maskctc_arguments(parser)
        return parser

    @staticmethod
    def add_maskctc_arguments(parser):
        group = parser.add_argument_group("maskctc specific setting")
        group.add_argument("--maskctc-use-conformer-encoder", default=False, type=strtobool)
        add_arguments_conformer_common(group)
        return parser

    def _build_encoder(self, idim, args):
        if args.maskctc_use_conformer_encoder:
            return E2EConformer._build_encoder(self, idim, args)
        return E2ETransformer._build_encoder(self, idim, args)

    reports_errors = False     # error_calculator stays None here (CER / WER reporting)

    def __init__(self, idim, odim, args, ignore_id=-1):
        odim += 1  # for the mask token
        super().__init__(idim, odim, args, ignore_id)
        assert 0.0 <= self.mtlalpha < 1.0, "mtlalpha should be [0.0, 1.0)"
        self.mask_token = odim - 1
        self.sos = odim - 2
        self.eos = odim - 2
        self.odim = odim
        self._padded = False     # prepare() is building a batch padded to a bucket
        self.host_reads = 0      # blocking device-to-host reads of the last maskctc_decode_batch + its caller
        if getattr(args, "maskctc_use_conformer_encoder", False):
            self.reset_parameters(args)      # the reference initialises a second time after building the Conformer

    # ---- training forward ---------------------------------------------------------------------------------------------
    def decoder_inputs(self, ys_host, ys_pad, dev):
        """reference: e2e_asr_maskctc.py:121-125.  The masking draws run on the host (global numpy RNG, batch order); with
        prepare(pad_to=) the label axis is padded further (ys_in with eos, ys_out with ignore_id), which the square mask hides."""
        ys_in, ys_out = mask_uniform(ys_host, self.mask_token, self.eos, self.ignore_id)
        L = ys_pad.size(1) if self._padded else ys_in.shape[1]
        if L > ys_in.shape[1]:
            B, n = ys_in.shape
            ys_in = torch.cat([ys_in, ys_in.new_full((B, L - n), self.eos)], 1)
            ys_out = torch.cat([ys_out, ys_out.new_full((B, L - n), self.ignore_id)], 1)
        ys_mask = square_mask(ys_in, self.eos).to(torch.uint8)
        n_valid = torch.tensor(int((ys_out != self.ignore_id).sum()), dtype=torch.int64)
        return dict(ys_in_pad=ops.h2d_async(ys_in, dev), ys_out_pad=ops.h2d_async(ys_out, dev),
                    ys_mask=ops.h2d_async(ys_mask, dev), n_valid=ops.h2d_async(n_valid, dev))

    def prepare(self, xs_pad, ilens, ys_pad, pad_to=None):
        """Transformer E2E prepare() with the Mask-CTC decoder inputs (decoder_inputs); forward_core() is the Transformer's:
        decoder on (ys_in, square mask, encoder output), label-smoothing loss and accuracy on the masked positions, CTC on the
        original labels, alpha * ctc + (1 - alpha) * att."""
        self._padded = pad_to is not None
        try:
            return super().prepare(xs_pad, ilens, ys_pad, pad_to=pad_to)
        finally:
            self._padded = False

    # ---- inference ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def maskctc_decode_batch(self, xs_pad, ilens, thr=0.999, K=10):
        """Mask-CTC decoding of a padded batch (reference: e2e_asr_maskctc.py:180-249 per utterance).  xs_pad (B, T, idim),
        ilens (B) -> (y [B, Lmax] int64, len [B] int32) device tensors: hypothesis b is y[b, :len[b]] (without sos / eos).
        thr: --maskctc-probability-threshold, K: --maskctc-n-iterations.  One blocking host read (lengths and pass counts)."""
        hs, hl = encode_batch(self, xs_pad, ilens, alone=True)
        was_training = self.training
        self.eval()
        try:
            B, T, _ = hs.shape
            dev = hs.device
            hl_d = ops.h2d_async(torch.tensor(hl, dtype=torch.int32), dev)
            logits = self.ctc.logits(hs).contiguous()
            seed = ops.maskctc_seed(logits, hl_d, thr, K, self.mask_token, self.eos, self.blank, Lcap=max(1, max(hl)))
            info = torch.stack([seed["len"], seed["niter"]]).cpu()
            self.host_reads = 1
            lens, nit = info[0].tolist(), info[1].tolist()
            Lmax, Nmax = max(lens), max(nit)
            y = seed["y_in"][:, :Lmax].contiguous()
            if Nmax > 0:
                tgt_mask = ops.h2d_async(length_square_mask(lens, Lmax).to(torch.uint8), dev)
                mem_mask = ops.h2d_async(make_non_pad_mask(hl, T).unsqueeze(-2).to(torch.uint8), dev)
                score = arg = None
                for p in range(Nmax):
                    pred, _ = self.decoder(y, tgt_mask, hs, mem_mask)
                    score, arg = ops.maskctc_update(p, pred.contiguous(), y, seed["len"], seed["niter"], seed["kper"],
                                                    self.mask_token, score, arg)
            return y, seed["len"]
        finally:
            self.train(was_training)

    def _hyps(self, y, lens):
        """final read: (y, len) device tensors -> one n-best list per utterance (reference: e2e_asr_maskctc.py:245-249)"""
        B, L = y.shape
        host = torch.cat([y, lens.to(torch.int64).view(B, 1)], 1).cpu()
        self.host_reads += 1
        out = []
        for b in range(B):
            n = int(host[b, L])
            out.append([{"score": 0.0, "yseq": [self.sos] + host[b, :n].tolist() + [self.eos]}])
        return out

    @ops.inference_call
    def recognize(self, x, recog_args, char_list=None, rnnlm=None):
        """reference: e2e_asr_maskctc.py:180-249.  x (T, idim); rnnlm is ignored, as in the reference."""
        x = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x, dtype=torch.float32)
        y, lens = self.maskctc_decode_batch(x.unsqueeze(0), [x.shape[0]], recog_args.maskctc_probability_threshold,
                                            recog_args.maskctc_n_iterations)
        return self._hyps(y, lens)[0]

    @ops.inference_call
    def recognize_batch(self, xs, recog_args, char_list=None, rnnlm=None):
        """xs: list of (T_i, idim) features -> list of n-best lists (one hypothesis each), as asr_recog --batchsize expects.
        With the Transformer encoder every hypothesis is the one recognize() gives; a Conformer's convolution module sees the
        padding of the shorter utterances (nets.ctc_align.encode_batch)."""
        xs = [torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x, dtype=torch.float32) for x in xs]
        ilens = [int(x.shape[0]) for x in xs]
        xs_pad = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True)
        y, lens = self.maskctc_decode_batch(xs_pad, ilens, recog_args.maskctc_probability_threshold,
                                            recog_args.maskctc_n_iterations)
        return self._hyps(y, lens)
