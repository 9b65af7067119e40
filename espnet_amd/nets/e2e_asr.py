"""espnet1 RNN model surface: VGG-BLSTM(P) encoder + location-aware attention LSTM decoder + CTC on the
espnet_amd HIP kernels.

Plug-in slot: ``--model-module espnet_amd.nets.e2e_asr:E2E``
(reference: espnet/nets/pytorch_backend/e2e_asr.py:57-338; BASELINE config 4).
"""
import math

import numpy as np
import torch

from .. import functional as F_
from .. import ops
from .asr_interface import ASRInterface
from .frontends.feature_transform import feature_transform_for
from .frontends.frontend import frontend_for
from .modules import CTC
from .rnn.attentions import att_for
from .rnn.decoders import decoder_for
from .rnn.encoders import encoder_for

CTC_LOSS_THRESHOLD = 10000  # reference: e2e_asr.py:43


def get_subsample(train_args, mode, arch):
    """reference: nets_utils.py:390-468 (asr / rnn and rnn-t arches; transformer -> [1])"""
    if arch == "transformer":
        return np.array([1])
    if mode == "asr" and arch in ("rnn", "rnn-t"):
        subsample = np.ones(train_args.elayers + 1, dtype=np.int64)
        if train_args.etype.endswith("p") and not train_args.etype.startswith("vgg"):
            ss = train_args.subsample.split("_")
            for j in range(min(train_args.elayers + 1, len(ss))):
                subsample[j] = int(ss[j])
        return subsample
    raise ValueError("Invalid options: mode={}, arch={}".format(mode, arch))


def lecun_normal_init_parameters(module):
    """reference: espnet/nets/pytorch_backend/initialization.py:14-34"""
    for p in module.parameters():
        data = p.data
        if data.dim() == 1:
            data.zero_()
        elif data.dim() == 2:
            data.normal_(0, 1.0 / math.sqrt(data.size(1)))
        elif data.dim() in (3, 4):
            n = data.size(1)
            for k in data.size()[2:]:
                n *= k
            data.normal_(0, 1.0 / math.sqrt(n))
        else:
            raise NotImplementedError


def set_forget_bias_to_one(bias):
    """reference: initialization.py:49-54"""
    n = bias.size(0)
    bias.data[n // 4: n // 2].fill_(1.0)


def to_spectrum(x, device=None):
    """the input forms of a frontend model (what the reference's to_torch_tensor accepts) -> float32 with a trailing
    (re, im) axis: a complex tensor or numpy array, a dict with "real" and "imag", or a float tensor that already carries
    the axis"""
    if isinstance(x, dict):
        if "real" not in x or "imag" not in x:
            raise ValueError("has 'real' and 'imag' keys: {}".format(list(x)))
        x = torch.stack([torch.as_tensor(x["real"]), torch.as_tensor(x["imag"])], dim=-1)
    elif isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    if not torch.is_tensor(x):
        raise ValueError("a frontend model takes a complex spectrum (tensor, numpy array or real/imag dict), not %r" % type(x))
    if x.is_complex():
        x = torch.view_as_real(x.resolve_conj())
    elif x.size(-1) != 2:
        raise ValueError("a real tensor must carry the trailing (re, im) axis, got shape {}".format(tuple(x.shape)))
    x = x.to(torch.float32)
    return x.contiguous() if device is None else x.to(device).contiguous()


class E2E(ASRInterface, torch.nn.Module):
    """reference: e2e_asr.py:57-338 (single encoder; use_frontend: the MVDR beamformer and the espnet1 feature transform
    in front of it, trained from the ASR loss)"""

    def __init__(self, idim, odim, args):
        torch.nn.Module.__init__(self)
        self.mtlalpha = args.mtlalpha
        assert 0.0 <= self.mtlalpha <= 1.0, "mtlalpha should be [0.0, 1.0]"
        self.etype = args.etype
        self.verbose = args.verbose
        args.char_list = getattr(args, "char_list", None)
        self.char_list = args.char_list
        self.outdir = args.outdir
        self.space = args.sym_space
        self.blank = args.sym_blank
        self.sos = odim - 1
        self.eos = odim - 1
        self.subsample = get_subsample(args, mode="asr", arch="rnn")
        if getattr(args, "lsm_type", ""):
            raise NotImplementedError("unigram label smoothing needs the training json (out of the hot-path scope)")
        if getattr(args, "use_frontend", False):      # e2e_asr.py:141-146: idim counts the bins of the spectrum
            self.frontend = frontend_for(args, idim)
            self.feature_transform = feature_transform_for(args, (idim - 1) * 2)
            idim = args.n_mels
        else:
            self.frontend = None
        self.enc = encoder_for(args, idim, self.subsample)
        self.ctc = CTC(odim, args.eprojs, args.dropout_rate, ctc_type=args.ctc_type)
        self.att = att_for(args)
        self.dec = decoder_for(args, odim, self.sos, self.eos, self.att, None)
        self.init_like_chainer()
        # options for the validation beam search (reference: e2e_asr.py:160-180)
        self.report_cer = bool(getattr(args, "report_cer", False))
        self.report_wer = bool(getattr(args, "report_wer", False))
        if self.report_cer or self.report_wer:
            import argparse
            self.recog_args = argparse.Namespace(
                beam_size=args.beam_size, penalty=args.penalty, ctc_weight=args.ctc_weight, maxlenratio=args.maxlenratio,
                minlenratio=args.minlenratio, lm_weight=args.lm_weight, rnnlm=args.rnnlm, nbest=args.nbest,
                space=args.sym_space, blank=args.sym_blank)
        self.error_calculator = None
        if self.char_list is not None and (self.mtlalpha != 0 or self.report_cer or self.report_wer):
            from .e2e_asr_common import ErrorCalculator
            self.error_calculator = ErrorCalculator(self.char_list, self.space, self.blank, self.report_cer, self.report_wer)
        self._cer_ctc_n = self._cer_n = self._wer_n = None
        self.rnnlm = None
        self.logzero = -10000000000.0
        self.loss = None
        self.acc = None

    def init_like_chainer(self):
        """reference: e2e_asr.py:187-203"""
        lecun_normal_init_parameters(self)
        self.dec.embed.weight.data.normal_(0, 1)
        for i in range(len(self.dec.decoder)):
            set_forget_bias_to_one(self.dec.decoder[i].bias_ih)

    def _features(self, xs_pad, ilens):
        """frontend -> feature transform (e2e_asr.py:215-217): a spectrum [B,T,C,F] in any form to_spectrum takes ->
        (log-mel features on the parameters' device, lengths).  In training the frontend draws on the host per call
        (pass-through or beamformer, then the channel), so such a step runs eagerly: a captured and replayed graph would
        freeze the draw."""
        dev = next(self.parameters()).device
        if self.training and dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a training step with a frontend draws on the host at every call: run it eagerly, a captured "
                               "graph would replay one frozen draw")
        xs_pad = to_spectrum(xs_pad, dev)
        hs_pad, hlens, _ = self.frontend(xs_pad, ilens)
        return self.feature_transform(hs_pad, hlens)

    def forward(self, xs_pad, ilens, ys_pad):
        """xs_pad (B,Tmax,idim), ilens (B), ys_pad (B,Lmax) -> loss (e2e_asr.py:205-338)"""
        if self.frontend is not None:
            xs_pad, ilens = self._features(xs_pad, ilens)
        if xs_pad.is_cuda:
            if self.training and torch.is_grad_enabled():
                ops.zero_arena_begin(xs_pad.device)      # the decoder loop's zero-filled buffers: one fill per step
            else:
                ops.zero_arena_off()
        hs_pad, hlens, _ = self.enc(xs_pad, ilens)
        self.hs_pad, self.hlens = hs_pad, hlens
        self.loss_ctc = None if self.mtlalpha == 0 else self.ctc(hs_pad, hlens, ys_pad)
        if self.mtlalpha == 1:
            self.loss_att, acc = None, None
        else:
            self.loss_att, acc, _ = self.dec(hs_pad, hlens, ys_pad)
        self.acc = acc
        self._score(hs_pad, hlens, ys_pad)
        alpha = self.mtlalpha
        if alpha == 0:
            self.loss = self.loss_att
        elif alpha == 1:
            self.loss = self.loss_ctc
        else:
            self.loss = F_.WeightedSumFn.apply(self.loss_ctc, self.loss_att, alpha)
        return self.loss

    def _score(self, hs_pad, hlens, ys_pad):
        """per-utterance error counts of this batch as device tensors (reference: e2e_asr.py:237-315); the rates are the
        properties cer_ctc / cer / wer, which read them when asked"""
        self._cer_ctc_n = self._cer_n = self._wer_n = None
        ec = self.error_calculator
        if ec is None:
            return
        with torch.no_grad():
            ys_dev = ys_pad if ys_pad.is_cuda else ops.h2d_async(ys_pad, hs_pad.device)
            if self.mtlalpha != 0:          # greedy CTC, in training too
                self._cer_ctc_n = ec.counts_ctc_text(self.ctc.argmax(hs_pad), ys_dev)
            if self.training or not (self.report_cer or self.report_wer):
                return
            lpz = self.ctc.log_softmax(hs_pad) if self.recog_args.ctc_weight > 0.0 else None
            nbest_hyps = self.dec.recognize_beam_batch(hs_pad, hlens, lpz, self.recog_args, self.char_list, self.rnnlm)
            y_hats = [nbest_hyp[0]["yseq"][1:-1] for nbest_hyp in nbest_hyps]      # without <sos> and <eos>
            host = torch.full((len(y_hats), max(1, max(len(y) for y in y_hats))), -1, dtype=torch.int32)
            for b, y in enumerate(y_hats):
                host[b, : len(y)] = torch.tensor([int(v) for v in y], dtype=torch.int32)
            ys_hat = ops.h2d_async(host, hs_pad.device)
            # the whole hypothesis is scored (no ymax): a reference row without padding, as wide as the hypotheses, lifts it
            t = ec._tables_on(ys_hat.device)
            ref = ys_dev.to(torch.int32).contiguous()
            if self.report_cer:
                h, hn = ec._units(ys_hat, t["hyp"], drop_cp=0x20)
                r, rn = ec._units(ref, t["ref"], drop_cp=0x20)
                self._cer_n = (ops.edit_distance(h, hn, r, rn), rn)
            if self.report_wer:
                h, hn = ec._units(ys_hat, t["hyp"], mode=ops.TEXT_WORDS)
                r, rn = ec._units(ref, t["ref"], mode=ops.TEXT_WORDS)
                self._wer_n = (ops.edit_distance(h, hn, r, rn), rn)

    @property
    def cer_ctc(self):
        """mean over the utterances with a non-empty reference of errors / reference length (e2e_asr.py:258-263); None when
        there is none or CTC / the token list is absent.  One host read of the 2B counts, Python arithmetic as the reference."""
        if self._cer_ctc_n is None:
            return None
        eds, lens = torch.stack(self._cer_ctc_n).tolist()
        cers = [e / n for e, n in zip(eds, lens) if n > 0]
        return sum(cers) / len(cers) if cers else None

    @property
    def cer(self):
        """float(sum errors) / sum lengths of the validation beam search's 1-best; 0.0 in training or without --report-cer"""
        if self._cer_n is None:
            return 0.0
        (e, n), = self.error_calculator.sums(self._cer_n)
        return float(e) / n

    @property
    def wer(self):
        if self._wer_n is None:
            return 0.0
        (e, n), = self.error_calculator.sums(self._wer_n)
        return float(e) / n

    def scorers(self):
        from .ctc_prefix_score import CTCPrefixScorer
        return dict(decoder=self.dec, ctc=CTCPrefixScorer(self.ctc, self.eos))

    def encode(self, x):
        """x ndarray (T, D) -> encoder states (T', eprojs) (e2e_asr.py:344-369)"""
        self.eval()
        ops.zero_arena_off()                    # recognition: no slices of a training step's zero arena
        p = next(self.parameters())
        with torch.no_grad():
            if self.frontend is not None:
                x = to_spectrum(x)
                h, hlens = self._features(x.unsqueeze(0), [x.shape[0]])
            else:
                h, hlens = torch.as_tensor(x, device=p.device, dtype=p.dtype).unsqueeze(0), [x.shape[0]]
            hs, _, _ = self.enc(h, hlens)
        return hs.squeeze(0)

    @ops.inference_call
    def recognize_batch(self, xs, recog_args, char_list=None, rnnlm=None, ctc_scoring_num=None):
        """xs list of ndarrays (T_b, D) -> per utterance an n-best list (e2e_asr.py:394-445 -> Decoder.recognize_beam_batch)"""
        self.eval()
        ops.zero_arena_off()
        p = next(self.parameters())
        if self.frontend is not None:
            feats = [to_spectrum(x, p.device) for x in xs]
        else:
            feats = [torch.as_tensor(x, device=p.device, dtype=p.dtype) for x in xs]
        ilens = [int(x.shape[0]) for x in feats]
        xs_pad = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
        with torch.no_grad():
            if self.frontend is not None:
                xs_pad, ilens = self._features(xs_pad, ilens)
            hs_pad, hlens, _ = self.enc(xs_pad, ilens)
            if recog_args.ctc_weight > 0.0:
                lpz, normalize = self.ctc.log_softmax(hs_pad), False
            else:
                lpz, normalize = None, True
            return self.dec.recognize_beam_batch(hs_pad, hlens, lpz, recog_args, char_list, rnnlm, normalize_score=normalize,
                                                 ctc_scoring_num=ctc_scoring_num)

    @ops.inference_call
    def enhance(self, xs):
        """xs list of spectra (T_b, C, F) -> (enhanced (B,T,F,2), speech mask (B,T,C,F), ilens) as numpy arrays
        (e2e_asr.py:447-470; the model's training mode is restored)"""
        if self.frontend is None:
            raise RuntimeError("Frontend does't exist")
        prev = self.training
        self.eval()
        p = next(self.parameters())
        xs = [to_spectrum(x, p.device) for x in xs]
        ilens = np.fromiter((x.shape[0] for x in xs), dtype=np.int64)
        xs_pad = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True)
        with torch.no_grad():
            enhanced, _, mask = self.frontend(xs_pad, ilens)
        if prev:
            self.train()
        return enhanced.cpu().numpy(), None if mask is None else mask.cpu().numpy(), ilens

    @ops.inference_call
    def recognize(self, x, recog_args, char_list=None, rnnlm=None):
        """x ndarray (T, D) -> n-best list of {"score", "yseq"} (e2e_asr.py:372-392)"""
        hs = self.encode(x).unsqueeze(0)
        lpz = self.ctc.log_softmax(hs)[0] if recog_args.ctc_weight > 0.0 else None
        return self.dec.recognize_beam(hs[0], lpz, recog_args, char_list, rnnlm)
