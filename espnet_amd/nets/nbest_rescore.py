"""Second-pass n-best rescoring: the n-best of a fast first pass (the time-synchronous CTC prefix beam search of
nets.ctc_prefix_beam) scored once, teacher-forced with all positions in parallel, by the attention decoder and / or a neural
LM, then re-ranked.  The reference has no second pass: its hybrid models decode through the label-synchronous BeamSearch
(espnet/nets/beam_search.py), a decoder step and a full-vocabulary CTC prefix score per output token, and its CTC-only path
has no way to use a neural LM.

Score of a hypothesis y = y_1 .. y_L with first-pass score s1:

    f   = ctc_weight * s1 + (1 - ctc_weight) * att + lm_weight * lm          (with a decoder)
    f   = s1 + lm_weight * lm                                                (without one)
    att = sum_{i=1..L+1} log p_dec(y_i | sos y_<i, memory),  y_{L+1} = eos;   lm = the same sum under the LM

s1 is the first-pass score as it stands.  With no n-gram and penalty = 0 it is log p_ctc(y), and f is what the reference's
BeamSearch assigns to the same ended hypothesis (its length bonus aside).  A first-pass n-gram or length term rides inside s1
and is scaled with it.

Everything stays on the device: eamd_nbest_pack builds the teacher-forcing operands, Decoder.forward_nbest / the LM's
forward_hidden give the hidden rows in front of the output Linear, eamd_gemm's row-statistics epilogue (ops.row_target_stats)
turns them into per-row (max, sum exp) tile partials and the target's logit - neither [rows, V] logits nor log-probabilities
are ever written - and eamd_nbest_rescore sums, combines and ranks.  A call makes two blocking device-to-host reads: the
longest hypothesis length (to size U) and, in rescore(), the result.
"""
import numpy as np
import torch

from .. import ops
from .modules import make_non_pad_mask


def _lm_dropout_active(lm):
    if not lm.training:
        return False
    for m in lm.modules():
        if isinstance(m, torch.nn.Dropout) and m.p > 0:
            return True
        if isinstance(m, torch.nn.RNNBase) and m.dropout > 0:
            return True
        rate = getattr(m, "dropout_rate", None)            # the attention / FFN / positional-encoding modules of nets.modules
        if isinstance(rate, (int, float)) and rate > 0:
            return True
    return False


def _lm_kind(lm):
    """-> ("transformer" | "seq_rnn" | "rnnlm", the module that owns forward_hidden, its output Linear)"""
    from ..espnet2.lm import SequentialRNNLM, TransformerLM         # here: espnet2's package imports this module
    from .lm import RNNLM, ClassifierWithState, DefaultRNNLM
    if isinstance(lm, DefaultRNNLM):
        lm = lm.model
    if isinstance(lm, TransformerLM):            # espnet2.lm.TransformerLM and its subclass nets.lm.TransformerLM
        return "transformer", lm, lm.decoder
    if isinstance(lm, SequentialRNNLM):
        return "seq_rnn", lm, lm.decoder
    if isinstance(lm, ClassifierWithState) and isinstance(lm.predictor, RNNLM):
        return "rnnlm", lm.predictor, lm.predictor.lo
    raise TypeError("n-best rescoring: a TransformerLM, SequentialRNNLM or ClassifierWithState(RNNLM), not %s" % type(lm).__name__)


def lm_output(lm):
    """the output Linear of a supported LM"""
    return _lm_kind(lm)[2]


def lm_hidden_rows(lm, ys_in):
    """the LM's teacher-forced forward on ys_in [R, U] -> (hidden rows [R*U, D] in front of its output Linear, that Linear)"""
    kind, m, lin = _lm_kind(lm)
    if kind == "transformer":
        h = m.forward_hidden(ys_in)
    elif kind == "seq_rnn":
        h = m.forward_hidden(ys_in)[0]
    else:
        state, outs = None, []
        for i in range(ys_in.shape[1]):
            state, y = m.forward_hidden(state, ys_in[:, i].contiguous())
            outs.append(y)
        h = torch.stack(outs, dim=1)
    return h.reshape(ys_in.numel(), -1), lin


class NBestRescorer:
    """decoder: a nets.modules.Decoder or None; lm: a TransformerLM (espnet2.lm / nets.lm), SequentialRNNLM, DefaultRNNLM or
    ClassifierWithState(RNNLM), or None; at least one of them.  f as in the module docstring: with a decoder
    ctc_weight in (0, 1) weighs s1 against the decoder (ctc_weight = 1 needs no decoder), without one s1 has weight 1."""

    def __init__(self, decoder=None, lm=None, ctc_weight=0.5, lm_weight=1.0, sos=None, eos=None):
        if decoder is None and lm is None:
            raise ValueError("n-best rescoring needs a decoder or a language model to rescore with")
        if sos is None or eos is None:
            raise ValueError("n-best rescoring: sos and eos ids")
        ctc_weight = float(ctc_weight)
        if decoder is not None and not 0.0 < ctc_weight < 1.0:
            raise ValueError("n-best rescoring with a decoder: 0 < ctc_weight < 1, not %r" % (ctc_weight,))
        if decoder is not None and getattr(decoder, "output_layer", None) is None:
            raise ValueError("n-best rescoring: the decoder has no output layer")
        self.decoder, self.lm, self.sos, self.eos = decoder, lm, int(sos), int(eos)
        self.w0 = ctc_weight if decoder is not None else 1.0
        self.w_dec = 1.0 - ctc_weight
        self.w_lm = float(lm_weight)
        self._padded = {}
        if lm is not None:
            lm_output(lm)              # TypeError for an LM without a teacher-forced hidden-row forward

    def _stats(self, hidden, lin, col):
        hidden, W = ops.to_act(hidden.contiguous()), ops.wshadow(lin.weight).detach()
        pad = -hidden.shape[1] % 8
        if pad:         # the row-statistics GEMM stages 16-byte groups (a 650-unit LSTM LM): zero columns add nothing to a product
            key = (id(lin), lin.weight._version, W.dtype)
            if self._padded.get("key") != key:
                self._padded = dict(key=key, W=torch.nn.functional.pad(W, (0, pad)).contiguous())
            hidden, W = torch.nn.functional.pad(hidden, (0, pad)).contiguous(), self._padded["W"]
        return ops.row_target_stats(hidden, W, None if lin.bias is None else lin.bias.detach(), col)

    @torch.no_grad()
    def rescore_device(self, memory, hlens, nbest):
        """memory [B, T', D] encoder output (None without a decoder), hlens [B] its valid frames (list or tensor), nbest int32
        [B, N, 2 + T] on the device: CTCPrefixBeamSearch.search_device's result, or built by the caller from any hypotheses and
        first-pass scores (fp32 score bits, length or -1, tokens in [1, V - 2]) -> (nbest_out, terms [B, N, 1 + S], order
        [B, N]) on the device as ops.nbest_rescore returns them; terms = (s1, decoder term, lm term) for the scorers present"""
        if self.decoder is not None and self.decoder.training:
            raise ValueError("n-best rescoring: the decoder is in training mode (call eval())")
        if self.lm is not None and _lm_dropout_active(self.lm):
            raise ValueError("n-best rescoring: the language model is in training mode with dropout > 0 (call eval())")
        B, N, W = nbest.shape
        U = max(int(nbest[:, :, 1].max().item()), 0) + 1               # host read 1 of 2: sizes every operand below
        V = (self.decoder.output_layer if self.decoder is not None else lm_output(self.lm)).out_features
        ys_in, col, ulen = ops.nbest_pack(nbest, U, V, self.sos, self.eos)
        scorers = []
        if self.decoder is not None:
            if torch.is_tensor(hlens) and hlens.is_cuda:
                mask = (torch.arange(memory.shape[1], device=hlens.device).view(1, 1, -1) < hlens.view(-1, 1, 1))
            else:
                hl = [int(v) for v in (hlens.tolist() if torch.is_tensor(hlens) else hlens)]
                mask = make_non_pad_mask(hl, memory.shape[1]).unsqueeze(-2)
            hidden = self.decoder.forward_nbest(ys_in.view(B, N, U), ulen, memory.contiguous(), mask)
            scorers.append(self._stats(hidden, self.decoder.output_layer, col) + (self.w_dec,))
        if self.lm is not None:
            hidden, lin = lm_hidden_rows(self.lm, ys_in)
            if lin.out_features != V:
                raise ValueError("n-best rescoring: the language model covers %d tokens, the decoder %d" % (lin.out_features, V))
            scorers.append(self._stats(hidden, lin, col) + (self.w_lm,))
        return ops.nbest_rescore(nbest, ulen, U, scorers, self.w0)

    def rescore(self, memory, hlens, nbest):
        """-> per utterance [{"score": f, "yseq": [sos] + y + [eos], "scores": {"ctc": s1, "decoder": att, "lm": lm}}], best
        first ("scores" holds the terms of the scorers present, unweighted)"""
        out, terms, order = self.rescore_device(memory, hlens, nbest)
        B, N, W = out.shape
        flat = torch.cat([out.view(B, N, W), terms.view(torch.int32), order.unsqueeze(-1)], dim=2).cpu().numpy()   # host read 2 of 2
        names = ["ctc"] + (["decoder"] if self.decoder is not None else []) + (["lm"] if self.lm is not None else [])
        res = []
        for b in range(B):
            hyps = []
            for k in range(N):
                L = int(flat[b, k, 1])
                if L < 0:
                    continue
                tv = flat[b, k, W:W + len(names)].copy().view(np.float32)
                hyps.append({"score": float(flat[b, k, :1].copy().view(np.float32)[0]),
                             "yseq": [self.sos] + flat[b, k, 2:2 + L].tolist() + [self.eos],
                             "scores": {n: float(v) for n, v in zip(names, tv)}})
            res.append(hyps)
        return res
