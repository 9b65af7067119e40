"""Time-synchronous CTC prefix beam search (Hannun et al. 2014, "First-pass large vocabulary continuous speech recognition using
bi-directional recurrent DNNs") with n-gram shallow fusion, for CTC-only models.  The reference has no such search: its
Transformer E2E raises NotImplementedError("Pure CTC beam search is not implemented.") and espnet2 runs a pure-CTC model through
the label-synchronous BeamSearch, a full-vocabulary CTC prefix score per hypothesis per output token.

Definition (blank = 0, sos = eos = V - 1).  The beam is a set of distinct prefixes l with (pb, pnb): the log-probabilities of
all alignments of the frames so far that spell l and end in blank / non-blank; it starts as {(): (0, -inf)}.  Frame t < hlen,
C_t = the K largest logp[t, v] over v in 1 .. V-2 (equal values to the lower id), tot = logaddexp(pb, pnb), `+=` = logaddexp:

    pb'(l) += tot + logp[t, blank]
    for c in C_t:   c == last(l):  pnb'(l) += pnb + logp[t, c];  pnb'(l + c) += pb + logp[t, c]
                    otherwise:     pnb'(l + c) += tot + logp[t, c]

(l + c may itself be in the beam: one entry).  Kept: the W entries of largest finite
s(l) = logaddexp(pb', pnb') + ngram_weight * LM(l) + penalty * |l|, LM(l) = sum_i log10 p(w_i | <s> w_<i) - base-10 logs, passed
on unconverted as the other n-gram scorers do.  After the last frame s += ngram_weight * log10 p(</s> | context) and the n-best
is sorted by s.  The search is one launch for the whole batch (csrc/ctc_beam.hip); log-softmax, candidate top-K, search and
backtrace are enqueued back to back and ONE device-to-host copy fetches the n-best lists.
"""
import numpy as np
import torch

from .. import ops
from .ngram import ArpaLM

MAX_BEAM, MAX_CAND, MAX_FRAMES = ops.CTC_BEAM_MAX_W, ops.CTC_BEAM_MAX_K, ops.CTC_BEAM_MAX_T


class CTCPrefixBeamSearch:
    """beam_size W <= 32, cand_size K <= 32 (default min(W, V - 2)), nbest <= W, length bonus `penalty`; ngram: an ArpaLM, or an
    n-gram scorer of nets.ngram (its .lm is used), fused with ngram_weight"""

    def __init__(self, beam_size, cand_size=None, nbest=1, penalty=0.0, ngram=None, ngram_weight=0.0, blank=0, eos=None):
        if blank != 0:
            raise ValueError("CTC prefix beam search: blank must be id 0, not %r" % (blank,))
        beam_size, nbest = int(beam_size), int(nbest)
        if not 1 <= beam_size <= MAX_BEAM:
            raise ValueError("beam_size %d outside 1 .. %d" % (beam_size, MAX_BEAM))
        if cand_size is not None and not 1 <= int(cand_size) <= MAX_CAND:
            raise ValueError("cand_size %d outside 1 .. %d" % (cand_size, MAX_CAND))
        if not 1 <= nbest <= beam_size:
            raise ValueError("nbest %d outside 1 .. beam_size %d" % (nbest, beam_size))
        lm = getattr(ngram, "lm", ngram)
        if lm is not None and not isinstance(lm, ArpaLM):
            raise TypeError("ngram: an ArpaLM or an n-gram scorer of nets.ngram, not %s" % type(ngram).__name__)
        self.beam_size, self.cand_size, self.nbest = beam_size, None if cand_size is None else int(cand_size), nbest
        self.penalty, self.lm, self.ngram_weight, self.eos = float(penalty), lm, float(ngram_weight), eos

    def _cand(self, V):
        return self.cand_size if self.cand_size is not None else min(self.beam_size, V - 2)

    def search_device(self, logp, hlens):
        """logp [B, T, V] fp32 log-softmax rows on the device, hlens [B] (list or tensor), 1 <= hlens[b] <= T -> the packed
        n-best int32 [B, nbest, 2 + T] on the device (ops.ctc_prefix_beam); nothing is read back"""
        if logp.dim() != 3:
            raise ValueError("logp: [B, T, V], not %s" % (tuple(logp.shape),))
        B, T, V = logp.shape
        if self.eos is not None and self.eos != V - 1:
            raise ValueError("CTC prefix beam search: eos must be the last id %d, not %d" % (V - 1, self.eos))
        if V < 3:
            raise ValueError("a vocabulary of %d leaves no token between blank and eos" % V)
        K = self._cand(V)
        if K > V - 2:
            raise ValueError("cand_size %d: only %d tokens between blank and eos" % (K, V - 2))
        if T > MAX_FRAMES:
            raise ValueError("%d frames: the search keeps at most %d" % (T, MAX_FRAMES))
        if not (torch.is_tensor(hlens) and hlens.is_cuda):           # host lengths: checked here at no cost
            hl = [int(v) for v in (hlens.tolist() if torch.is_tensor(hlens) else hlens)]
            if len(hl) != B or not all(1 <= h <= T for h in hl):
                raise ValueError("hlens: %d lengths in 1 .. %d" % (B, T))
            hlens = torch.as_tensor(hl, dtype=torch.int32)
        hlens = hlens.to(device=logp.device, dtype=torch.int32).contiguous()
        if self.lm is not None:
            if self.lm.n_vocab != V:
                raise ValueError("the n-gram LM covers %d tokens, the posteriors %d" % (self.lm.n_vocab, V))
            self.lm.to(logp.device)
        return ops.ctc_prefix_beam(logp.to(torch.float32).contiguous(), hlens, self.beam_size, K, self.nbest, self.penalty,
                                   self.lm, self.ngram_weight if self.lm is not None else 0.0)

    def forward_batch(self, logp, hlens):
        """-> per utterance the n-best list [{"score": s, "yseq": [sos] + l + [eos]}], best first"""
        V = logp.shape[2]
        out = self.search_device(logp, hlens).cpu().numpy()          # the one device-to-host copy
        score = out[:, :, 0].copy().view(np.float32)
        res = []
        for b in range(out.shape[0]):
            hyps = []
            for n in range(out.shape[1]):
                L = int(out[b, n, 1])
                if L >= 0:
                    hyps.append({"score": float(score[b, n]), "yseq": [V - 1] + out[b, n, 2:2 + L].tolist() + [V - 1]})
            res.append(hyps)
        return res

    def __call__(self, logp):
        """logp [T, V] of one utterance -> its n-best list"""
        if logp.dim() != 2:
            raise ValueError("logp of one utterance: [T, V], not %s" % (tuple(logp.shape),))
        return self.forward_batch(logp.unsqueeze(0), [logp.shape[0]])[0]
