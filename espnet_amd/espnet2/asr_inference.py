"""Speech2Text: encoder + joint CTC/attention(/LM) beam search for one utterance.

reference: espnet2/bin/asr_inference.py:36-211.  The reference builds its models from a training config
through `ASRTask.build_model_from_file` / `LMTask.build_model_from_file`; that task registry is control
plane (SURVEY.md §8 out of scope), so this class takes the built modules instead - an `ESPnetASRModel`
(ours or the reference's, holding our encoder / decoder / CTC) and optionally a language model.  Everything
after model construction follows the reference: scorer and weight dictionaries, BatchBeamSearch when every
full scorer is a BatchScorerInterface, `__call__(speech) -> [(text, token, token_int, hyp)]`.
"""
import numpy as np
import torch

from .. import ops

from ..nets.batch_beam_search import BatchBeamSearch
from ..nets.beam_search import BeamSearch, Hypothesis
from ..nets.ctc_prefix_beam import CTCPrefixBeamSearch
from ..nets.ctc_prefix_score import CTCPrefixScorer, LengthBonus
from ..nets.nbest_rescore import NBestRescorer
from ..nets.scorer_interface import BatchScorerInterface


class TokenIDConverter:
    """reference: espnet2/text/token_id_converter.py (list-backed subset)"""

    def __init__(self, token_list, unk_symbol="<unk>"):
        self.token_list = list(token_list)
        self.token2id = {t: i for i, t in enumerate(self.token_list)}
        self.unk_id = self.token2id.get(unk_symbol, None)

    def ids2tokens(self, integers):
        return [self.token_list[i] for i in integers]

    def tokens2ids(self, tokens):
        return [self.token2id.get(t, self.unk_id) for t in tokens]


class CharTokenizer:
    """reference: espnet2/text/char_tokenizer.py (tokens2text: join, <space> -> ' ')"""

    def __init__(self, space_symbol="<space>"):
        self.space_symbol = space_symbol

    def tokens2text(self, tokens):
        return "".join(" " if t == self.space_symbol else t for t in tokens)


class Speech2Text:
    def __init__(self, asr_model, lm=None, token_list=None, tokenizer=None, device="cuda", maxlenratio=0.0,
                 minlenratio=0.0, batch_size=1, beam_size=20, ctc_weight=0.5, lm_weight=1.0, penalty=0.0, nbest=1,
                 graph_steps=False, ctc_search="label", ngram=None, ngram_weight=0.0, ctc_cand_size=None):
        """ctc_search (not in the reference): "label" decodes through the label-synchronous BeamSearch whatever the weights;
        "time" with ctc_weight == 1.0 runs the time-synchronous CTC prefix beam search (nets.ctc_prefix_beam) with an optional
        n-gram LM (ngram: an ArpaLM or n-gram scorer, ngram_weight) and ctc_cand_size candidates per frame; "rescore" with
        0 < ctc_weight <= 1 is two-pass decoding: that search (ngram / ctc_cand_size belong to it) proposes its whole beam and
        nets.nbest_rescore.NBestRescorer re-ranks it with the decoder (ctc_weight < 1) and / or lm (lm_weight)"""
        if ctc_search not in ("label", "time", "rescore"):
            raise ValueError("ctc_search: 'label', 'time' or 'rescore', not %r" % (ctc_search,))
        if ctc_search == "rescore":
            if not 0.0 < ctc_weight <= 1.0:
                raise ValueError("ctc_search='rescore': 0 < ctc_weight <= 1, not %r (the first pass proposes the hypotheses)"
                                 % (ctc_weight,))
            if ctc_weight == 1.0 and lm is None:
                raise ValueError("ctc_search='rescore' with ctc_weight == 1.0 and no lm: there is nothing to rescore with")
        if ctc_search == "time" and ctc_weight != 1.0:
            raise ValueError("ctc_search='time' is the pure-CTC search: ctc_weight must be 1.0, not %r" % (ctc_weight,))
        if ctc_search == "label" and (ngram is not None or ctc_cand_size is not None):
            raise ValueError("ngram / ctc_cand_size belong to ctc_search='time': the label-synchronous search would ignore them")
        if ctc_search == "time" and lm is not None:
            raise ValueError("ctc_search='time' fuses n-gram LMs only (ngram=): a neural lm is not fused time-synchronously")
        self.ctc_search, self.ctc_prefix_beam = ctc_search, None
        if ctc_search in ("time", "rescore"):       # the second pass re-ranks the whole beam
            self.ctc_prefix_beam = dict(beam_size=beam_size, cand_size=ctc_cand_size, penalty=penalty, ngram=ngram,
                                        nbest=min(nbest, beam_size) if ctc_search == "time" else beam_size,
                                        ngram_weight=ngram_weight if ngram is not None else 0.0)
            CTCPrefixBeamSearch(**self.ctc_prefix_beam)            # the limits are checked here, before any model work
        self.rescorer = None
        asr_model.to(device).eval()
        if ctc_search == "rescore":
            if ctc_weight < 1.0 and getattr(asr_model, "decoder", None) is None:
                raise ValueError("ctc_search='rescore' with ctc_weight < 1 needs an attention decoder; this model has none")
            self.rescorer = NBestRescorer(decoder=asr_model.decoder if ctc_weight < 1.0 else None,
                                          lm=None if lm is None else lm.to(device).eval(), ctc_weight=ctc_weight,
                                          lm_weight=lm_weight if lm is not None else 0.0, sos=asr_model.sos, eos=asr_model.eos)
        token_list = token_list if token_list is not None else getattr(asr_model, "token_list", None)
        vocab = len(token_list) if token_list is not None else asr_model.vocab_size
        scorers = dict(decoder=asr_model.decoder, ctc=CTCPrefixScorer(ctc=asr_model.ctc, eos=asr_model.eos),
                       length_bonus=LengthBonus(vocab))
        if lm is not None:
            scorers["lm"] = lm.to(device).eval()
        weights = dict(decoder=1.0 - ctc_weight, ctc=ctc_weight, lm=lm_weight, length_bonus=penalty)
        beam_search = BeamSearch(beam_size=beam_size, weights=weights, scorers=scorers, sos=asr_model.sos,
                                 eos=asr_model.eos, vocab_size=vocab, token_list=token_list,
                                 pre_beam_score_key=None if ctc_weight == 1.0 else "full")
        if batch_size == 1 and all(isinstance(v, BatchScorerInterface) for v in beam_search.full_scorers.values()):
            beam_search.__class__ = BatchBeamSearch          # asr_inference.py:108-118
        beam_search.to(device).eval()
        # graph_steps (not in the reference): the steps of a search replayed as hipGraphs, see nets.beam_search.BeamSearch.graph_steps
        beam_search.graph_steps = bool(graph_steps)
        self.asr_model, self.beam_search = asr_model, beam_search
        self.converter = TokenIDConverter(token_list) if token_list is not None else None
        self.tokenizer = tokenizer
        self.maxlenratio, self.minlenratio, self.device, self.nbest = maxlenratio, minlenratio, device, nbest

    @torch.no_grad()
    @ops.inference_call
    def __call__(self, speech):
        """speech: (Nsamples,) waveform or (T, F) features, as the model's frontend expects"""
        if isinstance(speech, np.ndarray):
            speech = torch.tensor(speech)
        speech = speech.unsqueeze(0).to(torch.float32).to(self.device)
        lengths = torch.full([1], speech.size(1), dtype=torch.long)
        enc, _ = self.asr_model.encode(speech=speech, speech_lengths=lengths)
        assert len(enc) == 1, len(enc)
        if self.ctc_search == "time":
            hyps = self.asr_model.ctc.prefix_beam_search(enc, [enc.shape[1]], **self.ctc_prefix_beam)[0]
            nbest_hyps = [Hypothesis(yseq=torch.tensor(h["yseq"], dtype=torch.long), score=h["score"], scores=dict(ctc=h["score"]),
                                     states=dict()) for h in hyps]
        elif self.ctc_search == "rescore":
            ctc = self.asr_model.ctc
            search = CTCPrefixBeamSearch(blank=0, eos=ctc.ctc_lo.out_features - 1, **self.ctc_prefix_beam)
            nbest = search.search_device(ctc.log_softmax(enc.contiguous()), [enc.shape[1]])
            hyps = self.rescorer.rescore(enc, [enc.shape[1]], nbest)[0]
            nbest_hyps = [Hypothesis(yseq=torch.tensor(h["yseq"], dtype=torch.long), score=h["score"], scores=h["scores"],
                                     states=dict()) for h in hyps]
        else:
            nbest_hyps = self.beam_search(x=enc[0], maxlenratio=self.maxlenratio, minlenratio=self.minlenratio)
        results = []
        for hyp in nbest_hyps[: self.nbest]:
            assert isinstance(hyp, Hypothesis), type(hyp)
            token_int = [t for t in hyp.yseq[1:-1].tolist() if t != 0]     # drop sos/eos and the blank id 0
            token = self.converter.ids2tokens(token_int) if self.converter is not None else None
            text = self.tokenizer.tokens2text(token) if (self.tokenizer is not None and token is not None) else None
            results.append((text, token, token_int, hyp))
        return results
