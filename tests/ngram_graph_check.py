#!/usr/bin/env python3
"""Child process of test_gpu_ngram.test_forward_batch_and_step_graphs: searches with the n-gram scorer as one batched search and
as hipGraph replays, exit code 0 when they agree with one eager search each."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from test_gpu_model import DEV, _fusion_models  # noqa: E402
from test_gpu_ngram import TOKENS30  # noqa: E402
from test_ngram import ARPA_BEAM  # noqa: E402


def same(tag, got, ref):
    assert [h.yseq.tolist() for h in got[:3]] == [h.yseq.tolist() for h in ref[:3]], tag
    for a, b in zip(got[:3], ref[:3]):
        assert abs(float(a.score) - float(b.score)) <= 1e-4 * max(1.0, abs(float(b.score))), tag
        assert abs(float(a.scores["ngram"]) - float(b.scores["ngram"])) <= 1e-4 * max(1.0, abs(float(b.scores["ngram"]))), tag


def main():
    from espnet_amd.nets.batch_beam_search import BatchBeamSearch
    from espnet_amd.nets.beam_search import BeamSearch
    from espnet_amd.nets.ctc_prefix_score import CTCPrefixScorer, LengthBonus
    from espnet_amd.nets.ngram import NgramFullScorer
    p, model, lms = _fusion_models()
    with torch.no_grad():
        enc, _ = model.encode(p["speech"].unsqueeze(0).to(DEV), torch.tensor([p["speech"].shape[0]]))
    x = enc[0]
    T = x.shape[0]
    utts = [x, x[: max(4, (2 * T) // 3)].contiguous(), (x[: max(3, T // 2)] * 1.5).contiguous(), x.flip(0).contiguous()]
    n_graphs = 0
    for cls in (BeamSearch, BatchBeamSearch):
        def mk():
            scorers = dict(decoder=model.decoder, ctc=CTCPrefixScorer(model.ctc, model.eos), length_bonus=LengthBonus(30),
                           lm=lms["tlm"], ngram=NgramFullScorer(ARPA_BEAM, TOKENS30))
            return cls(scorers, dict(decoder=0.7, ctc=0.3, lm=0.6, length_bonus=0.1, ngram=0.5), 4, 30, model.sos, model.eos,
                       pre_beam_score_key="full")
        eager, graphed = mk(), mk()
        assert len(eager.full_scorers) == 4 and eager._device_loop_ok(x)          # the limit eamd_beam_finish carries
        alone = [eager(u, maxlenratio=0.5) for u in utts]
        together = eager.forward_batch(utts, maxlenratio=0.5)
        for b in range(len(utts)):
            same("forward_batch %s %d" % (cls.__name__, b), together[b], alone[b])
        graphed.graph_steps, graphed.graph_frame_bucket = True, 16
        for rnd in range(3):                                                      # eager, capture, replay
            same("graph_steps %s search %d" % (cls.__name__, rnd), graphed(x, maxlenratio=0.5), alone[0])
        for rnd in range(3):
            got = graphed.forward_batch(utts, maxlenratio=0.5)
            for b in range(len(utts)):
                same("graph_steps %s forward_batch %d utt %d" % (cls.__name__, rnd, b), got[b], alone[b])
        assert graphed.graph_steps, "a step could not be captured: the searches above ran eagerly"
        n_graphs += sum(len(G["graphs"]) for G in graphed._step_graphs.values())
    assert n_graphs > 0
    print("[parity] ngram forward_batch and step graphs: %d captured steps" % n_graphs)


if __name__ == "__main__":
    main()
