#!/usr/bin/env python3
"""Two-pass decoding (nets.nbest_rescore, csrc/rescore.hip) at BASELINE config 2's decode width: the DECODE_R4 model of
oracle/seeded_weights.py (adim 256, d_k 64, ff 2048, 2 + 2 layers, |V| = 5000), T' = 249 encoder frames per utterance (1000
input frames), beam = N = 10, B = 32 and 16 utterances per call.  The encoder is outside every figure: all of them start from
the same encoder outputs.

  first_pass    CTC log-softmax + CTCPrefixBeamSearch.search_device (the whole beam as n-best, left on the device)
  second_pass   NBestRescorer.rescore on that n-best: decoder only, and decoder + a 2-layer LSTM LM (SequentialRNNLM, 650 units)
  two_pass      the two together (first pass, then decoder-only / decoder + LM rescoring), host clock around calls that end in
                the result's device-to-host copy
  label_sync    the label-synchronous joint CTC/attention BeamSearch.forward_batch on the same utterances at the same beam and
                ctc_weight, in the same run (--no-baseline skips it)

Usage: python tools/bench_rescore.py [--iters 20] [--out profiles/rescore_bench.json] [--no-baseline]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def wall(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=1000, help="input frames per utterance (1000 -> T' = 249)")
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--ctc-weight", type=float, default=0.3)
    ap.add_argument("--lm-weight", type=float, default=0.5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark measures the GPU"
    import seeded_weights as SW

    import espnet_amd
    from espnet_amd.espnet2 import SequentialRNNLM
    from espnet_amd.nets.beam_search import BeamSearch
    from espnet_amd.nets.ctc_prefix_beam import CTCPrefixBeamSearch
    from espnet_amd.nets.ctc_prefix_score import LengthBonus
    from espnet_amd.nets.e2e_asr_conformer import E2E
    from espnet_amd.nets.nbest_rescore import NBestRescorer

    espnet_amd.set_precision("fp32")
    spec = SW.DECODE_R4
    model = SW.decode_r4_model(E2E).to("cuda").eval()
    V = spec["odim"]
    torch.manual_seed(11)
    lm = SequentialRNNLM(V, unit=650, nlayers=2, rnn_type="lstm").to("cuda").eval()
    search = CTCPrefixBeamSearch(a.beam, nbest=a.beam)
    dec_only = NBestRescorer(decoder=model.decoder, ctc_weight=a.ctc_weight, sos=model.sos, eos=model.eos)
    dec_lm = NBestRescorer(decoder=model.decoder, lm=lm, ctc_weight=a.ctc_weight, lm_weight=a.lm_weight, sos=model.sos, eos=model.eos)
    res = dict(frames=a.frames, V=V, beam=a.beam, ctc_weight=a.ctc_weight, lm_weight=a.lm_weight)
    g = torch.Generator().manual_seed(spec["seed"])
    for B in (32, 16):
        xs = [torch.randn(a.frames, spec["idim"], generator=g) for _ in range(B)]
        encs = [model.encode(x) for x in xs]
        hs_pad = torch.nn.utils.rnn.pad_sequence(encs, batch_first=True).contiguous()
        hlens = [e.shape[0] for e in encs]

        def first():
            with torch.no_grad():
                return search.search_device(model.ctc.log_softmax(hs_pad), hlens)

        nbest = first()
        lens = nbest[:, :, 1].cpu()
        r = dict(T_enc=hs_pad.shape[1], hyps=int((lens >= 0).sum()), longest=int(lens.max()), mean_len=float(lens[lens >= 0].float().mean()))
        t = wall(lambda: first().cpu(), a.iters)
        r["first_pass"] = dict(utt_per_s=B / t, call_ms=t * 1e3)
        for name, rs in (("decoder", dec_only), ("decoder_lm", dec_lm)):
            t2 = wall(lambda: rs.rescore(hs_pad, hlens, nbest), a.iters)
            t12 = wall(lambda: rs.rescore(hs_pad, hlens, first()), a.iters)
            r["second_pass_" + name] = dict(utt_per_s=B / t2, call_ms=t2 * 1e3)
            r["two_pass_" + name] = dict(utt_per_s=B / t12, call_ms=t12 * 1e3)
        if not a.no_baseline:
            scorers = model.scorers()
            scorers["length_bonus"] = LengthBonus(V)
            bs = BeamSearch(scorers, dict(decoder=1.0 - a.ctc_weight, ctc=a.ctc_weight, length_bonus=0.0), a.beam, V, model.sos,
                            model.eos, pre_beam_score_key="full")
            t = wall(lambda: bs.forward_batch(encs), min(a.iters, 3))
            r["label_sync"] = dict(utt_per_s=B / t, call_ms=t * 1e3)
            r["two_pass_decoder_vs_label_sync"] = r["two_pass_decoder"]["utt_per_s"] / r["label_sync"]["utt_per_s"]
        res["B%d" % B] = r
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
