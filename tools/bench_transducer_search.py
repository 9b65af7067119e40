#!/usr/bin/env python3
"""Transducer searches at BASELINE configs[4] width: encoder output 256, 1-layer LSTM prediction network 512, joint 320,
V 5000, seeded random weights; seeded encoder outputs of T' = 375 frames (1500 input frames after 4x subsampling) for
16 utterances.  The default, tsd, alsd and nsc searches (nets.beam_search_transducer) at beam 4 and 8.

Per search: ms per utterance and utterances per second (host clock around the search, device synchronized), passes per
frame and blocking host reads per frame (counted by the search; the default search has neither counter).  Kernel launches
per frame come from a separate `rocprofv3 --kernel-trace --stats` run of this tool with --only <search> --beam <b>
--utts 1.  One JSON line per (search, beam).

    python tools/bench_transducer_search.py [--utts 16] [--beams 4 8] [--only tsd] [--frames 375]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEARCHES = {"default": dict(search_type="default"), "tsd": dict(search_type="tsd", max_sym_exp=2),
            "alsd": dict(search_type="alsd", u_max=50), "nsc": dict(search_type="nsc", nstep=2, prefix_alpha=2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--frames", type=int, default=375)
    ap.add_argument("--beams", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    from espnet_amd.nets.transducer.rnn_decoder import DecoderRNNT
    torch.manual_seed(0)
    dec = DecoderRNNT(256, 5000, "lstm", 1, 512, 0, 512, 320).cuda().eval()
    g = torch.Generator().manual_seed(1)
    hs = [torch.randn(a.frames, 256, generator=g).cuda() for _ in range(a.utts)]
    for name in ([a.only] if a.only else list(SEARCHES)):
        for beam in a.beams:
            bs = BeamSearchTransducer(dec, beam_size=beam, **SEARCHES[name])
            bs(hs[0][:20])                                   # warm-up: library load, kernels, allocator
            torch.cuda.synchronize()
            passes = reads = 0
            t0 = time.perf_counter()
            for h in hs:
                bs(h)
                passes += bs.passes
                reads += bs.host_reads
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            frames = a.frames * a.utts
            print(json.dumps(dict(search=name, beam=beam, utts=a.utts, frames=a.frames,
                                  ms_per_utt=round(1e3 * dt / a.utts, 2), utt_per_s=round(a.utts / dt, 2),
                                  passes_per_frame=round(passes / frames, 3) if name != "default" else None,
                                  host_reads_per_frame=round(reads / frames, 3) if name != "default" else None)), flush=True)


if __name__ == "__main__":
    main()
