#!/usr/bin/env python3
"""Time-synchronous CTC prefix beam search (nets.ctc_prefix_beam, csrc/ctc_beam.hip) on synthetic log-posteriors at BASELINE
config 2's decode width: T = 249 frames, |V| = 5000, beam 10, 10 candidates per frame, B = 1 and 32 utterances per call,
without an LM and with a seeded random trigram ARPA model (tools/bench_ngram.py: write_random_trigram).

  search     utt/s of CTCPrefixBeamSearch.forward_batch (candidate top-K + the one-launch search + one device-to-host copy),
             host clock around calls that end in that copy
  kernels    device time of the candidate top-K launch and of the eamd_ctc_prefix_beam launch, each alone on buffers made
             beforehand (events around a burst of 50 back-to-back launches of that one kernel, so launch gaps between them are
             in the figure and allocations are not), the search kernel's time per frame and the top-K launch's share of the two
  ambiguity  the same search on posteriors that are sharp everywhere except one early frame with two equally likely tokens:
             the two best hypotheses differ in that token and share every later one, as the n-best of real speech does
  baseline   the label-synchronous BeamSearch(weights={"ctc": 1.0}, pre_beam_score_key=None) on the same posteriors at the same
             beam - before this search the only pure-CTC beam search - and greedy CTC (argmax + collapse) beside it

Usage: python tools/bench_ctc_prefix_beam.py [--iters 50] [--out profiles/ctc_prefix_beam_bench.json] [--no-baseline]"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def posteriors(B, T, V, seed):
    """fp32 log-softmax rows [B, T, V]: N(0, 1) logits with up to +8 on one class per frame, the blank 60 % of the time"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, T, V, generator=g, device="cuda")
    tok = torch.randint(1, V - 1, (B, T), generator=g, device="cuda")
    cls = torch.where(torch.rand(B, T, generator=g, device="cuda") < 0.6, torch.zeros_like(tok), tok)
    x.scatter_add_(2, cls.unsqueeze(-1), 8.0 * torch.rand(B, T, 1, generator=g, device="cuda"))
    return torch.log_softmax(x, dim=-1).contiguous()


def posteriors_early_ambiguity(B, T, V, seed):
    """+14 on one class per frame (the blank 60 % of the time), and on TWO tokens in frame 1"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, T, V, generator=g, device="cuda")
    tok = torch.randint(1, V - 1, (B, T), generator=g, device="cuda")
    cls = torch.where(torch.rand(B, T, generator=g, device="cuda") < 0.6, torch.zeros_like(tok), tok)
    cls[:, 1] = tok[:, 1]
    x.scatter_add_(2, cls.unsqueeze(-1), torch.full((B, T, 1), 14.0, device="cuda"))
    x[:, 1].scatter_add_(1, (tok[:, 1:2] % (V - 3)) + 1 + (tok[:, 1:2] % (V - 3) + 1 == tok[:, 1:2]).long(), torch.full((B, 1), 14.0, device="cuda"))
    return torch.log_softmax(x, dim=-1).contiguous()


class _Posteriors:
    """stands in for a CTC module whose encoder output already is the log-posterior"""

    def log_softmax(self, x):
        return x


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


def device_us(fn, calls, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / calls)
    return median(ts)


def bench_search(logp, hlens, beam, K, lm, weight, iters):
    import ctypes as C
    from espnet_amd import _lib, ops
    from espnet_amd.nets.ctc_prefix_beam import CTCPrefixBeamSearch
    B, T, V = logp.shape
    search = CTCPrefixBeamSearch(beam, K, nbest=1, ngram=lm, ngram_weight=weight)
    t = wall(lambda: search.forward_batch(logp, hlens), iters)
    hl = torch.as_tensor(hlens, dtype=torch.int32).cuda()
    rows = B * T
    cval = torch.empty(rows, K, device="cuda", dtype=torch.float32)
    cidx = torch.empty(rows, K, device="cuda", dtype=torch.int64)
    cid = torch.empty(rows, K, device="cuda", dtype=torch.int32)
    topk = device_us(lambda: _lib.check(_lib.lib().eamd_topk_rows_i32(_lib.ptr(logp, 1), C.c_int64(V), rows, V - 2, K, _lib.ptr(cval),
                                                                       _lib.ptr(cidx), _lib.ptr(cid), _lib.stream_ptr()), "topk"), 50)
    out, ws = ops.ctc_prefix_beam_search(logp, cval, cid, hl, beam, 1, 0.0, lm, weight)
    serial = device_us(lambda: ops.ctc_prefix_beam_search(logp, cval, cid, hl, beam, 1, 0.0, lm, weight, ws=ws, out=out), 50)
    both = topk + serial
    best = search.forward_batch(logp, hlens)
    return dict(utt_per_s=B / t, call_ms=t * 1e3, topk_launch_us=topk, search_launch_us=serial,
                search_us_per_frame=serial / T, topk_share=topk / both if both else None,
                best_len_utt0=len(best[0][0]["yseq"]) - 2, best_score_utt0=best[0][0]["score"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--T", type=int, default=249)
    ap.add_argument("--V", type=int, default=5000)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--ngrams", type=int, default=100000, help="bigrams and trigrams listed, each")
    ap.add_argument("--weight", type=float, default=0.3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark measures the GPU"
    import espnet_amd
    from bench_ngram import write_random_trigram
    from espnet_amd import ops
    from espnet_amd.nets.beam_search import BeamSearch
    from espnet_amd.nets.ctc_prefix_score import CTCPrefixScorer
    from espnet_amd.nets.ngram import ArpaLM

    espnet_amd.set_precision("fp32")
    T, V = a.T, a.V
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tri.arpa")
        toks, total = write_random_trigram(path, V - 10, a.ngrams, 7, V)
        lm = ArpaLM(path, toks).to("cuda")
    res = dict(T=T, V=V, beam=a.beam, K=a.K, ngrams=total, order=lm.order, ngram_weight=a.weight)
    for B in (1, 32):
        logp = posteriors(B, T, V, seed=B)
        hlens = [T] * B
        r = dict(prefix_beam=bench_search(logp, hlens, a.beam, a.K, None, 0.0, a.iters),
                 prefix_beam_ngram=bench_search(logp, hlens, a.beam, a.K, lm, a.weight, a.iters),
                 prefix_beam_early_ambiguity=bench_search(posteriors_early_ambiguity(B, T, V, seed=B), hlens, a.beam, a.K, None, 0.0,
                                                          a.iters))

        def greedy():
            ids = ops.argmax_rows(logp.view(B * T, V)).view(B, T).to(torch.int32).contiguous()
            out, n = ops.ctc_collapse(ids, None, 0)
            return out.cpu(), n.cpu()

        t = wall(greedy, a.iters)
        r["greedy"] = dict(utt_per_s=B / t, call_ms=t * 1e3)
        if not a.no_baseline:
            bs = BeamSearch(dict(ctc=CTCPrefixScorer(_Posteriors(), V - 1)), dict(ctc=1.0), a.beam, V, V - 1, V - 1,
                            pre_beam_score_key=None)
            encs = [logp[b] for b in range(B)]
            t = wall(lambda: bs.forward_batch(encs) if B > 1 else bs(encs[0]), min(a.iters, 3))
            r["label_sync_baseline"] = dict(utt_per_s=B / t, call_ms=t * 1e3)
            r["speedup_vs_label_sync"] = r["prefix_beam"]["utt_per_s"] / r["label_sync_baseline"]["utt_per_s"]
        res["B%d" % B] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
