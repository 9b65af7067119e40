#!/usr/bin/env python3
"""n-gram LM shallow fusion at BASELINE config 2's decode width: the DECODE_R4 model of oracle/seeded_weights.py (adim 256,
aheads 4, units 2048, |V| = 5000), beam 10, 32 utterances per search (320 hypothesis rows), a seeded random trigram ARPA model
of about 200k n-grams over the vocabulary.

  kernel   eamd_ngram_score at n = 320 rows: us per call, issued back to back from the host and as replays of a hipGraph of
           20 calls (the device time), next to the floor of the n V 4 bytes every call writes
  search   utt/s of BeamSearch.forward_batch with and without the n-gram scorer, eager and with step graphs, and the
           kernel's share of a beam step

Usage: python tools/bench_ngram.py [--iters 3] [--B 32] [--ngrams 100000]"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def write_random_trigram(path, n_words, n_per_order, seed, n_tokens):
    """a seeded random well-formed trigram ARPA file (every n-gram's context and its suffix are listed one order lower)
    -> token list: <blank>, <unk>, the words, tokens the file does not list, <eos>"""
    rnd = random.Random(seed)
    words = ["w%d" % i for i in range(n_words)]
    levels = [[("<unk>",), ("<s>",), ("</s>",)] + [(w,) for w in words]]
    ext = {(): words + ["</s>"]}
    for _k in (2, 3):
        ctxs = [g for g in levels[-1] if g[-1] != "</s>" and g[0] != "<unk>"]
        new = set()
        for _ in range(4 * n_per_order):
            if len(new) >= n_per_order:
                break
            g = rnd.choice(ctxs)
            cand = ext.get(g[1:], [])
            if cand:
                new.add(g + (rnd.choice(cand),))
        new = sorted(new)
        ext = {}
        for g in new:
            ext.setdefault(g[:-1], []).append(g[-1])
        levels.append(new)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n" + "".join("ngram %d=%d\n" % (k + 1, len(lv)) for k, lv in enumerate(levels)) + "\n")
        for k, lv in enumerate(levels):
            f.write("\\%d-grams:\n" % (k + 1))
            for g in lv:
                bo = "" if k == 2 else "\t%.7f" % rnd.uniform(-1.0, 0.0)
                f.write("%.7f\t%s%s\n" % (rnd.uniform(-3.0, -0.05), " ".join(g), bo))
            f.write("\n")
        f.write("\\end\\\n")
    return ["<blank>", "<unk>"] + words + ["x%d" % i for i in range(n_tokens - n_words - 3)] + ["<eos>"], sum(len(lv) for lv in levels)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def bench_kernel(lm, n, V, reps=5):
    from espnet_amd import ops
    g = torch.Generator().manual_seed(0)
    W = len(lm.words)
    ctx = torch.randint(0, W, (n, lm.order - 1), generator=g, dtype=torch.int32).cuda()
    ys = torch.randint(0, V, (n, 12), generator=g).cuda()
    tok = ys[:, -1]
    # contexts a search meets: rows whose newest two words form a listed bigram reach depth 2
    cs, cw = lm.child_start.cpu(), lm.child_word.cpu()
    t2w = lm.tok2word.cpu()
    for r in range(0, n, 2):
        w = int(t2w[int(ys[r, -1])])
        node = int(torch.searchsorted(cw[: int(cs[1])].contiguous(), torch.tensor(w, dtype=torch.int32))) + 1 if int(cs[1]) else 0
        if 0 < node < cs.numel() - 1 and int(cw[node - 1]) == w and int(cs[node + 1]) > int(cs[node]):
            ctx[r, 0] = int(cw[int(cs[node])])
    calls = 200

    def burst():
        for _ in range(calls):
            ops.ngram_score(lm, ctx, tok)

    burst()
    torch.cuda.synchronize()
    host = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        burst()
        e1.record()
        torch.cuda.synchronize()
        host.append(e0.elapsed_time(e1) * 1e3 / calls)
    gcalls = 20
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for _ in range(gcalls):
                keep = ops.ngram_score(lm, ctx, tok)
    torch.cuda.synchronize()
    dev = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3 / (10 * gcalls))
    del keep
    return dict(n=n, V=V, host_issued_us=median(host), graph_replay_us=median(dev[1:]), bytes_written=n * V * 4)


def timed_search(bs, encs, ratio, iters):
    bs.forward_batch(encs, maxlenratio=ratio)
    bs.forward_batch(encs[1:] + encs[:1], maxlenratio=ratio)          # (with step graphs: the capturing search)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = bs.forward_batch(encs, maxlenratio=ratio)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--ngrams", type=int, default=100000, help="bigrams and trigrams listed, each")
    ap.add_argument("--ratio", type=float, default=0.2)
    ap.add_argument("--weight", type=float, default=0.3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark measures the GPU"
    import seeded_weights as SW
    import espnet_amd
    from espnet_amd import ops
    from espnet_amd.nets.beam_search import BeamSearch
    from espnet_amd.nets.ctc_prefix_score import CTCPrefixScorer, LengthBonus
    from espnet_amd.nets.e2e_asr_conformer import E2E
    from espnet_amd.nets.ngram import ArpaLM, NgramFullScorer

    espnet_amd.set_precision("fp32")
    V, beam = SW.DECODE_R4["odim"], SW.DECODE_R4["beam"]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tri.arpa")
        toks, total = write_random_trigram(path, V - 10, a.ngrams, 7, V)
        t0 = time.perf_counter()
        lm = ArpaLM(path, toks).to("cuda")
        t_tables = time.perf_counter() - t0
    res = dict(V=V, beam=beam, B=a.B, ngrams=total, order=lm.order, nodes=lm.node_bo.numel(), successors=lm.succ_tok.numel(),
               tables_s=t_tables, kernel=bench_kernel(lm, a.B * beam, V))
    model = SW.decode_r4_model(E2E).to("cuda").eval()
    g = torch.Generator().manual_seed(2)
    lens = [int(v) for v in torch.linspace(1000, 600, a.B).round().tolist()]
    encs = [model.encode(torch.randn(T, SW.DECODE_R4["idim"], generator=g)) for T in lens]

    def mk(ngram, graphs):
        scorers = dict(decoder=model.decoder, ctc=CTCPrefixScorer(model.ctc, model.eos), length_bonus=LengthBonus(V),
                       ngram=NgramFullScorer(lm, toks) if ngram else None)
        bs = BeamSearch(scorers, dict(decoder=0.7, ctc=0.3, length_bonus=0.1, ngram=a.weight), beam, V, model.sos, model.eos,
                        pre_beam_score_key="full")
        bs.graph_steps = graphs
        return bs

    # steps of one search = launches of the row kernel in it
    count = [0]
    real = ops.ngram_score

    def counting(*args, **kw):
        count[0] += 1
        return real(*args, **kw)

    ops.ngram_score = counting
    mk(True, False).forward_batch(encs, maxlenratio=a.ratio)
    ops.ngram_score = real
    res["steps_per_search"] = count[0]
    for graphs in (False, True):
        tag = "graphs" if graphs else "eager"
        bs0, bs1 = mk(False, graphs), mk(True, graphs)
        t_without, _ = timed_search(bs0, encs, a.ratio, a.iters)
        t_with, out = timed_search(bs1, encs, a.ratio, a.iters)
        assert not graphs or (bs0.graph_steps and bs1.graph_steps), "a step could not be captured"
        step_us = t_with / max(1, count[0]) * 1e6
        res[tag] = dict(without_utt_per_s=a.B / t_without, with_utt_per_s=a.B / t_with, step_us_with=step_us,
                        kernel_share_of_step=res["kernel"]["graph_replay_us"] / step_us)
    res["best_ngram_score_utt0"] = float(out[0][0].scores["ngram"]) if out and out[0] else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
