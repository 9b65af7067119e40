#!/usr/bin/env python3
"""RNN LM shallow fusion in the batched alsd / tsd transducer searches (BeamSearchTransducer.alsd_batch / tsd_batch with
lm=ClassifierWithState(RNNLM), lm_batched=True; csrc/rnnt_alsd.hip / rnnt_tsd.hip: eamd_rnnt_*_step_lm) at the width of BASELINE config 5 as
tools/bench_transducer_alsd.py builds it: encoder states of T' = 374 frames x 256, one LSTM layer of 512 units behind a 512-wide
embedding, joint space 320, |V| = 5000, u_max 50 (alsd), max_sym_exp 2 (tsd); beams 4 and 8; B = 16 and 32 utterances per call.
LMs: 2-layer LSTM LMs of 650 units (the reference's default; 650 is no multiple of 64, so its steps are a GEMM + a cell kernel) and
of 1024 units (the one-launch LSTM step), seeded, lm_weight 0.3.

  batched_lm    median over `--iters` calls of alsd_batch / tsd_batch with the LM (host clock around calls that end in their one
                device-to-host copy), utt/s and the time per step (alsd: T + min(u_max, T - 1) per call) / pass (tsd: T x max_sym_exp)
  batched       the same search without an LM, timed the same way in the same process, the two alternating
  per_utt_lm    the per-utterance search with the LM (BeamSearchTransducer.__call__) on the first `--per-utt` utterances, one call
                each: what recognize_batch fell back to before

Launches per step / pass come from profiler runs of their own, one per (search, LM size):
  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_transducer_lm.py --trace 2 --trace-search alsd \\
      --trace-units 650
  python tools/bench_transducer_lm.py --launches DIR --trace 2 --trace-search alsd --trace-units 650 --out profiles/transducer_lm_bench.json
(--trace N: only N batched calls at B = 16, nothing timed; --launches: kernel dispatches of that run / (N x steps), the set-up
- seeded weights, encoder projection, buffer fills, the initial steps - included, merged into the JSON of an earlier run).

--parent DIR compares the searches WITHOUT an LM with another checkout of the project (DIR, built; the parent commit): its package
is loaded under another name into the same process, both get the same calibrated weights, and every configuration is timed other
checkout, this tree, other checkout again, the three taking turns within each of `--iters` iterations; the two columns of the other
checkout show the spread.  It also says whether both return the same sequences and how far the scores differ, between the trees
and between two calls of the same tree.  Nothing else is measured in that run; the result goes under "nolm_vs_parent".

Usage: python tools/bench_transducer_lm.py [--iters 8] [--out profiles/transducer_lm_bench.json]
       python tools/bench_transducer_lm.py --parent DIR --iters 16 --out profiles/transducer_lm_bench.json"""
import argparse
import csv
import importlib
import importlib.util
import glob
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
LM_WEIGHT = 0.3


def searches(a, dec, lm, beam, cls=None):
    if cls is None:
        from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer as cls
    kw = dict(alsd=dict(u_max=a.u_max), tsd=dict(max_sym_exp=a.max_sym_exp))
    fused = {} if lm is None else dict(lm=lm, lm_weight=LM_WEIGHT, lm_batched=True)
    return {kind: cls(decoder=dec, beam_size=beam, search_type=kind, **fused, **kw[kind]) for kind in ("alsd", "tsd")}


def language_model(a, units):
    from espnet_amd.nets.lm import ClassifierWithState, RNNLM
    torch.manual_seed(units)
    return ClassifierWithState(RNNLM(a.V, 2, units, None, "lstm", 0.0)).to(DEV).eval()


def units_per_call(a, kind):
    return a.T + min(a.u_max, a.T - 1) if kind == "alsd" else a.T * a.max_sym_exp


def alternating(fns, iters, warm):
    """median wall time of every fn, the fns taking turns so that drift of the machine falls on all alike"""
    import time
    from bench_transducer_greedy import median
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for j, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[j].append(time.perf_counter() - t0)
    return [median(t) for t in ts]


def bench(a):
    from bench_transducer_alsd import decoder, wall
    dec, g, tokens = decoder(a)
    res = dict(greedy_tokens_per_utt=tokens, lm_weight=LM_WEIGHT, lm_layers=2,
               units_per_call=dict(alsd=units_per_call(a, "alsd"), tsd=units_per_call(a, "tsd")))
    states = {B: torch.randn(B, a.T, 256, generator=g).to(DEV) for B in (16, 32)}
    for units in (650, 1024):
        lm = language_model(a, units)
        for beam in (4, 8):
            plain = searches(a, dec, None, beam)
            fused = searches(a, dec, lm, beam)
            for kind in ("alsd", "tsd"):
                n_units = units_per_call(a, kind)
                for B, hs in states.items():
                    run = lambda s: getattr(s, kind + "_batch")(hs)      # noqa: E731
                    row = lambda t: dict(utt_per_s=B / t, call_ms=t * 1e3, unit_us=t * 1e6 / n_units)      # noqa: E731
                    key = "%s_beam%d_B%d" % (kind, beam, B)
                    assert fused[kind]._lm_batched_ok(), "the device loop does not take this LM"
                    want = run(fused[kind])
                    t_f, t_p = alternating([lambda: run(fused[kind]), lambda: run(plain[kind])], a.iters, warm=2)
                    m = min(B, a.per_utt)
                    one = [fused[kind](hs[b]) for b in range(m)]
                    t_u = wall(lambda: [fused[kind](hs[b]) for b in range(m)], 1, warm=0)
                    same = [[h.yseq for h in nb] for nb in one] == [[h.yseq for h in nb] for nb in want[:m]]
                    res["lm%d_%s" % (units, key)] = dict(
                        batched_lm=row(t_f), batched=row(t_p), per_utt_lm=dict(utt_per_s=m / t_u, ms_per_utt=t_u * 1e3 / m, utterances=m),
                        lm_cost=t_f / t_p, speedup_over_per_utt=(t_u / m) / (t_f / B), rows=B * min(beam, a.V),
                        one_launch_lm_step=units % 64 == 0 and B * min(beam, a.V) <= 64,
                        best_len=len(want[0][0].yseq) - 1, same_nbest_as_per_utt=same)      # seeded weights: a near-tie may differ
                    print("lm %d %s: with LM %.1f ms, without %.1f ms, per utterance %.1f ms" % (units, key, t_f * 1e3, t_p * 1e3,
                                                                                                 t_u * 1e3 / m), file=sys.stderr, flush=True)
    return res


def compare_parent(a):
    """alsd_batch / tsd_batch without an LM: the checkout a.parent against this tree, in one process"""
    from bench_transducer_alsd import decoder
    path = os.path.join(os.path.abspath(a.parent), "espnet_amd")
    spec = importlib.util.spec_from_file_location("espnet_amd_parent", os.path.join(path, "__init__.py"),
                                                  submodule_search_locations=[path])
    other = importlib.util.module_from_spec(spec)
    sys.modules["espnet_amd_parent"] = other
    spec.loader.exec_module(other)
    other.set_precision("fp32")
    dec, g, tokens = decoder(a)
    odec = importlib.import_module("espnet_amd_parent.nets.transducer.rnn_decoder").DecoderRNNT(
        256, a.V, "lstm", 1, 512, 0, 512, 320, "tanh").to(DEV).eval()
    odec.load_state_dict(dec.state_dict())
    ocls = importlib.import_module("espnet_amd_parent.nets.beam_search_transducer").BeamSearchTransducer
    states = {B: torch.randn(B, a.T, 256, generator=g).to(DEV) for B in (16, 32)}

    def diff(x, y):
        """(utterances whose n-best sequences differ, largest absolute score difference)"""
        seq = sum([h.yseq for h in p] != [h.yseq for h in q] for p, q in zip(x, y))
        return seq, max([abs(h.score - k.score) for p, q in zip(x, y) for h, k in zip(p, q)] + [0.0])

    res = dict(iters=a.iters, greedy_tokens_per_utt=tokens)
    for beam in (4, 8):
        new, old = searches(a, dec, None, beam), searches(a, odec, None, beam, ocls)
        for kind in ("alsd", "tsd"):
            for B, hs in states.items():
                f_new = lambda: getattr(new[kind], kind + "_batch")(hs)      # noqa: E731
                f_old = lambda: getattr(old[kind], kind + "_batch")(hs)      # noqa: E731
                r_new, r_old, r_new2, r_old2 = f_new(), f_old(), f_new(), f_old()
                t = alternating([f_old, f_new, f_old], a.iters, warm=2)
                key = "%s_beam%d_B%d" % (kind, beam, B)
                res[key] = dict(parent_ms=t[0] * 1e3, this_ms=t[1] * 1e3, parent_again_ms=t[2] * 1e3, rows=B * min(beam, a.V),
                                this_vs_parent=diff(r_new, r_old), this_vs_this=diff(r_new, r_new2), parent_vs_parent=diff(r_old, r_old2))
                print("%s: parent %.2f, this tree %.2f, parent again %.2f ms" % ((key,) + tuple(x * 1e3 for x in t)), file=sys.stderr,
                      flush=True)
    return res


def trace(a):
    """a.trace batched calls at B = 16, nothing timed: the process a kernel trace is taken of.  The blank bias is not calibrated
    here (that would run the greedy search in the traced process): the launches of a step do not depend on the data"""
    from bench_transducer_alsd import decoder
    dec, g, _ = decoder(a, calibrated=False)
    hs = torch.randn(16, a.T, 256, generator=g).to(DEV)
    lm = language_model(a, a.trace_units) if a.trace_units else None
    search = searches(a, dec, lm, a.trace_beam)[a.trace_search]
    for _ in range(a.trace):
        getattr(search, a.trace_search + "_batch")(hs)
    torch.cuda.synchronize()


def launches(a):
    """kernel dispatches per step / pass from the kernel statistics of a traced --trace run"""
    files = glob.glob(os.path.join(a.launches, "**", "*kernel_stats.csv"), recursive=True)
    assert files, "no kernel statistics under %s" % a.launches
    n = sum(int(row["Calls"]) for f in files for row in csv.DictReader(open(f)))
    per = units_per_call(a, a.trace_search)
    return dict(calls=a.trace, beam=a.trace_beam, B=16, kernel_dispatches=n, launches_per_unit=n / (a.trace * per),
                includes="the process's set-up: seeded weights, encoder projection, buffer fills, the initial steps, the result's "
                         "concatenation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--per-utt", dest="per_utt", type=int, default=2)
    ap.add_argument("--T", type=int, default=374)
    ap.add_argument("--V", type=int, default=5000)
    ap.add_argument("--u-max", dest="u_max", type=int, default=50)
    ap.add_argument("--max-sym-exp", dest="max_sym_exp", type=int, default=2)
    ap.add_argument("--tokens", type=float, default=100.0)
    ap.add_argument("--parent", default=None, help="another built checkout: compare the searches without an LM with it")
    ap.add_argument("--trace", type=int, default=None)
    ap.add_argument("--trace-search", dest="trace_search", default="alsd", choices=("alsd", "tsd"))
    ap.add_argument("--trace-units", dest="trace_units", type=int, default=650, help="0: without an LM")
    ap.add_argument("--trace-beam", dest="trace_beam", type=int, default=4)
    ap.add_argument("--launches", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))
    if a.launches:
        res["launches_%s_lm%d" % (a.trace_search, a.trace_units)] = launches(a)
    else:
        assert torch.cuda.is_available(), "the benchmark measures the GPU"
        import espnet_amd
        espnet_amd.set_precision("fp32")
        if a.trace is not None:
            trace(a)
            return
        if a.parent:
            res["nolm_vs_parent"] = compare_parent(a)
            print(json.dumps(res["nolm_vs_parent"]))
            if a.out:
                with open(a.out, "w") as f:
                    f.write(json.dumps(res, indent=1) + "\n")
            return
        res.update(dict(T=a.T, V=a.V, D_enc=256, dunits=512, embed=512, joint=320, u_max=a.u_max, max_sym_exp=a.max_sym_exp,
                        iters=a.iters))
        res.update(bench(a))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
