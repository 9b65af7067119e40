#!/usr/bin/env python3
"""What CER / WER reporting costs per validation batch: the device scoring (ErrorCalculator.counts for cer_ctc + cer + wer, one
read of the six sums at the end) beside the reference's way on the same ids (copy ys_hat / ys_pad to the host, join Python
strings, edit distance per utterance), and the eval forward of the bench model with and without reporting.

Workload: B = 32, T' = 249 encoder frames, V = 5000 BPE-style tokens (no <space> in the list), frame lengths as tools/bench_decode.py
draws them (T' - 13 i / 4 valid frames for utterance i), a label per four valid frames; the frame-level hypothesis holds each label
for about three frames with blanks in between and one label in ten wrong, the teacher-forced one has one label in ten wrong.
The editdistance C extension the reference calls is not a dependency of this project: the host side runs the textbook DP of
tests/test_error_calc.py in Python (`host_ms`), and is also timed without any edit distance (`host_strings_ms`: the device-to-host
copies and the string handling alone) - the reference's cost lies between the two.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, TP, V = 32, 249, 5000


def token_list(rng):
    letters = "abcdefghijklmnopqrstuvwxyz"
    toks = ["<blank>", "<unk>"]
    while len(toks) < V - 1:
        n = int(rng.integers(1, 7))
        toks.append(("▁" if rng.random() < 0.4 else "") + "".join(letters[i] for i in rng.integers(0, 26, n)))
    return toks + ["<eos>"]


def draw(rng):
    frames = [TP - (13 * i) // 4 for i in range(B)]
    lens = [f // 4 for f in frames]
    L = max(lens)
    ys = np.full((B, L), -1, np.int64)
    att = rng.integers(2, V - 1, (B, L + 1))
    ctc = np.zeros((B, TP), np.int64)
    for b, n in enumerate(lens):
        y = rng.integers(2, V - 1, n)
        ys[b, :n] = y
        h = np.where(rng.random(n) < 0.1, rng.integers(2, V - 1, n), y)
        att[b, :n] = h
        att[b, n] = V - 1
        f = []
        for tok in np.where(rng.random(n) < 0.1, rng.integers(2, V - 1, n), y):
            f += [int(tok)] * int(rng.integers(2, 4)) + [0] * int(rng.integers(0, 2))
        ctc[b, :min(TP, len(f))] = f[:TP]
    return ys, att, ctc


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="skip the eval forward of the bench model")
    a = ap.parse_args()
    import espnet_amd
    from espnet_amd.nets.e2e_asr_common import ErrorCalculator
    from test_error_calc import char_counts, convert_to_char, ctc_counts, word_counts
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    tokens = token_list(rng)
    ys, att, ctc = draw(rng)
    ys_d, att_d, ctc_d = (torch.from_numpy(x).to(dev) for x in (ys, att, ctc))
    ec = ErrorCalculator(tokens, "<space>", "<blank>", report_cer=True, report_wer=True)

    def device_scoring():
        n_ctc = ec.counts(ctc_d, ys_d, is_ctc=True)
        n_cer, n_wer = ec.counts(att_d, ys_d)
        return ec.sums(n_ctc, n_cer, n_wer)

    def host_scoring(distances=True):
        c, h, y = ctc_d.cpu().numpy(), att_d.cpu().numpy(), ys_d.cpu().numpy()
        if not distances:
            import test_error_calc as R
            keep, R.levenshtein = R.levenshtein, lambda a, b: 0
        try:
            n_ctc = ctc_counts(tokens, "<space>", "<blank>", c, y)
            hats, trues = convert_to_char(tokens, "<space>", "<blank>", h, y)
            n_cer, n_wer = char_counts(hats, trues), word_counts(hats, trues)
        finally:
            if not distances:
                R.levenshtein = keep
        return [(sum(e), sum(n)) for e, n in (n_ctc, n_cer, n_wer)]

    assert [tuple(v) for v in device_scoring()] == host_scoring(), "device and host scoring disagree"
    res = dict(workload="B=%d T'=%d V=%d, %d reference characters" % (B, TP, V, host_scoring()[1][1]),
               device_ms=round(timed(device_scoring, a.reps), 3),
               host_ms=round(timed(host_scoring, 2), 2),
               host_strings_ms=round(timed(lambda: host_scoring(False), 5), 3))
    res["host_over_device"] = round(res["host_ms"] / res["device_ms"], 1)
    res["host_strings_over_device"] = round(res["host_strings_ms"] / res["device_ms"], 2)
    if not a.no_model:
        import bench
        from espnet_amd.nets.e2e_asr_conformer import E2E
        espnet_amd.set_precision("fp32")
        T = 1000
        g = torch.Generator().manual_seed(11)
        xs = torch.randn(B, T, 80, generator=g)
        ilens = [T - 13 * i for i in range(B)]
        for i, n in enumerate(ilens):
            xs[i, n:] = 0.0
        xd = xs.to(dev)
        for flag in (False, True):
            torch.manual_seed(0)
            args = bench.c2_args(0.0)
            args.report_cer = args.report_wer = flag
            args.char_list = tokens
            model = E2E(80, V, args).to(dev).eval()

            def fwd():
                with torch.no_grad():
                    model(xd, ilens, ys_d)
            res["eval_forward_ms_report_%s" % ("on" if flag else "off")] = round(timed(fwd, 5), 2)
            del model
        res["report_share_of_eval_forward"] = round(
            1.0 - res["eval_forward_ms_report_off"] / res["eval_forward_ms_report_on"], 4)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
