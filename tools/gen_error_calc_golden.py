#!/usr/bin/env python3
"""tests/golden/error_calc.npz by RUNNING THE REFERENCE's ErrorCalculator (espnet/nets/e2e_asr_common.py:103-246, CPU).

Two token lists:
  char  single characters (one non-ASCII) + <blank> <unk> <space> <eos>
  bpe   multi-character pieces, two of them non-ASCII, no <space> in the list (idx_space is None)
For each list a seeded batch of references `{list}_ys_pad` [B, L] (-1 padding; row 3 is empty, the others are not), a
teacher-forced style hypothesis batch `{list}_att_hat` [B, L + 1] (always longer than ymax; holds repeats, blanks and, for the
char list, leading / trailing / double spaces) and a frame-level CTC hypothesis batch `{list}_ctc_hat` [B, T] (runs of equal
ids, blanks between them).  Recorded from the reference, called on the whole batch:
  {list}_cer, {list}_wer       ErrorCalculator(report_cer=True, report_wer=True)(att_hat, ys_pad)
  {list}_cer_ctc               the same object with is_ctc=True on ctc_hat
and, from the reference called on one utterance at a time with editdistance.eval wrapped by a recorder, the per-utterance
  {list}_char_ed / _char_len, {list}_word_ed / _word_len, {list}_ctc_ed / _ctc_len      int32 [B]
(ctc_ed is 0 where the reference skips the utterance: empty reference).  `{list}_tokens` is the token list.
The missing editdistance package is the textbook DP of oracle/gen_golden.install_stubs.
Usage: python tools/gen_error_calc_golden.py [--ref /root/reference] [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gen_golden import install_stubs, save  # noqa: E402

SPACE, BLANK = "<space>", "<blank>"
CHAR_LIST = [BLANK, "<unk>", SPACE] + list("abcdefgh") + ["'", "é", "<eos>"]
BPE_LIST = [BLANK, "<unk>", "▁he", "llo", "▁wor", "ld", "▁a", "ing", "▁ñu", "日本", "s", "▁",
            "<eos>"]
B, L, T = 6, 12, 30


def draw(tokens, seed):
    """-> ys_pad [B, L], att_hat [B, L+1], ctc_hat [B, T] (int64)"""
    rng = np.random.default_rng(seed)
    V = len(tokens)
    space = tokens.index(SPACE) if SPACE in tokens else None
    plain = [i for i in range(V) if i not in (0, space, V - 1)]
    ys_pad = np.full((B, L), -1, np.int64)
    att = np.zeros((B, L + 1), np.int64)
    ctc = np.zeros((B, T), np.int64)
    for b in range(B):
        n = [L, 7, 9, 0, 5, 1][b]
        y = list(rng.choice(plain, n))
        if space is not None and n >= 5:
            y[2] = space
            if b == 1:
                y[0] = space                   # leading space
            if b == 2:
                y[-1] = space                  # trailing space
                y[3] = space                   # double space
        ys_pad[b, :n] = y
        # teacher-forced style hypothesis: the reference with substitutions, a blank, a repeat; then <eos> and noise past ymax
        h = list(y) + [V - 1] + list(rng.choice(plain, L + 1))
        h = h[: L + 1]
        for i in range(min(n, L + 1)):
            r = rng.random()
            if r < 0.15:
                h[i] = int(rng.choice(plain))
            elif r < 0.25:
                h[i] = 0
            elif r < 0.35 and i > 0:
                h[i] = h[i - 1]
            elif r < 0.42 and space is not None:
                h[i] = space
        att[b] = h
        # frame-level hypothesis: every label held for 1-3 frames, sometimes a blank between labels, some labels wrong
        f = []
        for tok in y:
            if rng.random() < 0.2:
                tok = int(rng.choice(plain))
            f += [tok] * int(rng.integers(1, 4))
            if rng.random() < 0.4:
                f += [0] * int(rng.integers(1, 3))
        f = (f + [0] * T)[:T]
        ctc[b] = f
    return ys_pad, att, ctc


class Recorder:
    """wraps editdistance.eval: keeps (distance, len(reference)) of every call"""

    def __init__(self, mod):
        self.mod, self.inner, self.calls = mod, mod.eval, []

    def __enter__(self):
        self.mod.eval = self
        return self

    def __exit__(self, *a):
        self.mod.eval = self.inner

    def __call__(self, a, b):
        d = self.inner(a, b)
        self.calls.append((int(d), len(b)))
        return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    install_stubs()
    sys.path.insert(0, args.ref)
    import editdistance
    from espnet.nets.e2e_asr_common import ErrorCalculator

    out = {}
    for name, tokens, seed in (("char", CHAR_LIST, 11), ("bpe", BPE_LIST, 12)):
        ys_pad, att, ctc = draw(tokens, seed)
        ec = ErrorCalculator(tokens, SPACE, BLANK, report_cer=True, report_wer=True)
        assert (ec.idx_space is None) == (name == "bpe")
        tp, ta, tc = torch.from_numpy(ys_pad), torch.from_numpy(att), torch.from_numpy(ctc)
        cer, wer = ec(ta, tp)
        cer_ctc = ec(tc, tp, is_ctc=True)
        per = {k: np.zeros(B, np.int32) for k in ("char_ed", "char_len", "word_ed", "word_len", "ctc_ed", "ctc_len")}
        for b in range(B):
            with Recorder(editdistance) as rec:
                try:
                    ec(ta[b:b + 1], tp[b:b + 1])
                except ZeroDivisionError:        # the empty reference alone: the distances were taken before the division
                    pass
            # calculate_cer runs before calculate_wer; with a zero length the first division already raised
            per["char_ed"][b], per["char_len"][b] = rec.calls[0]
            if len(rec.calls) > 1:
                per["word_ed"][b], per["word_len"][b] = rec.calls[1]
            else:
                assert rec.calls[0][1] == 0
            with Recorder(editdistance) as rec:
                ec(tc[b:b + 1], tp[b:b + 1], is_ctc=True)
            if rec.calls:
                per["ctc_ed"][b], per["ctc_len"][b] = rec.calls[0]
        assert per["char_len"][3] == 0 and (per["char_len"][[0, 1, 2, 4, 5]] > 0).all()
        assert cer == float(per["char_ed"].sum()) / per["char_len"].sum()
        assert wer == float(per["word_ed"].sum()) / per["word_len"].sum()
        assert cer_ctc == float(per["ctc_ed"].sum()) / per["ctc_len"].sum()
        out.update({f"{name}_tokens": np.array(tokens), f"{name}_ys_pad": ys_pad, f"{name}_att_hat": att,
                    f"{name}_ctc_hat": ctc, f"{name}_cer": np.float64(cer), f"{name}_wer": np.float64(wer),
                    f"{name}_cer_ctc": np.float64(cer_ctc)})
        out.update({f"{name}_{k}": v for k, v in per.items()})
        print(name, "cer", cer, "wer", wer, "cer_ctc", cer_ctc, {k: v.tolist() for k, v in per.items()})
    out["sym_space"], out["sym_blank"] = np.array(SPACE), np.array(BLANK)
    save(os.path.join(args.out, "error_calc.npz"), **out)


if __name__ == "__main__":
    main()
