#!/usr/bin/env python3
"""tests/golden/ctc_align.npz by RUNNING THE REFERENCE's CTC.forced_align (ctc.py:153-216, PyTorch CPU + numpy).

For each of the three DECODE_R4 utterances (oracle/seeded_weights.py: the Conformer at BASELINE config 2's width, T' = 249 /
159 / 74 encoder frames) and three seeded label sequences per utterance -
  short    5 tokens
  repeats  T'/4 tokens, about one in four equal to the one before it
  tight    L + (adjacent repeats) = T': a single CTC path exists
- the file holds
  u{i}_enc                     reference encoder output [T', 256] fp32
  u{i}_{kind}_label            the labels (int64)
  u{i}_{kind}_align            reference model.ctc.forced_align(enc, label): token per frame (int64 [T'])
  u{i}_{kind}_ids, _lpz        the reference's log-posteriors restricted to blank + the label ids: [T', K] fp32 and the K ids
  u{i}_{kind}_gap              smallest winner-minus-runner-up margin of the Viterbi decisions along the path
  u{i}_{kind}_seed             the seed the labels were drawn from
Every recorded path is checked to be a valid CTC path of its labels, and to be the path of the true CTC lattice (the reference
also lets state 0 read the last state at t - 1); a draw whose margin is below 1e-3 (except for the tight sequences: one path)
is redrawn from the next seed.  Weights and inputs are not stored (both sides build them from oracle/seeded_weights.py).
Usage: python tools/gen_golden_ctc_align.py [--ref /root/reference] [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gen_golden import install_stubs, save  # noqa: E402
import seeded_weights as SW  # noqa: E402

MIN_GAP = 1e-3


def draw_labels(kind, T, odim, seed):
    rng = np.random.default_rng(seed)
    if kind == "short":
        return rng.integers(1, odim - 1, 5)
    if kind == "repeats":
        L, rep = T // 4, 0.25
    else:                                   # tight: L + repeats == T
        r = T // 6
        L = T - r
        while True:
            y = rng.integers(1, odim - 1, L)
            for i in np.sort(rng.choice(np.arange(1, L), r, replace=False)):
                y[i] = y[i - 1]
            if n_repeats(y) == r:               # (an unselected neighbour pair may have become equal by chance)
                return y
    y = rng.integers(1, odim - 1, L)
    for i in range(1, L):
        if rng.random() < rep:
            y[i] = y[i - 1]
    return y


def n_repeats(y):
    return int(np.sum(y[1:] == y[:-1])) if len(y) > 1 else 0


def viterbi_margins(em, ext, blank):
    """true-lattice fp32 Viterbi (the reference's operations) on emissions em [T, S] -> (states, min decision margin)"""
    T, S = em.shape
    skip = np.zeros(S, bool)
    for s in range(2, S):
        skip[s] = ext[s] != blank and ext[s] != ext[s - 2]
    d = np.full(S, -np.inf, np.float32)
    d[0] = em[0, 0]
    if S > 1:
        d[1] = em[0, 1]
    cols, bps = [d.copy()], [np.zeros(S, np.int64)]
    for t in range(1, T):
        c = np.stack([d, np.concatenate([[-np.inf], d[:-1]]), np.where(skip, np.concatenate([[-np.inf, -np.inf], d[:-2]]), -np.inf)])
        k = np.argmax(c, axis=0)
        d = (c[k, np.arange(S)] + em[t]).astype(np.float32)
        cols.append(d.copy())
        bps.append(k)
    end = [S - 1, S - 2][int(np.argmax([d[S - 1], d[S - 2]]))]
    assert np.isfinite(d[end])
    states = [end]
    for t in range(T - 1, 0, -1):
        states.append(states[-1] - int(bps[t][states[-1]]))
    states = states[::-1]
    gaps = [abs(float(d[S - 1]) - float(d[S - 2]))] if np.isfinite(d[S - 1]) and np.isfinite(d[S - 2]) else []
    for t in range(1, T):
        s, prev = states[t], cols[t - 1]
        cand = [prev[s]] + ([prev[s - 1]] if s >= 1 else []) + ([prev[s - 2]] if skip[s] else [])
        cand = sorted([float(v) for v in cand if np.isfinite(v)], reverse=True)
        if len(cand) > 1:
            gaps.append(cand[0] - cand[1])
    return np.asarray(states), (min(gaps) if gaps else np.inf)


def check_valid_path(states, ext):
    S = len(ext)
    assert states[0] in (0, 1) and states[-1] in (S - 1, S - 2), (states[0], states[-1], S)
    for a, b in zip(states[:-1], states[1:]):
        step = b - a
        assert step in (0, 1) or (step == 2 and ext[b] != ext[a] and ext[b] != ext[0]), (a, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    install_stubs()
    sys.path.insert(0, a.ref)
    torch.set_num_threads(8)
    from espnet.nets.pytorch_backend.e2e_asr_conformer import E2E

    spec = SW.DECODE_R4
    odim, blank = spec["odim"], 0
    model = SW.decode_r4_model(E2E)
    rec = {}
    with torch.no_grad():
        for u, x in enumerate(SW.decode_r4_inputs()):
            enc = model.encode(x.numpy())
            T = enc.shape[0]
            rec["u%d_enc" % u] = enc.numpy().astype(np.float32)
            lpz = model.ctc.log_softmax(enc.unsqueeze(0))[0].numpy()
            for kind, seed0 in (("short", 100), ("repeats", 200), ("tight", 300)):
                seed = seed0 + u * 1000
                while True:
                    y = draw_labels(kind, T, odim, seed)
                    if kind == "tight":
                        assert len(y) + n_repeats(y) == T, (len(y), n_repeats(y), T)
                    ext = np.zeros(2 * len(y) + 1, np.int64)
                    ext[1::2] = y
                    states, gap = viterbi_margins(lpz[:, ext], ext, blank)
                    if kind == "tight" or gap >= MIN_GAP:
                        break
                    print("u%d %s seed %d: margin %.2e, redrawn" % (u, kind, seed, gap))
                    seed += 1
                ali = np.asarray(model.ctc.forced_align(enc.unsqueeze(0), y, blank), dtype=np.int64)
                check_valid_path(states, ext)
                assert ali.tolist() == ext[states].tolist(), (u, kind, "reference path is not the true-lattice path")
                ids = np.unique(np.concatenate([[blank], y])).astype(np.int64)
                tag = "u%d_%s" % (u, kind)
                rec[tag + "_label"] = y.astype(np.int64)
                rec[tag + "_align"] = ali
                rec[tag + "_ids"] = ids
                rec[tag + "_lpz"] = lpz[:, ids].astype(np.float32)
                rec[tag + "_gap"] = np.asarray(gap, dtype=np.float64)
                rec[tag + "_seed"] = np.asarray(seed, dtype=np.int64)
                print(tag, "T'=%d L=%d repeats=%d margin %.3e seed %d" % (T, len(y), n_repeats(y), gap, seed), flush=True)
    save(os.path.join(a.out, "ctc_align.npz"), **rec)


if __name__ == "__main__":
    main()
