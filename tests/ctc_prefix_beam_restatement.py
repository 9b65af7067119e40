"""Support for the CTC prefix beam search tests (not collected: no test_ prefix): the definition of
espnet_amd/nets/ctc_prefix_beam.py restated in float64 on a dictionary {prefix tuple: (pb, pnb)}, the exact CTC sequence
log-probability, the n-gram LM term restated from an ARPA file as tests/test_ngram.py restates rows, and the seeded generator
of peaked posteriors the GPU tests use."""
import math

import numpy as np
import torch

from test_ngram import arpa_dict, definition

NEG = -math.inf


def lae(a, b):
    return float(np.logaddexp(a, b))


def ctc_log_prob(logp, y, blank=0):
    """exact log p(y | x) of the CTC forward recursion in float64.  logp [T, V], y: label ids"""
    logp = np.asarray(logp, dtype=np.float64)
    ext = [blank]
    for c in y:
        ext += [int(c), blank]
    S = len(ext)
    alpha = np.full(S, NEG)
    alpha[0] = logp[0, blank]
    if S > 1:
        alpha[1] = logp[0, ext[1]]
    for t in range(1, logp.shape[0]):
        new = np.full(S, NEG)
        for s in range(S):
            a = alpha[s]
            if s >= 1:
                a = lae(a, alpha[s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                a = lae(a, alpha[s - 2])
            new[s] = a + logp[t, ext[s]]
        alpha = new
    return lae(alpha[S - 1], alpha[S - 2]) if S > 1 else float(alpha[0])


class ArpaDefinition:
    """log10 p(token | <s> + prefix) of an ARPA file by the back-off definition in float64 (tests/test_ngram.py: definition).
    tokens: the token list (<eos> reads </s>; a token the file does not list reads <unk>)"""

    def __init__(self, path, tokens):
        self.grams, self.order = arpa_dict(path)
        self.words = ["</s>" if t == "<eos>" else t for t in tokens]
        self.memo = {}

    def __call__(self, prefix, tok):
        hist = (("<s>",) + tuple(self.words[c] for c in prefix))[-(self.order - 1):] if self.order > 1 else ()
        key = (hist, tok)
        if key not in self.memo:
            self.memo[key] = definition(self.grams, self.order, hist, self.words[tok])[0]
        return self.memo[key]


def candidates(row, K):
    """the K largest of row[1 .. V-2], equal values to the lower id -> token ids"""
    x = np.asarray(row[1:-1])
    return [int(i) + 1 for i in np.argsort(-x, kind="stable")[:K]]


def prefix_beam_search(logp, W, K, nbest, penalty=0.0, lm=None, ngram_weight=0.0, track=None):
    """logp [T, V] (any float dtype; worked on in float64), lm: callable (prefix tuple, token) -> log10 p
    -> (n-best [(score, prefix tuple, logaddexp(pb, pnb))], beam margin, n-best margin): the smallest gap over the frames between
    the W-th and the (W+1)-th ranked entry, and the smallest gap between neighbours of the final n-best (inf where there is none).
    track: a dict that receives "recreated_parent_merges", counted with the node-id bookkeeping of csrc/ctc_beam.hip (a prefix
    gets a fresh id whenever it enters the beam and remembers the id its parent had then): the (frame, prefix j) pairs where
    last(j) is a candidate, the string parent(j) is in the beam, but under another id than the one j remembers - the merges
    that the kernel can only find by comparing the parent chains token by token"""
    logp = np.asarray(logp, dtype=np.float64)
    T, V = logp.shape
    beam = {(): (0.0, NEG)}
    lmsum = {(): 0.0}
    beam_margin = math.inf
    node_id, parent_id, next_id, recreated = {(): 0}, {(): -1}, 1, 0

    def rank_score(l, pb, pnb):
        return lae(pb, pnb) + (ngram_weight * lmsum[l] if lm is not None else 0.0) + penalty * len(l)

    for t in range(T):
        cand = candidates(logp[t], K)
        new = {}
        recreated += sum(1 for j in beam if j and j[-1] in cand and j[:-1] in beam and node_id[j[:-1]] != parent_id[j])

        def add(l, dpb, dpnb):
            pb, pnb = new.get(l, (NEG, NEG))
            new[l] = (lae(pb, dpb), lae(pnb, dpnb))

        for l, (pb, pnb) in beam.items():
            tot = lae(pb, pnb)
            add(l, tot + logp[t, 0], NEG)
            for c in cand:
                lc = l + (c,)
                if lm is not None and lc not in lmsum:
                    lmsum[lc] = lmsum[l] + lm(l, c)
                if l and c == l[-1]:
                    add(l, NEG, pnb + logp[t, c])
                    add(lc, NEG, pb + logp[t, c])
                else:
                    add(lc, NEG, tot + logp[t, c])
        ranked = sorted(((rank_score(l, *v), l) for l, v in new.items() if lae(*v) > NEG), key=lambda x: -x[0])
        if len(ranked) > W:
            beam_margin = min(beam_margin, ranked[W - 1][0] - ranked[W][0])
        kept = [l for _, l in ranked[:W]]
        ids, pars = {}, {}
        for l in kept:
            if l in beam:
                ids[l], pars[l] = node_id[l], parent_id[l]
            else:                                    # enters the beam: a fresh node under the parent's present id
                ids[l], pars[l], next_id = next_id, node_id[l[:-1]], next_id + 1
        node_id, parent_id = ids, pars
        beam = {l: new[l] for l in kept}
    final = []
    for l, (pb, pnb) in beam.items():
        s = rank_score(l, pb, pnb)
        if lm is not None:
            s += ngram_weight * lm(l, V - 1)
        final.append((s, l, lae(pb, pnb)))
    final.sort(key=lambda x: -x[0])
    if track is not None:
        track["recreated_parent_merges"] = recreated
    nbest_margin = min([a[0] - b[0] for a, b in zip(final[:nbest], final[1:nbest + 1])], default=math.inf)
    return final[:nbest], beam_margin, nbest_margin


def peaked_posteriors(seed, B, T, V, peak=6.0, constant=False):
    """fp32 log-softmax rows [B, T, V] of N(0, 1) logits with up to +peak (constant: exactly +peak) on one class per frame, the
    blank 60 % of the time: posteriors as a trained CTC model gives them, so that beams are decided by more than rounding"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g)
    tok = torch.randint(1, V - 1, (B, T), generator=g)
    cls = torch.where(torch.rand(B, T, generator=g) < 0.6, torch.zeros_like(tok), tok)
    amp = torch.full((B, T), float(peak)) if constant else peak * torch.rand(B, T, generator=g)
    x.scatter_add_(2, cls.unsqueeze(-1), amp.unsqueeze(-1))
    return torch.log_softmax(x, dim=-1)
