"""CTC segmentation (Kuerzinger et al. 2020) restated in NumPy, cell by cell and in the order the recursion is written down:
the windowed trellis, its backpointers, the walk back and the utterance segments.  `dtype` is the type every table value and
every sum is formed in (np.float32: what the kernel computes; np.float64: the reference the tests compare against).
Unreachable cells are -inf.  Not a product module: the tests import it, espnet_amd does not."""
import numpy as np

OK, NO_PATH = 0, 1


def trellis(lpz, gt, blank=0, window=8000, dtype=np.float64, gratis_blank=False):
    """lpz [T,V] log-probabilities, gt [L,S] token index of the span ending at each character (-1: none)
    -> dict(status, offsets [L], bp [W,L] uint8, end_row, best, timings [L] frames, char_probs [T], states [T], table_last)"""
    lpz = np.asarray(lpz).astype(dtype)
    gt = np.asarray(gt)
    T, (L, S) = lpz.shape[0], gt.shape
    W = min(int(window), T)
    ninf = dtype(-np.inf)
    if gratis_blank:                         # the blank column reads as 0 everywhere below
        lpz[:, blank] = 0
    lpb = lpz[:, blank]
    table = np.full((W, L), ninf, dtype)
    table[0, 0] = 0
    bp = np.zeros((W, L), np.uint8)
    offsets = np.zeros(L, np.int64)
    higher = int((T - W) / float(L)) + 1
    off = osum = 0
    cur = [-1] * S
    last_arg = 0
    for c in range(L):
        if c > 0:
            off = min(max(0, last_arg - W // 2), min(higher, (T - W) - osum))
            for s in range(S - 1):
                cur[s + 1] = cur[s] + off
            cur[0] = off
            osum += off
        offsets[c] = osum
        first = 1 if c == 0 else 0
        for t in range(first, W):
            sw = mx = ninf
            sb = 0
            for s in range(S):
                g = gt[c, s]
                if g == -1:
                    continue
                e = lpz[t + osum, g]
                if c == 0 or c - 1 - s < 0 or t - 1 + cur[s] < 0 or t >= W - (cur[s] - 1):
                    p = ninf
                else:
                    p = dtype(table[t - 1 + cur[s], c - 1 - s] + e)
                if p > sw:
                    sw, sb = p, s
                if e > mx:
                    mx = e
            st = ninf if t == 0 else dtype(table[t - 1, c] + max(lpb[t + osum], mx))
            if st >= sw:
                table[t, c], bp[t, c] = st, 0
            else:
                table[t, c], bp[t, c] = sw, 1 + sb
        col = table[first:, c]
        last_arg = first + (int(np.argmax(col)) if col.size else 0)
    end_row = int(np.argmax(table[:, L - 1]))
    best = table[end_row, L - 1]
    out = dict(status=OK if np.isfinite(best) else NO_PATH, offsets=offsets, bp=bp, end_row=end_row, best=best, W=W,
               timings=np.zeros(L, np.int64), char_probs=np.zeros(T, dtype), states=np.full(T, -2, np.int64))
    if out["status"] != OK:
        return out
    t, c = end_row, L - 1
    tm, cp, stt = out["timings"], out["char_probs"], out["states"]
    while (t, c) != (0, 0):
        assert 0 <= t < W and c >= 0, (t, c)
        f = offsets[c] + t
        mx = ninf
        if c > 0:
            for s in range(S):
                if gt[c, s] != -1:
                    mx = max(mx, lpz[f, gt[c, s]])
        if bp[t, c]:
            s = int(bp[t, c]) - 1
            for k in range(s + 1):
                tm[c - k] = f
            cp[f] = mx
            stt[f] = gt[c, s]
            d = offsets[c] - (offsets[c - 1 - s] if c - s > 0 else 0)
            c -= 1 + s
            t -= 1 - d
        else:
            cp[f] = max(lpb[f], mx)
            stt[f] = -1
            t -= 1
    return out


def path_score(lpz, gt, blank, timings, states, gratis_blank=False):
    """float64 score of a returned path, summed along it frame by frame, after checking that it is a valid monotone path
    through gt: frames 1 .. end on the path and no others, every switch a token gt[c, s] that ends at the character it moves to,
    timings the frame each character was entered at, the last character reached.  AssertionError otherwise."""
    lpz = np.asarray(lpz, np.float64).copy()
    if gratis_blank:
        lpz[:, blank] = 0
    gt, timings, states = np.asarray(gt), np.asarray(timings), np.asarray(states)
    L, S = gt.shape
    on = np.nonzero(states != -2)[0]
    if L == 1 and on.size == 0:
        return 0.0
    assert on.size and on[0] == 1 and on[-1] == on.size, "path frames are not 1 .. end"
    c, score = 0, 0.0
    for f in on:
        if states[f] == -1:
            mx = max([lpz[f, g] for g in gt[c] if g != -1], default=-np.inf) if c > 0 else -np.inf
            score += max(lpz[f, blank], mx)
        else:
            fits = [s for s in range(S) if c + 1 + s < L and gt[c + 1 + s, s] == states[f]
                    and np.all(timings[c + 1:c + 2 + s] == f)]
            assert fits, "frame %d: token %d does not continue the text behind character %d" % (f, states[f], c)
            c += 1 + fits[0]
            score += lpz[f, states[f]]
    assert c == L - 1, "the path ends at character %d of %d" % (c, L)
    assert np.all(np.diff(timings) >= 0)
    return score


def segments(utt_begin, char_probs, timings_sec, index_duration, n):
    """timings in seconds -> [(start, end, confidence)] per utterance, in float64"""
    tm = np.asarray(timings_sec, np.float64)
    cp = np.asarray(char_probs, np.float64)
    res = []
    for i in range(len(utt_begin) - 1):
        b, e = utt_begin[i], utt_begin[i + 1]
        start = max(tm[b + 1] - 0.5, (tm[b] + tm[b - 1]) / 2)
        end = min(tm[e - 1] + 0.5, (tm[e] + tm[e - 1]) / 2)
        a, z = int(round(start / index_duration)), int(round(end / index_duration))
        if z <= a:
            conf = -np.inf
        elif z - a <= n:
            conf = cp[a:z].mean()
        else:
            conf = min(0.0, min(cp[t:t + n].mean() for t in range(a, z - n)))
        res.append((float(start), float(end), float(conf)))
    return res


def segment(lpz, gt, utt_begin, blank=0, min_window=8000, max_window=100000, index_duration=0.01, n=30, dtype=np.float64,
            gratis_blank=False):
    """window doubling around trellis() + segments(): -> (result dict with 'segments', 'window', 'passes')"""
    window, passes = int(min_window), 0
    while True:
        r = trellis(lpz, gt, blank, window, dtype, gratis_blank)
        passes += 1
        if r["status"] == OK:
            break
        window *= 2
        if window >= max_window:
            raise AssertionError("no path up to the largest window")
    r["segments"] = segments(utt_begin, r["char_probs"], r["timings"] * index_duration, index_duration, n)
    r["window"], r["passes"] = window, passes
    return r
