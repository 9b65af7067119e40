"""CTC segmentation on the GPU (csrc/ctc_segment.hip through ops.ctc_segment_*, nets.ctc_segmentation, CTC.segment,
nets.ctc_align.ctc_segment_recordings) against the float64 NumPy restatement of tests/ctc_segmentation_restatement.py.

Grid form: log-probabilities rounded to multiples of 1/64.  With T * max|lp| * 64 < 2^24 every sum the recursion forms is exact
in fp32 in any order of association, so the kernel's block scan must reproduce the float64 restatement exactly: offsets, end
frame, timings, states, char_probs bit for bit, segment bounds equal, confidence within 1e-6 relative (one division).  Ties are
frequent on the grid, which exercises the first-maximum rules.  Real-valued inputs: the scan re-associates the additions, so the
returned path is checked to be a valid path whose float64 score is within the a-priori bound of the restatement's best."""
import functools

import numpy as np
import pytest
import torch

import ctc_segmentation_restatement as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHARS3 = ["<b>", "a", "b", "c", "d", "e", "ab", "cd", "abc", "f", "g", "h"]
CHARS1 = ["_", "a", "b", "c", "d", "e", "f", "g", "h"]                      # S = 1: the blank symbol is one character too
CHARS_B3 = ["a", "b", "c", "<b>", "d", "e", "ab", "cd", "abc", "f", "g", "h"]


def config_for(chars, window, blank=0, gratis=False, **kw):
    from espnet_amd.nets.ctc_segmentation import CtcSegmentationParameters
    return CtcSegmentationParameters(char_list=chars, min_window_size=window, blank=blank, blank_transition_cost_zero=gratis, **kw)


@functools.lru_cache(maxsize=None)
def generate(seed, T=300, nutt=5, grid=True, chars=tuple(CHARS3), blank=0, late=0):
    """-> (text, gt [L,S], utt_begin, lp [T,12] fp32): a transcript of random letters and log-posteriors with a bump at a random
    frame for every character.  The order of the draws is fixed.  late: nothing but blank before that frame, so that the path
    runs through the upper rows of a large window."""
    from espnet_amd.nets.ctc_segmentation import prepare_text
    rng = np.random.default_rng(seed)
    text = []
    for _ in range(nutt):
        n = rng.integers(4, 9)
        text.append("".join(rng.choice(list("abcdefgh"), n)) + "\n")
    gt, begins = prepare_text(config_for(list(chars), 96, blank), text)
    L = gt.shape[0]
    pos = np.sort(rng.choice(np.arange(3, T - 3), L - 1, replace=False))
    z = rng.normal(0, 2, (T, 12))
    z[:, blank] += 4
    for i in range(L - 1):
        z[pos[i], gt[i + 1, 0]] += 8
    lp = torch.log_softmax(torch.from_numpy(z.astype(np.float32)), -1).numpy()
    if grid:
        lp = (np.round(lp * 64) / 64).astype(np.float32)
        assert T * np.abs(lp).max() * 64 < 2 ** 24
    if late:
        lp[:late, np.arange(12) != blank] = -np.inf
    lp.setflags(write=False)
    return text, gt, begins, lp


@functools.lru_cache(maxsize=None)
def restated(seed, window, T=300, nutt=5, grid=True, chars=tuple(CHARS3), blank=0, gratis=False, late=0):
    """the float64 restatement of one generated recording at one window (computed once, shared, not modified)"""
    text, gt, begins, lp = generate(seed, T, nutt, grid, chars, blank, late)
    r = R.trellis(lp, gt, blank, window, np.float64, gratis)
    if r["status"] == R.OK:
        r["segments"] = R.segments(begins, r["char_probs"], r["timings"] * 0.01, 0.01, 30)
    return r


def device_run(cfg, lps, gts, utts, ring_global=False, guards=False):
    """one window attempt at cfg.min_window_size for a batch, through ops -> dict of host arrays (all results, one copy)"""
    from espnet_amd import ops
    from espnet_amd.nets.ctc_segmentation import _plan
    B, lens = len(lps), [lp.shape[0] for lp in lps]
    Tmax, V = max(lens), lps[0].shape[1]
    pad = np.full((B, Tmax, V), np.nan, np.float32)                # NaN behind each recording: never to be read
    for b, lp in enumerate(lps):
        pad[b, :lens[b]] = lp
    tok, gtu, llens, utt, nutt = _plan(cfg, lens, gts, utts, V, 1 << 30)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    lens_d, tok_d = up(np.asarray(lens, np.int32)), up(tok)
    em = ops.ctc_segment_emissions(up(pad), lens_d, tok_d, cfg.blank, cfg.blank_transition_cost_zero)
    Lmax, S, NU = gtu.shape[1], gtu.shape[2], utt.shape[1] - 1
    window = cfg.min_window_size
    nbytes = ops.ctc_segment_workspace_layout(B, B, Tmax, Lmax, S, window, ring_global)[3]
    rbytes = ops.ctc_segment_result_bytes(B, Tmax, Lmax, NU)
    G = 256
    out_big = torch.full((rbytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    ws_big = torch.full((nbytes + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    res = ops.ctc_segment_result(B, Tmax, Lmax, NU, DEV, out=out_big[G:G + rbytes])
    ops.ctc_segment_run(em, up(gtu), tok_d, lens_d, up(llens), up(np.arange(B, dtype=np.int32)), up(utt), up(nutt), res, window,
                        cfg.score_min_mean_over_L, cfg.index_duration_in_seconds, ring_global=ring_global,
                        workspace=ws_big[G:G + nbytes])
    host = ops.ctc_segment_fetch(res, full=True)
    if guards:
        for big, n in ((out_big, rbytes), (ws_big, nbytes)):
            g = big.cpu().numpy()
            assert (g[:G] == 0xA5).all() and (g[G + n:] == 0xA5).all()
    return host


def check_exact(host, b, r, begins, T):
    """recording b of a device result against the float64 restatement r, exactly"""
    L = r["offsets"].size
    info = host["info"][b]
    assert info[0] == r["status"] == R.OK, info
    assert info[1] == r["end_row"] and info[2] == r["W"] and info[3] == r["offsets"][-1]
    assert host["offsets"][b, :L].tolist() == r["offsets"].tolist()
    assert host["timings"][b, :L].tolist() == r["timings"].tolist()
    assert host["states"][b, :T].tolist() == r["states"].tolist()
    assert np.array_equal(host["char_probs"][b, :T].astype(np.float64), r["char_probs"])
    assert (host["timings"][b, L:] == 0).all() and (host["offsets"][b, L:] == 0).all()
    assert (host["states"][b, T:] == -2).all() and (host["char_probs"][b, T:] == 0).all()
    n = len(begins) - 1
    for i, (start, end, conf) in enumerate(r["segments"]):
        s = host["seg"][b, i]
        assert s[0] == start and s[1] == end, (i, s, start, end)
        assert s[2] == conf or abs(s[2] - conf) <= 1e-6 * abs(conf), (i, s[2], conf)
    assert (host["seg"][b, n:] == 0).all()


# ---- 1. grid form, seeds 0-7, window 96: exact, with the ring of columns in LDS and in global memory -------------------------
@pytest.mark.parametrize("ring_global", [False, True])
@pytest.mark.parametrize("seed", range(8))
def test_exact_on_the_grid(seed, ring_global):
    text, gt, begins, lp = generate(seed)
    r = restated(seed, 96)
    host = device_run(config_for(CHARS3, 96), [lp], [gt], [begins], ring_global=ring_global, guards=True)
    check_exact(host, 0, r, begins, lp.shape[0])
    print(f"[parity] ctc segmentation seed {seed} ring_global={ring_global}: L={gt.shape[0]} end frame "
          f"{r['end_row'] + r['offsets'][-1]} last offset {r['offsets'][-1]} exact")


# ---- 2. the shapes at which the kernel takes another path ---------------------------------------------------------------------
SHAPES = {
    "window_not_multiple_of_64": dict(window=70),
    "several_rows_per_thread": dict(T=3000, window=2500, nutt=8),
    "several_rows_per_thread_late": dict(T=3000, window=2500, nutt=8, late=2300),
    "several_tiles_per_column": dict(T=9000, window=8500, chars=tuple(CHARS1), late=8300),      # > 1024 threads x 8 rows
    "window_covers_recording": dict(window=400),
    "window_one_short": dict(window=299),
    "single_character_tokens": dict(window=96, chars=tuple(CHARS1)),
    "blank_3": dict(window=96, chars=tuple(CHARS_B3), blank=3),
    "gratis_blank": dict(window=96, gratis=True),
    "tiny_window": dict(window=9, T=60, nutt=1),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_shapes(name):
    kw = dict(T=300, nutt=5, chars=tuple(CHARS3), blank=0, gratis=False, late=0)
    kw.update(SHAPES[name])
    window, gratis = kw.pop("window"), kw.pop("gratis")
    text, gt, begins, lp = generate(3, kw["T"], kw["nutt"], True, kw["chars"], kw["blank"], kw["late"])
    r = restated(3, window, kw["T"], kw["nutt"], True, kw["chars"], kw["blank"], gratis, kw["late"])
    cfg = config_for(list(kw["chars"]), window, kw["blank"], gratis)
    for ring_global in (False, True):
        host = device_run(cfg, [lp], [gt], [begins], ring_global=ring_global, guards=True)
        if r["status"] == R.NO_PATH:
            assert host["info"][0, 0] == R.NO_PATH
        else:
            check_exact(host, 0, r, begins, lp.shape[0])
    print(f"[parity] ctc segmentation {name}: T={kw['T']} W={r['W']} L={gt.shape[0]} S={gt.shape[1]} status {r['status']} exact")


def test_exact_batch_of_three_with_guards():
    cases = [(0, 300, 5), (1, 260, 3), (2, 200, 4)]
    gens = [generate(s, T, n) for s, T, n in cases]
    host = device_run(config_for(CHARS3, 96), [g[3] for g in gens], [g[1] for g in gens], [g[2] for g in gens], guards=True)
    for b, (s, T, n) in enumerate(cases):
        check_exact(host, b, restated(s, 96, T, n), gens[b][2], T)


# ---- 3. window doubling: the recording without a path is run again alone, the other keeps its result --------------------------
def test_window_doubling():
    from espnet_amd.nets.ctc_segmentation import ctc_segment_batch
    text0, gt0, begins0, lp0 = generate(0)
    text1, gt1, begins1, lp1 = generate(1)
    lp0 = lp0.copy()
    lp0[:200, 1:] = -np.inf
    for w in (32, 64, 128):
        assert R.trellis(lp0, gt0, 0, w)["status"] == R.NO_PATH
    r0 = R.segment(lp0, gt0, begins0, 0, 32, 100000, 0.01, 30)
    assert r0["window"] == 256 and r0["passes"] == 4 and r0["offsets"][-1] == 44 and r0["timings"][2] == 203
    cfg = config_for(CHARS3, 32)
    pad = torch.from_numpy(np.stack([lp0, lp1])).to(DEV)
    alone = ctc_segment_batch(cfg, pad[1:], [300], [text1])
    passes_alone, window_alone = ctc_segment_batch.passes, ctc_segment_batch.windows[0]
    both = ctc_segment_batch(cfg, pad, [300, 300], [text0, text1])
    assert ctc_segment_batch.passes == 4 and ctc_segment_batch.host_reads == 4
    assert ctc_segment_batch.windows == [256, window_alone] and passes_alone <= 4
    assert both[1] == alone[0]
    r1 = R.segment(lp1, gt1, begins1, 0, 32, 100000, 0.01, 30)
    assert r1["window"] == window_alone
    for got, want in ((both[0], r0["segments"]), (both[1], r1["segments"])):
        assert len(got) == len(want) == 5
        for (s, e, c), (rs, re_, rc) in zip(got, want):
            assert s == rs and e == re_ and abs(c - rc) <= 1e-6 * abs(rc)
    with pytest.raises(RuntimeError, match="max_window_size"):
        ctc_segment_batch(config_for(CHARS3, 32, max_window_size=128), pad, [300, 300], [text0, text1])


# ---- 4. real-valued log-posteriors: a valid path, as good as the float64 best up to the a-priori bound -------------------------
def test_real_valued_paths():
    from espnet_amd.nets.ctc_segmentation import prepare_text
    cases = [("seed %d" % k,) + generate(k, grid=False)[1:] + (CHARS3, 96) for k in range(8)]
    cfg = config_for(["•", "a", "c", "d", "g", "o", "s", "t"], 20)
    gt, begins = prepare_text(cfg, ["catzz#\n", "dogs!!\n"])
    cases.append(("reference lpz", gt, begins, load_golden("ctc_segmentation_lpz.npz")["lpz"], cfg.char_list, 20))
    left_out = []
    for name, gt, begins, lp, chars, window in cases:
        T = lp.shape[0]
        r = R.trellis(lp, gt, 0, window, np.float64)
        host = device_run(config_for(chars, window), [lp], [gt], [begins])
        assert host["info"][0, 0] == r["status"] == R.OK
        if host["offsets"][0].tolist() != r["offsets"].tolist():
            left_out.append(name)
            continue
        score = R.path_score(lp, gt, 0, host["timings"][0], host["states"][0])
        best = float(r["best"])
        bound = 2 * (T + 8) * 2.0 ** -24 * abs(best)
        print(f"[parity] ctc segmentation real-valued {name}: path score {score:.6f} float64 best {best:.6f} bound {bound:.2e}")
        assert score >= best - bound, (name, score, best, bound)
        on = host["states"][0] != -2
        assert np.array_equal(host["char_probs"][0][~on], np.zeros((~on).sum(), np.float32))
    assert len(left_out) <= 1, left_out


def test_package_call_surface_on_the_reference_lpz():
    from espnet_amd.nets.ctc_segmentation import ctc_segmentation, determine_utterance_segments, prepare_text
    lpz = load_golden("ctc_segmentation_lpz.npz")["lpz"]
    cfg = config_for(["•", "a", "c", "d", "g", "o", "s", "t"], 20, max_window_size=50)
    text = ["catzz#\n", "dogs!!\n"]
    gt, begins = prepare_text(cfg, text)
    r = R.segment(lpz, gt, begins, 0, 20, 50, 0.01, 30)
    for arg in (lpz, torch.from_numpy(lpz), torch.from_numpy(lpz).to(DEV)):
        timings, char_probs, state_list = ctc_segmentation(cfg, arg, gt)
        assert np.array_equal(timings, r["timings"] * 0.01) and len(state_list) == 30
        assert np.array_equal(char_probs.astype(np.float64), r["char_probs"])
        names = {-1: "ε", -2: ""}
        assert state_list == [names[s] if s < 0 else cfg.char_list[s] for s in r["states"]]
        seg = determine_utterance_segments(cfg, begins, char_probs, timings, text)
        assert seg == r["segments"]


# ---- 5. model level ------------------------------------------------------------------------------------------------------------
def test_model_level():
    import argparse
    from espnet_amd.espnet2 import CTC as CTC2
    from espnet_amd.nets.ctc_align import ctc_segment_recordings, encode_batch
    from espnet_amd.nets.ctc_segmentation import ctc_segment_batch
    from espnet_amd.nets.e2e_asr_transformer import E2E
    ns = argparse.Namespace(adim=64, aheads=4, elayers=2, eunits=256, dlayers=1, dunits=256, mtlalpha=0.3, lsm_weight=0.1,
                            dropout_rate=0.0, transformer_length_normalized_loss=False)
    torch.manual_seed(0)
    model = E2E(20, 50, ns).to(DEV).eval()
    chars = ["<blank>"] + [chr(ord("a") + i) for i in range(26)] + ["th", "he", "in"] + ["<%d>" % i for i in range(19)] + ["<eos>"]
    assert len(chars) == 50
    cfg = config_for(chars, 48, subsampling_factor=4, score_min_mean_over_L=5)
    g = torch.Generator().manual_seed(7)
    xs = torch.randn(2, 400, 20, generator=g)
    ilens = [400, 330]
    texts = [["the cat\n", "sat in\n", "the hat\n"], ["hello there\n", "thin\n"]]
    got = ctc_segment_recordings(model, xs, ilens, texts, cfg)
    assert ctc_segment_batch.host_reads == 1 and ctc_segment_batch.passes == 1
    hs, hlens = encode_batch(model, xs, ilens)
    with torch.no_grad():
        want = ctc_segment_batch(cfg, model.ctc.log_softmax(hs), hlens, texts)
    assert got == want and [len(s) for s in got] == [3, 2]
    for rec in got:
        for start, end, conf in rec:
            assert 0 <= start < end <= 99 * 0.04 and -np.inf < conf <= 0
    ctc2 = CTC2(50, 64)
    ctc2.ctc_lo.load_state_dict(model.ctc.ctc_lo.state_dict())
    assert ctc2.to(DEV).segment(hs, hlens, texts, cfg) == want
