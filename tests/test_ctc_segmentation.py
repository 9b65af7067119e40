"""CTC segmentation without a GPU (nets.ctc_segmentation): prepare_text and determine_utterance_segments on the vectors of the
reference's test/test_ctc_segmentation.py, the NumPy restatement (tests/ctc_segmentation_restatement.py) on the reference test's
30 x 8 log-posteriors (tests/golden/ctc_segmentation_lpz.npz), the limits that are refused before any launch, the argument
checks of the C entry points, and the segments file format."""
import numpy as np
import pytest
import torch

import ctc_segmentation_restatement as R
from conftest import load_golden
from espnet_amd.nets.ctc_segmentation import (CtcSegmentationParameters, ctc_segment_batch, ctc_segmentation,
                                              determine_utterance_segments, format_segments, prepare_text)

CHARS = ["•", "a", "c", "d", "g", "o", "s", "t"]
TEXT = ["catzz#\n", "dogs!!\n"]


def test_parameters_defaults():
    c = CtcSegmentationParameters()
    assert (c.min_window_size, c.max_window_size, c.subsampling_factor, c.frame_duration_ms, c.score_min_mean_over_L) == \
        (8000, 100000, 1, 10, 30)
    assert (c.blank, c.space, c.self_transition, c.start_of_ground_truth) == (0, "·", "ε", "#")
    assert c.excluded_characters == ".,-?!:»«;'›‹()" and c.replace_spaces_with_blanks and not c.blank_transition_cost_zero
    assert c.char_list is None and c.index_duration_in_seconds == 0.01
    c = CtcSegmentationParameters(subsampling_factor=4, frame_duration_ms=10, char_list=CHARS)
    assert c.index_duration_in_seconds == 0.04 and c.char_list is CHARS
    with pytest.raises(TypeError):
        CtcSegmentationParameters(window=3)


def test_prepare_text_reference_vectors():
    config = CtcSegmentationParameters()
    mat, begins = prepare_text(config, TEXT, CHARS)
    assert begins.tolist() == [1, 5, 10] and mat.shape == (11, 1)
    # "#" is no token; the space symbol reads as the blank token; z and # are not in the list, ! is excluded
    assert mat[:, 0].tolist() == [-1, 0, 2, 1, 7, 0, 3, 5, 4, 6, 0]
    assert config.char_list is CHARS


def test_prepare_text_multi_character_tokens_and_options():
    chars = ["<b>", "a", "b", "ab", "abc", "c", ".", " "]
    config = CtcSegmentationParameters(char_list=chars)
    mat, begins = prepare_text(config, ["ab c.\n", "abc\n"])
    # ground truth: # · a b · c · a b c ·   (the excluded "." is dropped, the inner space becomes one space symbol)
    assert begins.tolist() == [1, 6, 10] and mat.shape == (11, 3)
    assert mat[:, 0].tolist() == [-1, 0, 1, 2, 0, 5, 0, 1, 2, 5, 0]
    assert mat[:, 1].tolist() == [-1, -1, -1, 3, -1, -1, -1, -1, 3, -1, -1]
    assert mat[:, 2].tolist() == [-1] * 9 + [4, -1]
    # spaces kept as the list's own " " token; the line end is no token and is dropped; "." stays excluded
    config = CtcSegmentationParameters(char_list=chars, replace_spaces_with_blanks=False)
    mat, begins = prepare_text(config, ["ab c.\n", "abc\n"])
    assert begins.tolist() == [1, 6, 10]
    assert mat[:, 0].tolist() == [-1, 0, 1, 2, 7, 5, 0, 1, 2, 5, 0]
    # nothing excluded: "." is a character of the text
    config = CtcSegmentationParameters(char_list=chars, excluded_characters="")
    mat, begins = prepare_text(config, ["ab c.\n"])
    assert begins.tolist() == [1, 7] and mat[:, 0].tolist() == [-1, 0, 1, 2, 0, 5, 6, 0]


def test_determine_utterance_segments_reference_vectors():
    config = CtcSegmentationParameters(frame_duration_ms=1000, score_min_mean_over_L=2)
    seg = determine_utterance_segments(config, [1, 4, 9], np.array([-0.5] * 10), np.arange(10) + 0.5, TEXT)
    assert seg == [(2.0, 4.0, -0.5), (5.0, 9.0, -0.5)]
    assert seg == R.segments([1, 4, 9], np.array([-0.5] * 10), np.arange(10) + 0.5, 1.0, 2)
    # an empty frame range scores -inf; a sliding minimum picks the worst run of n frames, capped at 0
    cp = np.array([0.0, -1.0, -4.0, -4.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    seg = determine_utterance_segments(config, [1, 8], cp, np.arange(10) + 0.5, ["x"])
    assert seg == [(2.0, 8.0, -4.0)] and seg == R.segments([1, 8], cp, np.arange(10) + 0.5, 1.0, 2)
    seg = determine_utterance_segments(config, [1, 2], cp, np.array([0.0, 3.0, 3.2, 3.2]), ["x"])
    assert seg[0][2] == -np.inf


def test_restatement_on_the_reference_lpz():
    lpz = load_golden("ctc_segmentation_lpz.npz")["lpz"]
    assert lpz.shape == (30, 8) and lpz.dtype == np.float32
    config = CtcSegmentationParameters(min_window_size=20, max_window_size=50)
    gt, begins = prepare_text(config, TEXT, CHARS)
    r32, r64 = (R.segment(lpz, gt, begins, 0, 20, 50, config.index_duration_in_seconds, 30, dt) for dt in (np.float32, np.float64))
    for r in (r32, r64):
        assert r["status"] == R.OK and r["passes"] == 1 and r["end_row"] == 13
        assert r["offsets"].tolist() == [0] * 10 + [1]
        assert r["timings"].tolist() == [0, 1, 3, 4, 6, 8, 9, 10, 12, 13, 14]
        (s0, e0, c0), (s1, e1, c1) = r["segments"]
        assert (s0, e0, s1, e1) == (0.005, 0.07, 0.07, 0.135)
        assert abs(c0 - -2.643941) < 1e-6 and abs(c1 - -3.258300) < 1e-6
        # the path the walk back returns is a path through the text, and it scores what the table says
        score = R.path_score(lpz, gt, 0, r["timings"], r["states"])
        assert abs(score - float(r64["best"])) < 1e-9
    assert np.array_equal(r32["bp"], r64["bp"]) and np.array_equal(r32["states"], r64["states"])
    # the host segment arithmetic of the product on the restatement's arrays
    seg = determine_utterance_segments(config, begins, r64["char_probs"], r64["timings"] * 0.01, TEXT)
    assert seg == r64["segments"]


def test_restatement_window_doubling():
    lpz = load_golden("ctc_segmentation_lpz.npz")["lpz"].copy()
    lpz[:20, 1:] = -np.inf                        # nothing but blank in the first 20 frames: a window of 8 rows never gets out
    config = CtcSegmentationParameters()
    gt, begins = prepare_text(config, TEXT, CHARS)
    assert R.trellis(lpz, gt, 0, 8)["status"] == R.NO_PATH
    r = R.segment(lpz, gt, begins, 0, 8, 50, 0.01, 30)
    assert r["passes"] == 3 and r["window"] == 32 and r["timings"][2] >= 20
    with pytest.raises(AssertionError):
        R.segment(lpz, gt, begins, 0, 8, 32, 0.01, 30)


def test_limits_are_refused_before_any_launch():
    lpz = torch.zeros(1, 30, 8)
    config = CtcSegmentationParameters(char_list=CHARS, min_window_size=20)
    with pytest.raises(ValueError, match="Audio is shorter than text"):
        ctc_segment_batch(config, lpz[:, :10], [10], [TEXT])
    gt, _ = prepare_text(config, TEXT)
    with pytest.raises(ValueError, match="Audio is shorter than text"):
        ctc_segmentation(config, np.zeros((10, 8), np.float32), gt)
    with pytest.raises(ValueError, match="at most 16"):
        ctc_segmentation(config, np.zeros((30, 8), np.float32), np.full((11, 17), -1, np.int64))
    with pytest.raises(ValueError, match="max_workspace_bytes") as e:
        ctc_segment_batch(config, lpz, [30], [TEXT], max_workspace_bytes=1000)
    from espnet_amd import ops
    assert "needs %d bytes" % ops.ctc_segment_bytes(1, 1, 30, 11, 1, 8, 20) in str(e.value)
    with pytest.raises(ValueError, match="outside"):
        ctc_segment_batch(CtcSegmentationParameters(char_list=CHARS, blank=8), lpz, [30], [TEXT])
    with pytest.raises(ValueError, match="token ids"):
        ctc_segmentation(config, np.zeros((30, 8), np.float32), np.full((11, 1), 8, np.int64))
    with pytest.raises(ValueError, match="valid frames"):
        ctc_segment_batch(config, lpz, [31], [TEXT])


def test_workspace_accounting():
    from espnet_amd import ops
    # backpointers: one byte per (window row, character) and recording; emission rows: U x T floats
    small = ops.ctc_segment_bytes(1, 1, 90000, 50000, 1, 30, 8000)
    assert 8000 * 50000 + 30 * 90000 * 4 <= small < 8000 * 50000 + 30 * 90000 * 4 + 90001 * 8 + 4096
    assert ops.ctc_segment_bytes(32, 32, 90000, 50000, 1, 30, 8000) > 8 << 30        # the batch of 32 is over the default limit
    # S + 1 = 4 columns of 8000 rows fit the LDS, 17 columns do not and go to the workspace
    assert ops.ctc_segment_ring_in_lds(3, 8000, 90000) and not ops.ctc_segment_ring_in_lds(16, 8000, 90000)
    assert ops.ctc_segment_ring_in_lds(16, 100000, 96)                               # the window is cut to the recording
    lay_lds = ops.ctc_segment_workspace_layout(2, 2, 300, 40, 3, 96)
    lay_glb = ops.ctc_segment_workspace_layout(2, 2, 300, 40, 3, 96, ring_global=True)
    assert lay_lds[1] is None and lay_glb[1] is not None and lay_glb[3] > lay_lds[3]


def test_entry_points_check_their_arguments_without_a_gpu():
    from espnet_amd import _lib
    L = _lib.lib()
    p = 4096                                                                         # any non-NULL address: nothing is launched
    assert L.eamd_ctc_segment_emissions(None, p, p, p, 1, 10, 8, 2, 0, 0, None) < 0
    assert L.eamd_ctc_segment_emissions(p, p, p, None, 1, 10, 8, 2, 0, 0, None) < 0
    for B, T, V, U, blank in ((0, 10, 8, 2, 0), (1, 0, 8, 2, 0), (1, 10, 8, 0, 0), (1, 10, 8, 2, 8), (1, 10, 8, 2, -1)):
        assert L.eamd_ctc_segment_emissions(p, p, p, p, B, T, V, U, blank, 0, None) < 0

    def run(ptrs=(p,) * 17, nsel=1, B=1, T=10, Lm=4, S=1, U=2, NU=1, W=8, n=30, idur=0.01):
        return L.eamd_ctc_segment_run(*ptrs, nsel, B, T, Lm, S, U, NU, W, n, idur, 0, None)
    for i in range(17):
        if i != 9:                                                                   # ring may be NULL while it fits the LDS
            assert run(tuple(None if j == i else p for j in range(17))) < 0, i
    for kw in (dict(nsel=0), dict(B=0), dict(nsel=2), dict(T=0), dict(Lm=0), dict(S=0), dict(U=0), dict(NU=0), dict(W=0),
               dict(n=0), dict(idur=0.0)):
        assert run(**kw) < 0, kw
    assert run(S=17) == _lib.EAMD_EUNSUPPORTED
    ring_null = tuple(None if j == 9 else p for j in range(17))
    assert run(ring_null, S=16, T=100000, W=100000) < 0                              # ring outside the LDS: needs its workspace
    assert L.eamd_ctc_segment_ring_in_lds(0, 8) < 0 and L.eamd_ctc_segment_ring_in_lds(17, 8) < 0
    assert L.eamd_ctc_segment_ring_in_lds(1, 0) < 0


def test_format_segments():
    lines = format_segments(["utt_0000", "utt_0001"], "rec1", [(0.005, 0.07, -2.643941112927028), (0.07, 0.135, -np.inf)])
    assert lines == ["utt_0000 rec1 0.01 0.07 -2.643941113", "utt_0001 rec1 0.07 0.14 -inf"]
