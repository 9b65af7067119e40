"""The float64 restatement of the batched greedy transducer search (tests/rnnt_greedy_restatement.py) against the REFERENCE, on
the CPU: with the recorded weights and encoder states of utterance 0 (full length, dropout 0) it must return the greedy
hypothesis the reference recorded - tokens exactly, score within 1e-4 relative (the bound of the transducer decoding tests).
That pins the yardstick of tests/test_gpu_rnnt_greedy.py to the reference before any GPU is involved."""
import numpy as np
import pytest

from conftest import load_golden, split_golden
from rnnt_greedy_restatement import greedy_batch64, weights_from_state_dict


@pytest.mark.parametrize("name", ["transducer_rnn.npz", "transducer_gru.npz"])
def test_restatement_reproduces_the_reference_greedy_search(name):
    p, sd, _ = split_golden(load_golden(name))
    w = weights_from_state_dict({k: np.asarray(v) for k, v in sd.items()})
    hs = np.asarray(p["hs_pad"])[:1]
    got = greedy_batch64(w, hs, None, act="tanh")
    n = int(p["dec_greedy_lens"][0])
    want_y = [int(v) for v in np.asarray(p["dec_greedy_yseq"])[:n]]
    want_s = float(np.asarray(p["dec_greedy_scores"])[0])
    assert got["yseq"][0] == want_y
    assert abs(got["score"][0] - want_s) <= 1e-4 * max(1.0, abs(want_s)), (got["score"][0], want_s)
    assert got["n_emit"][0] == n - 1 and got["n_blank"][0] + got["n_emit"][0] == hs.shape[1]
    # rows past their length decide nothing: the same utterance cut to half its frames keeps the hypothesis of those frames
    half = hs.shape[1] // 2
    cut = greedy_batch64(w, hs, [half], act="tanh")
    assert cut["yseq"][0] == greedy_batch64(w, hs[:, :half], None, act="tanh")["yseq"][0]
    assert cut["n_blank"][0] + cut["n_emit"][0] == half
