"""tests/alsd_restatement.py (the float64 restatement the GPU tests of the batched alsd transducer search compare against) pinned
to a literal per-utterance transcription of the reference's loop (espnet/nets/beam_search_transducer.py:349-464 without an LM,
transducer/utils.py:181-203): Python hypothesis objects, sorted(), recombine_hyps returning its input, `final` holding the
objects of A.  The fixtures' encoder output needs the GPU model, so the pin to the reference's recorded n-best lists
(dec_alsd3_*, dec_alsd2_* of tests/golden/transducer_rnn.npz / transducer_gru.npz) happens in tests/test_gpu_rnnt_alsd.py; here
seeded small models are decoded both ways.  Also checked here, on the CPU: every case of the GPU test finds a seed that meets its
preconditions."""
import numpy as np
import pytest

from alsd_restatement import alsd_batch64, alsd_step64, new_finals, new_state
from rnnt_greedy_restatement import act64, pred_step64, seeded_weights, weights_from_state_dict


class _H:
    def __init__(self, score, yseq):
        self.score, self.yseq = score, yseq


def _pred_out(w, yseq, cache):
    """prediction-network output after consuming yseq (leading blank included), from the zero state"""
    key = tuple(yseq)
    if key not in cache:
        L, H = len(w["layers"]), w["layers"][0][1].shape[1]
        st = (np.zeros((L, 1, H)), np.zeros((L, 1, H)))
        for t in yseq:
            st = pred_step64(w, np.array([t]), st, np.ones(1, bool))
        cache[key] = st[0][-1][0]
    return cache[key]


def reference_alsd(w, h, beam_size, u_max_arg, score_norm=True, act="tanh"):
    """align_length_sync_decoding, line by line, on one utterance's encoder states h [T, D_enc]; k = min(beam, V - 1) extensions as
    the package's per-utterance search takes them"""
    V = w["lin_out_w"].shape[0]
    beam = min(beam_size, V)
    k = min(beam, V - 1)
    h_length = h.shape[0]
    u_max = min(u_max_arg, h_length - 1)
    enc = np.asarray(h, np.float64) @ w["lin_enc_w"].T + w["lin_enc_b"]
    B = [_H(0.0, [0])]
    final = []
    cache = {}
    for i in range(h_length + u_max):
        A = []
        B_ = []
        h_states = []
        for hyp in B:
            u = len(hyp.yseq) - 1
            t = i - u + 1
            if t > (h_length - 1):
                continue
            B_.append(hyp)
            h_states.append((t, enc[t]))
        if B_:
            beam_y = np.stack([_pred_out(w, hyp.yseq, cache) for hyp in B_])
            h_enc = np.stack([x[1] for x in h_states])
            logits = act64(h_enc + beam_y @ w["lin_dec_w"].T, act) @ w["lin_out_w"].T + w["lin_out_b"]
            mx = logits.max(1, keepdims=True)
            beam_logp = logits - mx - np.log(np.exp(logits - mx).sum(1, keepdims=True))
            order = np.argsort(-beam_logp[:, 1:], axis=1, kind="stable")[:, :k]
            for j, hyp in enumerate(B_):
                new_hyp = _H(hyp.score + float(beam_logp[j, 0]), hyp.yseq[:])
                A.append(new_hyp)
                if h_states[j][0] == (h_length - 1):
                    final.append(new_hyp)
                for kk in order[j] + 1:
                    A.append(_H(hyp.score + float(beam_logp[j, kk]), hyp.yseq[:] + [int(kk)]))
            B = sorted(A, key=lambda x: x.score, reverse=True)[:beam]
            rec = []                                     # recombine_hyps: returns hyps
            for hyp in B:
                seq_final = [f.yseq for f in rec if f.yseq]
                if hyp.yseq in seq_final:
                    seq_pos = seq_final.index(hyp.yseq)
                    rec[seq_pos].score = np.logaddexp(rec[seq_pos].score, hyp.score)
                else:
                    rec.append(hyp)
    if final:
        if score_norm:
            final = sorted(final, key=lambda x: x.score / len(x.yseq), reverse=True)
        else:
            final = sorted(final, key=lambda x: x.score, reverse=True)
        return [(float(x.score), x.yseq) for x in final]
    return [(float(x.score), x.yseq) for x in B]


def _case(seed, dtype, L, H, J, V, n, T):
    sd = seeded_weights(seed, dtype, L, H, 6, J, V, 8, {2: 0.0, 6: 2.0}.get(V, 4.0))
    r = np.random.default_rng(seed + 1)
    hs = r.standard_normal((n, T, 8)).astype(np.float32)
    hlens = r.integers(3, T + 1, n)
    hlens[0], hlens[-1] = T, 1
    if n > 2:
        hlens[1] = 2
    return weights_from_state_dict(sd), hs, hlens


@pytest.mark.parametrize("dtype,L,H,J,V", [("lstm", 1, 12, 7, 6), ("gru", 2, 12, 7, 6), ("lstm", 2, 16, 20, 40), ("gru", 1, 12, 7, 2)])
@pytest.mark.parametrize("beam,u_max,score_norm", [(2, 4, False), (3, 20, True), (8, 5, True)])
def test_batched_restatement_equals_the_reference_loop(dtype, L, H, J, V, beam, u_max, score_norm):
    """alsd_batch64 (n * W rows in lock-step, arrays, alsd_step64) against the reference's loop on every utterance alone"""
    w, hs, hlens = _case(3 + beam, dtype, L, H, J, V, 5, 9)
    got = alsd_batch64(w, hs, hlens, beam, u_max, score_norm)
    for b in range(len(hlens)):
        want = reference_alsd(w, hs[b, :hlens[b]], beam, u_max, score_norm)
        assert [y for _s, y in got["nbest"][b]] == [y for _s, y in want], (b, got["nbest"][b], want)
        for (s, _y), (s_ref, _y2) in zip(got["nbest"][b], want):
            assert abs(s - s_ref) <= 1e-10 * max(1.0, abs(s_ref)), (b, s, s_ref)
    assert got["no_final"] >= 1                       # the utterance of one frame: B is returned as it is
    assert got["finals"] > 0 and got["min_gap"] > 0


def test_one_step_restatement_on_a_hand_made_step():
    """two slots reach [0, 3] - one by its blank continuation, one by emitting 3 - while a third sits past the last frame:
    the duplicate stays, the first occurrence grows, the inactive slot vanishes, the final carries the grown score"""
    n, W, V, T, u_max, i = 1, 3, 6, 4, 3, 3
    k = 3
    st, fin = new_state(n, W, T, u_max), new_finals(n, W, u_max)
    st["nhyp"][0] = 3
    st["ulen"][0] = [1, 0, 3]                          # t = 3, 4 (past T - 1 = 3), 1
    st["yseq"][0, 0, :2] = [0, 3]
    st["yseq"][0, 2, :4] = [0, 1, 2, 3]
    st["score"][0] = [-1.0, -0.5, -2.0]
    rec = np.full((3, 1 + 2 * k), -9.0, np.float32)
    rec[:, k + 1:] = [1, 2, 4]
    rec[0, 0] = -0.25                                  # [0, 3] by blank: -1.25, final (t == T - 1)
    rec[2, :] = [-0.125, -7, -8, -9, 4, 1, 2]          # [0, 1, 2, 3] by blank: -2.125
    out, fo, par, tok, live, frame, active = alsd_step64(rec, None, st, fin, V, T, u_max, i)
    assert active.tolist() == [[True, False, True]]
    assert out["nhyp"][0] == 3 and out["ulen"][0].tolist() == [1, 3, 4]
    assert out["score"][0].tolist() == [-1.25, -2.125, -9.0]
    assert par.tolist() == [0, 2, 2] and tok.tolist() == [0, 0, 4] and live.tolist() == [0, 0, 1]
    assert frame.tolist() == [3, 2, 1]
    assert fo["nfin"][0] == 1 and fo["score"][0, 0] == -1.25 and fo["yseq"][0, 0, :2].tolist() == [0, 3]
    # now slot 1 emits 3 onto [0] ... with a step in which [0] + 3 and [0, 3] + blank meet
    st2 = new_state(n, W, T, u_max)
    st2["nhyp"][0] = 2
    st2["ulen"][0] = [1, 0, 0]
    st2["yseq"][0, 0, :2] = [0, 3]
    st2["score"][0] = [-1.0, -1.5, 0.0]
    rec2 = np.full((3, 1 + 2 * k), -9.0, np.float32)
    rec2[:, k + 1:] = [3, 2, 4]
    rec2[0, 0] = -0.25                                 # [0, 3]: -1.25, on frame i - 1 + 1 = 1
    rec2[1, 1] = -0.5                                  # [0] + 3: -2.0
    out, fo, par, tok, live, frame, _ = alsd_step64(rec2, None, st2, fin, V, T, u_max, 1)
    grown = float(np.logaddexp(-1.25, -2.0))
    assert out["score"][0].tolist() == [grown, -2.0, -10.0] and out["ulen"][0].tolist() == [1, 1, 2]
    assert par.tolist() == [0, 1, 0] and live.tolist() == [0, 1, 1] and tok.tolist() == [0, 3, 3]
    assert fo["nfin"][0] == 0


def test_every_gpu_search_case_finds_a_seed():
    """the deterministic seed search of tests/test_gpu_rnnt_alsd.py, run with the restatement alone"""
    import test_gpu_rnnt_alsd as g
    for col, vals in enumerate([("lstm", "gru"), (1, 2), (12, 64), (7, 52), (6, 257), (3, 20), (4, 20), (2, 3, 8)]):
        assert {c[col] for c in g.SEARCH_CASES} == set(vals), col
    tot = dict(merges=0, dropped=0, no_final=0)
    for case in g.SEARCH_CASES:
        seed = g.search_seed(*case)
        ref = g.search_reference(*case, seed)
        assert ref["min_gap"] >= g.GAP
        for key in tot:
            tot[key] += ref[key]
    assert all(v > 0 for v in tot.values()), tot
