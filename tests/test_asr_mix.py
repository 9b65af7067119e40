"""Multi-speaker Transformer ASR, CPU side: a numpy restatement of permutation-invariant training (the reference's depth-first
permutation order, score arithmetic and tie rule) against the reference's recorded pair losses and choices
(tests/golden/asr_mix.npz, tools/gen_golden_asr_mix.py), the model's options, and the reference's state_dict layout.
No GPU is used here; tests/test_gpu_asr_mix.py runs eamd_ctc_pit_loss against this restatement."""
import argparse

import numpy as np
import pytest

from conftest import load_golden

SPKRS = (2, 3)
ALPHAS = (0.2, 1.0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("asr_mix.npz")


def dfs_perms(S):
    """PIT.permutationDFS (e2e_asr_mix.py:110-128)"""
    out = []

    def go(src, k):
        if k == len(src) - 1:
            out.append(list(src))
        for i in range(k, len(src)):
            src[k], src[i] = src[i], src[k]
            go(src, k + 1)
            src[k], src[i] = src[i], src[k]
    go(list(range(S)), 0)
    return out


def pit_ref(pair):
    """pair (B, S^2) float32 losses nll[i, j] / B in hypothesis-major order -> (perm (B, S), pit (B,)) in float32: each
    permutation's score is (sum over i in order of pair[i S + p[i]]) / S, the first minimum wins (torch.min)"""
    pair = np.asarray(pair, np.float32)
    B, S2 = pair.shape
    S = int(round(S2 ** 0.5))
    perms = dfs_perms(S)
    perm, pit = np.zeros((B, S), np.int64), np.zeros(B, np.float32)
    for b in range(B):
        scores = []
        for p in perms:
            sc = np.float32(0.0)
            for i in range(S):
                sc = np.float32(sc + pair[b, i * S + p[i]])
            scores.append(np.float32(sc / np.float32(S)))
        k = int(np.argmin(np.asarray(scores, np.float32)))      # first minimum
        perm[b], pit[b] = perms[k], scores[k]
    return perm, pit


def test_dfs_order_is_the_references():
    assert dfs_perms(2) == [[0, 1], [1, 0]]
    assert dfs_perms(3) == [[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 1, 0], [2, 0, 1]]
    from espnet_amd.nets.e2e_asr_mix_transformer import pit_permutations
    assert pit_permutations(2) == dfs_perms(2) and pit_permutations(3) == dfs_perms(3)


def test_tie_rule_is_first_minimum():
    pair = np.array([[1.0, 1.0, 2.0, 2.0]], np.float32)         # [0,1]: 1 + 2, [1,0]: 1 + 2
    perm, pit = pit_ref(pair)
    assert perm.tolist() == [[0, 1]] and pit[0] == np.float32(1.5)
    pair = np.array([[3.0, 1.0, 1.0, 3.0]], np.float32)
    assert pit_ref(pair)[0].tolist() == [[1, 0]]


@pytest.mark.parametrize("S", SPKRS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_pit_restatement_reproduces_reference(golden, S, alpha):
    tag = "tr_s%d_a%g" % (S, alpha)
    perm, pit = pit_ref(golden[tag + "_pair"])
    assert perm.tolist() == golden[tag + "_perm"].tolist()
    loss_ctc = float(np.float32(pit.sum(dtype=np.float32) / np.float32(len(pit))))
    assert abs(loss_ctc - float(golden[tag + "_loss_ctc"])) <= 1e-6 * abs(float(golden[tag + "_loss_ctc"]))


def test_fixture_covers_the_edge_cases(golden):
    ys = golden["tr_s2_ys"]
    assert (ys[1, 1] == -1).all()                                 # an empty transcript
    assert (ys[2, 0] == ys[2, 1]).all()                           # identical transcripts: an exact tie ...
    pair = golden["tr_s2_a0.2_pair"]
    assert pair[2, 0] == pair[2, 1] and pair[2, 2] == pair[2, 3]
    assert golden["tr_s2_a0.2_perm"][2].tolist() == [0, 1]        # ... which the first permutation wins
    assert len(set(golden["tr_s2_ilens"].tolist())) == 3          # unequal lengths


def test_options_match_reference_parser():
    """E2E.add_arguments: the Transformer E2E's options and --elayers-sd (e2e_asr_mix.py:149-166; --spa belongs to the RNN model)"""
    from espnet_amd.nets.e2e_asr_mix_transformer import E2E
    p = E2E.add_arguments(argparse.ArgumentParser())
    d = vars(p.parse_args([]))
    expect = dict(elayers_sd=4, transformer_init="pytorch", transformer_input_layer="conv2d", transformer_attn_dropout_rate=None,
                  dropout_rate=0.0, elayers=4, eunits=300, adim=320, aheads=4, dlayers=1, dunits=320,
                  transformer_length_normalized_loss=True)
    for k, v in expect.items():
        assert d[k] == v, k
    assert vars(p.parse_args(["--elayers-sd", "2"]))["elayers_sd"] == 2


@pytest.mark.parametrize("S", SPKRS)
def test_model_has_reference_state_dict_layout(golden, S):
    from espnet_amd.nets.e2e_asr_mix_transformer import E2E
    from tools.gen_golden_asr_mix import TRAIN_IDIM, TRAIN_ODIM, train_ns
    m = E2E(TRAIN_IDIM, TRAIN_ODIM, argparse.Namespace(**train_ns(S, 0.2)))
    sd = m.state_dict()
    keys = golden["keys_s%d" % S].tolist()
    assert list(sd.keys()) == keys
    for k, shp in zip(keys, golden["shapes_s%d" % S].tolist()):
        assert list(sd[k].shape) == [int(v) for v in shp if v], k
    assert m.num_spkrs == S and len(m.encoder.encoders_sd) == S and m.ctc.reduce is False


def test_num_spkrs_defaults_to_two():
    from espnet_amd.nets.e2e_asr_mix_transformer import E2E
    ns = argparse.Namespace(adim=64, aheads=4, elayers=1, elayers_sd=1, eunits=64, dlayers=1, dunits=64, mtlalpha=0.3)
    assert E2E(20, 12, ns).num_spkrs == 2


def test_ctc_reduce_false_constructs():
    from espnet_amd.nets.modules import CTC
    c = CTC(12, 16, 0.0, reduce=False)
    assert c.reduce is False
