"""Two-pass decoding (nets.nbest_rescore, csrc/rescore.hip): everything that needs no GPU - the refusals of the public surface fire
before any model or device work, and the entry points refuse their limits before any launch."""
import argparse
import ctypes

import pytest
import torch


def test_speech2text_rescore_checks_its_options_before_any_model_work():
    from espnet_amd.espnet2 import Speech2Text
    with pytest.raises(ValueError, match="ctc_weight"):
        Speech2Text(None, ctc_search="rescore", ctc_weight=0.0)
    with pytest.raises(ValueError, match="ctc_weight"):
        Speech2Text(None, ctc_search="rescore", ctc_weight=1.5)
    with pytest.raises(ValueError, match="nothing to rescore"):
        Speech2Text(None, ctc_search="rescore", ctc_weight=1.0)
    with pytest.raises(ValueError, match="beam_size"):               # the first pass's limits, as ctc_search="time" checks them
        Speech2Text(None, ctc_search="rescore", ctc_weight=0.3, beam_size=33)
    with pytest.raises(ValueError, match="cand_size"):
        Speech2Text(None, ctc_search="rescore", ctc_weight=0.3, beam_size=4, ctc_cand_size=40)
    with pytest.raises(ValueError, match="ctc_search"):
        Speech2Text(None, ctc_search="frames", ctc_weight=1.0)
    # the other branches keep their errors
    with pytest.raises(ValueError, match="ctc_weight"):
        Speech2Text(None, ctc_search="time", ctc_weight=0.5)
    with pytest.raises(ValueError, match="ctc_cand_size"):
        Speech2Text(None, ctc_weight=0.3, ctc_cand_size=8)


def _model(mtlalpha):
    from espnet_amd.nets.e2e_asr_conformer import E2E
    ns = argparse.Namespace(adim=16, aheads=2, elayers=1, eunits=16, dlayers=1, dunits=16, mtlalpha=mtlalpha, dropout_rate=0.0)
    return E2E(8, 6, ns)


def _args(**kw):
    return argparse.Namespace(**dict(dict(ctc_weight=0.3, beam_size=3, nbest=1, penalty=0.0, lm_weight=0.5, ctc_search="rescore"), **kw))


@pytest.mark.parametrize("call", ["recognize", "recognize_batch"])
def test_e2e_rescore_refusals_need_no_gpu(call):
    """each a ValueError with a plain message, raised on a CPU-constructed model before any encoder work"""
    x = torch.zeros(20, 8)

    def run(model, ra, rnnlm=None):
        return model.recognize(x, ra, rnnlm=rnnlm) if call == "recognize" else model.recognize_batch([x], ra, rnnlm=rnnlm)

    with pytest.raises(ValueError, match="no CTC head"):
        run(_model(0.0), _args())
    with pytest.raises(ValueError, match="ctc_weight == 0"):
        run(_model(0.3), _args(ctc_weight=0.0))
    with pytest.raises(ValueError, match="nothing to rescore"):
        run(_model(0.3), _args(ctc_weight=1.0))
    with pytest.raises(ValueError, match="nothing to rescore"):
        run(_model(1.0), _args(ctc_weight=0.3))                       # a CTC-only model decodes with ctc_weight 1.0
    hybrid = _model(0.3)
    hybrid.decoder = None
    with pytest.raises(ValueError, match="decoder"):
        run(hybrid, _args(ctc_weight=0.3))
    with pytest.raises(ValueError, match="beam_size"):
        run(_model(0.3), _args(beam_size=33))
    # without the switch the pure-CTC path still refuses a neural LM
    with pytest.raises(ValueError, match="rnnlm"):
        run(_model(1.0), _args(ctc_search="label", ctc_weight=1.0), rnnlm=torch.nn.Linear(1, 1))


def test_rescorer_refuses_what_it_cannot_score_with():
    from espnet_amd.espnet2 import SequentialRNNLM
    from espnet_amd.nets.nbest_rescore import NBestRescorer
    with pytest.raises(ValueError, match="decoder or a language model"):
        NBestRescorer(sos=5, eos=5)
    with pytest.raises(TypeError, match="TransformerLM"):
        NBestRescorer(lm=torch.nn.Linear(1, 1), sos=5, eos=5)
    with pytest.raises(ValueError, match="ctc_weight"):
        NBestRescorer(decoder=_model(0.3).decoder, ctc_weight=1.0, sos=5, eos=5)
    lm = SequentialRNNLM(6, unit=8, nlayers=2, dropout_rate=0.2).train()
    r = NBestRescorer(lm=lm, lm_weight=0.5, sos=5, eos=5)
    with pytest.raises(ValueError, match="training mode"):
        r.rescore_device(None, [3], torch.zeros(1, 2, 6, dtype=torch.int32))


def test_entry_points_are_declared_and_refuse_their_limits_before_any_launch():
    from espnet_amd import _lib
    for s in ("eamd_nbest_pack", "eamd_nbest_rescore"):
        assert s in _lib.SYMBOLS
    lib = _lib.lib()
    f = ctypes.c_float
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)          # valid-looking (never dereferenced) host addresses
    q = ctypes.cast(ctypes.addressof(buf) + 64, ctypes.c_void_p)

    def pack(nb, B, N, T, U, V, sos, eos, out=p):
        return lib.eamd_nbest_pack(nb, B, N, T, U, V, sos, eos, out, out, out, None)

    assert pack(None, 1, 2, 8, 3, 10, 9, 9) == -1
    assert pack(p, 1, 2, 8, 10, 10, 9, 9) == -1                                   # U > T + 1
    assert pack(p, 1, 2, 8, 3, 10, 10, 9) == -1                                   # sos outside the vocabulary
    assert pack(p, 1, 33, 8, 3, 10, 9, 9) == _lib.EAMD_EUNSUPPORTED               # N > 32
    assert pack(p, 1, 2, 2049, 3, 10, 9, 9) == _lib.EAMD_EUNSUPPORTED             # T > 2048

    def resc(nb, ul, B, N, T, U, S, p1, t1, p2, t2, out=q):
        return lib.eamd_nbest_rescore(nb, ul, B, N, T, U, S, p1, p1, t1, f(0.5), p2, p2, t2, f(0.5), f(0.5), out, out, out, None)

    assert resc(None, p, 1, 2, 8, 3, 1, p, 2, None, 0) == -1
    assert resc(p, p, 1, 2, 8, 3, 1, None, 2, None, 0) == -1
    assert resc(p, p, 1, 2, 8, 3, 2, p, 2, None, 0) == -1                          # two scorers, one given
    assert resc(p, p, 1, 2, 8, 3, 1, p, 0, None, 0) == -1                          # no tiles
    assert resc(p, p, 1, 2, 8, 3, 1, p, 2, None, 0, out=p) == -1                   # in place
    assert resc(p, p, 1, 2, 8, 10, 1, p, 2, None, 0) == -1                         # U > T + 1
    assert resc(p, p, 1, 2, 8, 3, 3, p, 2, p, 2) == _lib.EAMD_EUNSUPPORTED         # S = 3
    assert resc(p, p, 1, 33, 8, 3, 1, p, 2, None, 0) == _lib.EAMD_EUNSUPPORTED     # N > 32
    assert resc(p, p, 1, 2, 2049, 3, 1, p, 2, None, 0) == _lib.EAMD_EUNSUPPORTED   # T > 2048
    odd = ctypes.cast(ctypes.addressof(buf) + 4, ctypes.c_void_p)
    assert resc(p, p, 1, 2, 8, 3, 1, odd, 2, None, 0) == _lib.EAMD_EUNSUPPORTED    # partials not 8-byte aligned
