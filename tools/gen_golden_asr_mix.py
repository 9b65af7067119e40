#!/usr/bin/env python3
"""tests/golden/asr_mix.npz by RUNNING THE REFERENCE's multi-speaker Transformer (e2e_asr_mix_transformer.py, transformer/encoder_mix.py,
e2e_asr_mix.py PIT; PyTorch CPU).

Training (small widths, dropout 0, name-keyed weights from oracle/seeded_weights.py), S in {2, 3}, mtlalpha in {0.2, 1.0}:
  tr_s{S}_{xs,ilens,ys}                         the batch: unequal lengths, an empty transcript, two speakers with identical
                                                transcripts in the last utterance (an exact permutation tie)
  tr_s{S}_a{A}_{loss,loss_ctc,loss_att,acc}     the reference's losses and accuracy of one training forward (loss_att / acc: -1
                                                when mtlalpha = 1)
  tr_s{S}_a{A}_pair, _perm                      the (B, S^2) pair losses PIT.pit_process received (nll / B) and its min_perm
  tr_s{S}_a{A}/grad..., gprobe_...              gradients (seeded_weights.grad_record; probes above 512 elements)
  keys_s{S}, shapes_s{S}                        the reference's state_dict names and shapes (zero-padded to 4 dims), mtlalpha 0.2
Decoding (a DECODE_R4-like Transformer: adim 256, eunits = dunits = 2048, odim 5000, output layers sharpened and <eos> / blank
biased; S = 2; beam 10; three seeded utterances):
  dec_u{u}_seed                                 the features are decode_inputs(seed)[u]
  dec_c{c}_u{u}_s{s}_ids, _scores, _len         each speaker's n-best (NBEST) yseq (padded with -1) and scores, ctc_weight CTCW[c]
An utterance whose smallest relative gap between recorded n-best scores is below MIN_MARGIN is redrawn from the next seed.
Usage: python tools/gen_golden_asr_mix.py [--ref /root/reference] [--out tests/golden]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
from gen_golden import install_stubs, save  # noqa: E402
import seeded_weights as SW  # noqa: E402
from tools.gen_golden_maskctc import MIN_MARGIN, grad_rec  # noqa: E402

TRAIN_SALT = 71
DEC_SALT = 72
ALPHAS = (0.2, 1.0)
SPKRS = (2, 3)
CTCW = (0.3, 0.0)
NBEST = 3
TRAIN_NS = dict(adim=64, aheads=4, elayers=2, elayers_sd=1, eunits=128, dlayers=2, dunits=128, lsm_weight=0.1,
                dropout_rate=0.0, transformer_attn_dropout_rate=0.0, transformer_length_normalized_loss=False,
                transformer_init="pytorch", transformer_input_layer="conv2d", ctc_type="builtin", report_cer=False,
                report_wer=False, char_list=None, sym_space="<space>", sym_blank="<blank>",
                transformer_encoder_selfattn_layer_type="selfattn", transformer_decoder_selfattn_layer_type="selfattn")
TRAIN_IDIM, TRAIN_ODIM = 20, 12
DECODE = dict(idim=80, odim=5000, lens=(400, 300, 200), beam=10, out_scale=4.0, eos_bias=7.0, blank_bias=12.0, salt=DEC_SALT,
              ns=dict(TRAIN_NS, adim=256, aheads=4, elayers=2, elayers_sd=1, eunits=2048, dlayers=2, dunits=2048, mtlalpha=0.3,
                      num_spkrs=2))


def train_ns(S, alpha):
    return dict(TRAIN_NS, mtlalpha=alpha, num_spkrs=S)


def train_batch(S):
    """(xs, ilens, ys (B, S, L)): utterance 1's last speaker has an empty transcript, utterance 2's first two speakers say the
    same thing"""
    g = torch.Generator().manual_seed(11 + S)
    xs = torch.randn(3, 100, TRAIN_IDIM, generator=g)
    ilens = torch.tensor([100, 77, 60])
    ys = torch.randint(1, TRAIN_ODIM - 1, (3, S, 9), generator=g)
    ys[0, 1, 7:] = -1
    ys[1, 0, 5:] = -1
    ys[1, S - 1, :] = -1
    ys[2, 0, 4:] = -1
    ys[2, 1] = ys[2, 0]
    if S == 3:
        ys[2, 2, 6:] = -1
    return xs, ilens, ys


def decode_inputs(seed, spec=DECODE):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(T, spec["idim"], generator=g) for T in spec["lens"]]


def recog_args(ctc_weight):
    return argparse.Namespace(beam_size=DECODE["beam"], penalty=0.0, maxlenratio=0.0, minlenratio=0.0, ctc_weight=ctc_weight,
                              lm_weight=0.0, nbest=NBEST)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    install_stubs()
    sys.path.insert(0, a.ref)
    torch.set_num_threads(8)
    from espnet.nets.pytorch_backend.e2e_asr_mix_transformer import E2E

    rec = {}
    # ---- training ----------------------------------------------------------------------------------------------------
    for S in SPKRS:
        xs, ilens, ys = train_batch(S)
        rec.update({"tr_s%d_xs" % S: xs.numpy(), "tr_s%d_ilens" % S: ilens.numpy(), "tr_s%d_ys" % S: ys.numpy()})
        for alpha in ALPHAS:
            model = SW.fill_parameters(E2E(TRAIN_IDIM, TRAIN_ODIM, argparse.Namespace(**train_ns(S, alpha))), salt=TRAIN_SALT)
            model.train()
            if alpha < 1.0:         # the layout with a decoder
                rec["keys_s%d" % S] = np.asarray(list(model.state_dict().keys()))
                rec["shapes_s%d" % S] = np.asarray([list(v.shape) + [0] * (4 - v.dim()) for v in model.state_dict().values()], np.int64)
            cap = {}
            pit_process = model.pit.pit_process

            def wrapped(losses, _f=pit_process):
                loss, perm = _f(losses)
                cap.update(pair=losses.detach().clone().numpy(), perm=perm.clone().numpy(), loss_ctc=float(loss))
                return loss, perm
            model.pit.pit_process = wrapped
            # the reporter's arguments are the reference's float(loss_ctc), float(loss_att), acc (e2e_asr_mix_transformer.py:188-210)
            model.reporter = types.SimpleNamespace(report=lambda *r: cap.update(report=r))
            loss = model(xs, ilens, ys.clone())       # (the reference permutes the labels of its argument in place)
            loss.backward()
            tag = "tr_s%d_a%g" % (S, alpha)
            _, la, acc = cap["report"][:3]
            rec.update({tag + "_loss": np.float64(float(loss)), tag + "_loss_ctc": np.float64(cap["loss_ctc"]),
                        tag + "_loss_att": np.float64(-1.0 if la is None else la),
                        tag + "_acc": np.float64(-1.0 if acc is None else float(acc)),
                        tag + "_pair": cap["pair"], tag + "_perm": cap["perm"]})
            for name, p in model.named_parameters():
                if p.grad is not None:
                    rec.update({tag + "/" + k: v for k, v in grad_rec(name, p.grad).items()})
            print(tag, "loss %.6f ctc %.6f att %.6f acc %.4f perm %s" % (float(loss), cap["loss_ctc"], rec[tag + "_loss_att"],
                                                                         rec[tag + "_acc"], cap["perm"].tolist()), flush=True)

    # ---- decoding ----------------------------------------------------------------------------------------------------
    model = SW.decode_r4_model(E2E, DECODE)
    seed = 50
    for u in range(3):
        while True:
            x = decode_inputs(seed)[u]
            res, worst = {}, np.inf
            for c, w in enumerate(CTCW):
                with torch.no_grad():
                    nb = model.recognize(x.numpy(), recog_args(w), char_list=None)
                for s, hyps in enumerate(nb):
                    sc = [float(h["score"]) for h in hyps]
                    for k in range(len(sc) - 1):
                        worst = min(worst, (sc[k] - sc[k + 1]) / max(1.0, abs(sc[k])))
                    res[(c, s)] = hyps
            if worst >= MIN_MARGIN and all(len(h) == NBEST for h in res.values()):
                break
            print("dec u%d seed %d: margin %.2e, redrawn" % (u, seed, worst), flush=True)
            seed += 1
        rec["dec_u%d_seed" % u] = np.int64(seed)
        for (c, s), hyps in res.items():
            tag = "dec_c%d_u%d_s%d" % (c, u, s)
            Lm = max(len(h["yseq"]) for h in hyps)
            ids = np.full((len(hyps), Lm), -1, np.int32)
            for k, h in enumerate(hyps):
                ids[k, :len(h["yseq"])] = [int(t) for t in h["yseq"]]
            rec[tag + "_ids"] = ids
            rec[tag + "_scores"] = np.asarray([float(h["score"]) for h in hyps], np.float64)
            rec[tag + "_len"] = np.asarray([len(h["yseq"]) for h in hyps], np.int32)
            print(tag, "seed %d lens %s scores %s" % (seed, rec[tag + "_len"].tolist(), np.round(rec[tag + "_scores"], 3).tolist()),
                  flush=True)
        seed += 1
    save(os.path.join(a.out, "asr_mix.npz"), **rec)



if __name__ == "__main__":
    main()
