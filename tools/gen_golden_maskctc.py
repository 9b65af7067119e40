#!/usr/bin/env python3
"""tests/golden/maskctc.npz by RUNNING THE REFERENCE's Mask-CTC model (e2e_asr_maskctc.py, maskctc/*.py; PyTorch CPU + numpy).

Training (small Transformer and Conformer encoders, name-keyed weights from oracle/seeded_weights.py, numpy seeds 0 and 1):
  tr_{enc}_s{seed}_{loss,loss_ctc,loss_att,acc}   the reference's losses and accuracy of one training forward
  tr_{enc}_s{seed}_{ys_in,ys_out}                 the decoder input / target the reference's mask_uniform drew
  tr_{enc}_s{seed}/grad... , gprobe_...           gradients (seeded_weights.grad_record; probes above 512 elements)
  tr_xs, tr_ilens, tr_ys                          the batch (same for every case)
  keys_{enc}, shapes_{enc}                        the reference's state_dict names and shapes (zero-padded to 4 dims)
Decoding (a DECODE_R4-like model - BASELINE config 2's width, odim 5000, CTC output sharpened and blank-biased - with both
encoders, on three seeded utterances; thresholds at the quantiles of the recorded token probabilities that mask some, most, none
and all tokens; K in {0, 1, 3, 10}):
  dec_{enc}_u{u}_seed                             the features are decode_inputs(seed)[u]
  dec_{enc}_u{u}_fid, _fp                         the reference's per-frame CTC argmax and its probability
  dec_{enc}_u{u}_thr                              the four thresholds
  dec_{enc}_u{u}_t{i}_k{K}_seeded                 the seeded y_in (after the threshold)
  dec_{enc}_u{u}_t{i}_k{K}_passes                 y_in given to the decoder in each pass [npass, L]
  dec_{enc}_u{u}_t{i}_k{K}_score, _arg            max / argmax of the decoder logits at the masked positions in each pass
  dec_{enc}_u{u}_t{i}_k{K}_yseq                   the final hypothesis
  dec_{enc}_u{u}_t{i}_k{K}_margins                [token prob - thr, CTC argmax gap, top-k boundary gap, final argmax gap], relative
An utterance whose smallest margin is below MIN_MARGIN (2e-5; fp32 on the GPU moves these quantities by about 1e-6) is redrawn from the next seed.  Weights are not stored.
Usage: python tools/gen_golden_maskctc.py [--ref /root/reference] [--out tests/golden]
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

MIN_MARGIN = 2e-5
KS = (0, 1, 3, 10)
TRAIN_SALT = {"transformer": 61, "conformer": 62}
DEC_SALT = {"transformer": 63, "conformer": 4}

TRAIN_NS = dict(adim=64, aheads=4, elayers=2, eunits=128, dlayers=2, dunits=128, mtlalpha=0.3, lsm_weight=0.1,
                dropout_rate=0.0, transformer_attn_dropout_rate=0.0, transformer_length_normalized_loss=False,
                transformer_init="pytorch", transformer_input_layer="conv2d", ctc_type="builtin", report_cer=False,
                report_wer=False, char_list=None, sym_space="<space>", sym_blank="<blank>")
CONFORMER_NS = dict(maskctc_use_conformer_encoder=True, transformer_encoder_pos_enc_layer_type="rel_pos",
                    transformer_encoder_selfattn_layer_type="rel_selfattn", transformer_encoder_activation_type="swish",
                    macaron_style=True, use_cnn_module=True, cnn_module_kernel=15)
TRANSFORMER_NS = dict(maskctc_use_conformer_encoder=False, transformer_encoder_selfattn_layer_type="selfattn",
                      transformer_encoder_pos_enc_layer_type="abs_pos", macaron_style=False, use_cnn_module=False)
TRAIN_IDIM, TRAIN_ODIM = 20, 12


def grad_rec(name, grad):
    """seeded_weights.grad_record with the probe form above 512 elements (keeps the file small)"""
    if grad.numel() <= 512:
        return SW.grad_record(name, grad)
    l, r = SW.probe_vectors(name, grad.shape)
    G = grad.detach().cpu().double().reshape(grad.shape[0], -1)
    return {"gprobe_r/" + name: (G @ r).numpy(), "gprobe_l/" + name: (l @ G).numpy(), "gnorm/" + name: np.asarray(float(G.norm()))}


def train_ns(enc):
    return dict(TRAIN_NS, **(CONFORMER_NS if enc == "conformer" else TRANSFORMER_NS))


def train_batch():
    g = torch.Generator().manual_seed(7)
    xs = torch.randn(3, 100, TRAIN_IDIM, generator=g)
    ilens = torch.tensor([100, 77, 60])
    ys = torch.randint(1, TRAIN_ODIM - 1, (3, 9), generator=g)
    ys[1, 6:] = -1
    ys[2, 4:] = -1
    return xs, ilens, ys


def decode_ns(enc):
    ns = dict(SW.DECODE_R4["ns"])
    if enc == "transformer":
        ns.update(TRANSFORMER_NS, cnn_module_kernel=31)
    else:
        ns.update(maskctc_use_conformer_encoder=True)
    return ns


def decode_spec(enc):
    return dict(SW.DECODE_R4, ns=decode_ns(enc), salt=DEC_SALT[enc])


def decode_inputs(seed, spec=SW.DECODE_R4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(T, spec["idim"], generator=g) for T in spec["lens"]]


def token_probs(fid, fp, blank=0):
    """the reference's groupby + run max: (ids, probs) of the non-blank runs"""
    ids, probs = [], []
    prev = None
    for v, p in zip(fid.tolist(), fp.tolist()):
        if v != prev:
            ids.append(v)
            probs.append(p)
            prev = v
        else:
            probs[-1] = max(probs[-1], p)
    keep = [i for i, v in enumerate(ids) if v != blank]
    return np.asarray([ids[i] for i in keep], np.int64), np.asarray([probs[i] for i in keep], np.float64)


def thresholds(probs):
    """some / most / none / all masked: the midpoint of the widest (relative) gap between sorted token probabilities in the
    lower and in the upper part of the quantile range; 0; 2"""
    s = np.unique(probs)

    def widest(lo, hi):
        i0 = int(lo * (len(s) - 1))
        i1 = max(i0 + 1, int(hi * (len(s) - 1)))
        i = max(range(i0, min(i1, len(s) - 1)), key=lambda j: (s[j + 1] - s[j]) / s[j + 1])
        return float(0.5 * (s[i] + s[i + 1]))
    if len(s) < 2:
        return np.asarray([0.5 * s[0], 0.5 * s[0], 0.0, 2.0])
    return np.asarray([widest(0.1, 0.4), widest(0.5, 0.9), 0.0, 2.0])


def run_decode(model, x, thr, K):
    """the reference's recognize with its decoder wrapped: (yseq, passes, score, arg, margins)"""
    passes, scores, args, topk_gaps, arg_gaps = [], [], [], [], []
    fwd = model.decoder.forward

    def wrapped(tgt, tgt_mask, memory, memory_mask):
        out = fwd(tgt, tgt_mask, memory, memory_mask)
        logits = out[0][0].detach()
        passes.append(tgt[0].clone().numpy())
        sc, ar = logits.max(-1)
        scores.append(sc.numpy().copy())
        args.append(ar.numpy().astype(np.int32))
        top2 = logits.topk(2, -1)[0]
        masked = (tgt[0] == model.mask_token).numpy()
        gap = ((top2[:, 0] - top2[:, 1]) / top2[:, 0].abs().clamp_min(1.0)).numpy()
        arg_gaps.append(float(gap[masked].min()) if masked.any() else np.inf)
        return out
    model.decoder.forward = wrapped
    try:
        ra = argparse.Namespace(maskctc_probability_threshold=float(thr), maskctc_n_iterations=K)
        hyp = model.recognize(x.numpy(), ra, char_list=[str(i) for i in range(model.odim)])[0]
    finally:
        model.decoder.forward = fwd
    # top-k boundary gaps of the passes that select (all but the last)
    seed_y = passes[0] if passes else None
    if passes:
        M = int((seed_y == model.mask_token).sum())
        n_it = K if (M >= K and K > 0) else M
        kper = M // n_it
        for p in range(len(passes) - 1):
            m = passes[p] == model.mask_token
            s = np.sort(scores[p][m])[::-1]
            if len(s) > kper:
                topk_gaps.append(float((s[kper - 1] - s[kper]) / max(1.0, abs(float(s[kper - 1])))))
    return hyp["yseq"], passes, scores, args, (min(topk_gaps) if topk_gaps else np.inf), (min(arg_gaps) if arg_gaps else np.inf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    install_stubs()
    sys.path.insert(0, a.ref)
    torch.set_num_threads(8)
    from espnet.nets.pytorch_backend.e2e_asr_maskctc import E2E

    rec = {}
    # ---- training ----------------------------------------------------------------------------------------------------
    xs, ilens, ys = train_batch()
    rec.update(tr_xs=xs.numpy(), tr_ilens=ilens.numpy(), tr_ys=ys.numpy())
    for enc in ("transformer", "conformer"):
        for seed in (0, 1):
            model = SW.fill_parameters(E2E(TRAIN_IDIM, TRAIN_ODIM, argparse.Namespace(**train_ns(enc))), salt=TRAIN_SALT[enc])
            model.train()
            rec["keys_" + enc] = np.asarray(list(model.state_dict().keys()))
            rec["shapes_" + enc] = np.asarray([list(v.shape) + [0] * (4 - v.dim()) for v in model.state_dict().values()], np.int64)
            cap = {}
            dec_fwd = model.decoder.forward

            def dec_wrapped(tgt, tgt_mask, memory, memory_mask, _f=dec_fwd):
                cap["ys_in"] = tgt.clone()
                return _f(tgt, tgt_mask, memory, memory_mask)
            model.decoder.forward = dec_wrapped
            h = model.criterion.register_forward_hook(lambda m, i, o: cap.update(ys_out=i[1].clone(), loss_att=float(o.detach())))
            np.random.seed(seed)
            loss = model(xs, ilens, ys)
            loss.backward()
            h.remove()
            tag = "tr_%s_s%d" % (enc, seed)
            rec.update({tag + "_loss": np.float64(float(loss)), tag + "_loss_ctc": np.float64(float(model.ctc.loss)),
                        tag + "_loss_att": np.float64(cap["loss_att"]), tag + "_acc": np.float64(model.acc),
                        tag + "_ys_in": cap["ys_in"].numpy(), tag + "_ys_out": cap["ys_out"].numpy()})
            for name, p in model.named_parameters():
                if p.grad is not None:
                    rec.update({tag + "/" + k: v for k, v in grad_rec(name, p.grad).items()})
            print(tag, "loss %.6f ctc %.6f att %.6f acc %.4f" % (float(loss), float(model.ctc.loss), cap["loss_att"], model.acc),
                  flush=True)

    # ---- decoding ----------------------------------------------------------------------------------------------------
    for enc in ("transformer", "conformer"):
        spec = decode_spec(enc)
        model = SW.decode_r4_model(E2E, spec)
        assert model.mask_token == spec["odim"] and model.eos == spec["odim"] - 1
        seed = 40
        for u in range(3):
            while True:
                x = decode_inputs(seed)[u]
                with torch.no_grad():
                    h = model.encode(x.numpy()).unsqueeze(0)
                    fp, fid = torch.exp(model.ctc.log_softmax(h)).max(-1)
                    top2 = torch.exp(model.ctc.log_softmax(h)).topk(2, -1)[0][0]
                fid, fp = fid[0].numpy(), fp[0].numpy()
                ctc_gap = float(((top2[:, 0] - top2[:, 1]) / top2[:, 0]).min())
                ids, probs = token_probs(fid, fp)
                thr = thresholds(probs)
                cases, worst = {}, ctc_gap
                for ti, t in enumerate(thr):
                    pgap = float(np.min(np.abs(probs - t)) / max(t, 1e-30)) if len(probs) and 0.0 < t < 1.5 else np.inf
                    for K in KS:
                        yseq, passes, scores, args, tk, ag = run_decode(model, x, t, K)
                        cases[(ti, K)] = (yseq, passes, scores, args, [pgap, ctc_gap, tk, ag])
                        worst = min(worst, pgap, tk, ag)
                if worst >= MIN_MARGIN and len(probs) > 3:
                    break
                print("dec %s u%d seed %d: margin %.2e (ctc %.2e; cases %s), redrawn" % (
                    enc, u, seed, worst, ctc_gap, ["%.1e" % min(c[4]) for c in cases.values()]), flush=True)
                seed += 1
            tag = "dec_%s_u%d" % (enc, u)
            rec.update({tag + "_fid": fid.astype(np.int16), tag + "_fp": fp.astype(np.float32),
                        tag + "_thr": thr, tag + "_seed": np.int64(seed)})
            for (ti, K), (yseq, passes, scores, args, margins) in cases.items():
                ct = "%s_t%d_k%d" % (tag, ti, K)
                L = len(yseq) - 2
                mask_seed = np.asarray(passes[0] if passes else yseq[1:-1], np.int32)
                rec[ct + "_yseq"] = np.asarray(yseq, np.int32)
                P = np.asarray(passes, np.int16).reshape(len(passes), L)
                rec[ct + "_passes"] = P
                # scores only where they are read (masked positions): the rest is zero, which compresses
                rec[ct + "_score"] = np.where(P == model.mask_token, np.asarray(scores, np.float32).reshape(len(passes), L), 0)
                rec[ct + "_arg"] = np.where(P == model.mask_token, np.asarray(args, np.int16).reshape(len(passes), L), 0)
                rec[ct + "_margins"] = np.asarray(margins, np.float64)
                rec[ct + "_seeded"] = mask_seed
            nm = [int((cases[(ti, 10)][1][0] == model.mask_token).sum()) if cases[(ti, 10)][1] else 0 for ti in range(4)]
            print(tag, "seed %d T'=%d tokens %d masked per threshold %s margin %.2e" % (seed, len(fid), len(probs), nm, worst),
                  flush=True)
            seed += 1
    save(os.path.join(a.out, "maskctc.npz"), **rec)


if __name__ == "__main__":
    main()
