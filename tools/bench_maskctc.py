#!/usr/bin/env python3
"""Mask-CTC decoding throughput at BASELINE config 2's width: the DECODE_R4 model of oracle/seeded_weights.py (adim 256,
aheads 4, units 2048, CTC output sharpened and blank-biased by 8) grown to a 12-layer Conformer encoder and a 6-layer decoder,
|V| = 5000 (+ <mask>), thr = 0.999, K = 10, utterances of T = 1000 input frames (T' = 249).

  B = 1   recognize() on each of the utterances in turn
  B = 32  recognize_batch() on all of them
and, for B = 32, the split of one maskctc_decode_batch call (device events): encoder, seed (CTC projection + eamd_maskctc_seed +
the first host read), and one mask-predict pass (decoder + eamd_maskctc_update).

Usage: python tools/bench_maskctc.py [--iters 5] [--B 32] [--T 1000]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def split(model, xs_pad, il, thr, K, iters):
    """device time of the stages of maskctc_decode_batch (the same calls, events between them)"""
    from espnet_amd import ops
    from espnet_amd.nets.ctc_align import encode_batch
    from espnet_amd.nets.e2e_asr_maskctc import length_square_mask
    from espnet_amd.nets.modules import make_non_pad_mask
    tot = dict(encoder=0.0, seed=0.0, passes=0.0)
    npass = 0
    for it in range(iters + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        hs, hl = encode_batch(model, xs_pad, il, alone=True)
        ev[1].record()
        with torch.no_grad():
            B, T, _ = hs.shape
            hl_d = ops.h2d_async(torch.tensor(hl, dtype=torch.int32), hs.device)
            seed = ops.maskctc_seed(model.ctc.logits(hs).contiguous(), hl_d, thr, K, model.mask_token, model.eos, 0, Lcap=max(hl))
            info = torch.stack([seed["len"], seed["niter"]]).cpu()
            ev[2].record()
            lens, nit = info[0].tolist(), info[1].tolist()
            Lmax, Nmax = max(lens), max(nit)
            y = seed["y_in"][:, :Lmax].contiguous()
            tgt_mask = ops.h2d_async(length_square_mask(lens, Lmax).to(torch.uint8), hs.device)
            mem_mask = ops.h2d_async(make_non_pad_mask(hl, T).unsqueeze(-2).to(torch.uint8), hs.device)
            sc = ar = None
            for p in range(Nmax):
                pred, _ = model.decoder(y, tgt_mask, hs, mem_mask)
                sc, ar = ops.maskctc_update(p, pred.contiguous(), y, seed["len"], seed["niter"], seed["kper"], model.mask_token,
                                            sc, ar)
            ev[3].record()
        torch.cuda.synchronize()
        if it == 0:
            continue                                   # warm-up
        tot["encoder"] += ev[0].elapsed_time(ev[1])
        tot["seed"] += ev[1].elapsed_time(ev[2])
        tot["passes"] += ev[2].elapsed_time(ev[3])
        npass = Nmax
    out = {k + "_ms": v / iters for k, v in tot.items()}
    out["passes"] = npass
    out["per_pass_ms"] = out["passes_ms"] / max(1, npass)
    out["L_max"] = Lmax
    out["masked_mean"] = float(seed["nmask"].float().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--thr", type=float, default=0.999)
    ap.add_argument("--K", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark measures the GPU"
    import seeded_weights as SW
    from espnet_amd.nets.e2e_asr_maskctc import E2E

    ns = dict(SW.DECODE_R4["ns"], elayers=12, dlayers=6, maskctc_use_conformer_encoder=True)
    # blank bias 8 instead of 12: behind 12 encoder layers the seeded CTC layer then gives ~120 tokens per utterance (12: none)
    model = SW.decode_r4_model(E2E, dict(SW.DECODE_R4, ns=ns, blank_bias=8.0)).to("cuda:0").eval()
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(a.T, SW.DECODE_R4["idim"], generator=g) for _ in range(a.B)]
    ra = argparse.Namespace(maskctc_probability_threshold=a.thr, maskctc_n_iterations=a.K)
    t1 = timed(lambda: [model.recognize(x, ra) for x in xs], a.iters) / a.B
    tb = timed(lambda: model.recognize_batch(xs, ra), a.iters)
    res = dict(B=a.B, T=a.T, V=SW.DECODE_R4["odim"], elayers=12, dlayers=6, thr=a.thr, K=a.K,
               b1_ms_per_utt=t1 * 1e3, b1_utt_per_s=1.0 / t1, b32_ms_per_batch=tb * 1e3, b32_utt_per_s=a.B / tb,
               reference_cpu="not measured (the reference is not part of this repository)")
    res["split_b%d" % a.B] = split(model, torch.nn.utils.rnn.pad_sequence(xs, batch_first=True), [a.T] * a.B, a.thr, a.K, a.iters)
    res["split_b1"] = split(model, xs[0][None], [a.T], a.thr, a.K, a.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
