#!/usr/bin/env python3
"""Multi-speaker Transformer ASR at the wsj_mix recipe's size (train_multispkr_transformer.yaml: adim 256, aheads 4, 4 speaker
layers + 8 shared encoder layers, 6 decoder layers, eunits = dunits = 2048, mtlalpha 0.2, lsm 0.1), S = 2, B = 16 utterances of
~800 input frames (T' ~ 199), ~100 labels per speaker, |V| = 52, seeded weights and inputs, fp32.

  train_eager_ms      one eager training step (forward_core + backward + Adam), device-synchronised host clock
  train_graph_ms      the same step replayed by train.BucketedGraphStep
  pit_ms              eamd_ctc_pit_loss with gradient on [S, B, T', V] activations
  pit_ref_ms          the reference's structure on our kernels: S^2 eamd_ctc_loss calls with gradient, the pair matrix read by the
                      host and the permutations chosen there (PIT.pit_process)
  dec_b1_utt_per_s    recognize() one utterance at a time (each gives S n-best lists), beam 10, ctc_weight 0.3
  dec_b32_utt_per_s   recognize_batch() on 32 utterances at once
Each timing is the median of --iters windows after a warm-up of the same shapes.  Writes the JSON line to
profiles/asr_mix_bench.json (or --out).
Usage: python tools/bench_asr_mix.py [--iters 10] [--out profiles/asr_mix_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

RECIPE = dict(adim=256, aheads=4, elayers=8, elayers_sd=4, eunits=2048, dlayers=6, dunits=2048, mtlalpha=0.2, lsm_weight=0.1,
              dropout_rate=0.1, transformer_attn_dropout_rate=0.0, transformer_length_normalized_loss=False,
              transformer_init="pytorch", transformer_input_layer="conv2d", num_spkrs=2)
IDIM, ODIM = 80, 52


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def train_batch(B, T, L, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    ilens = torch.randint(T - 64, T + 1, (B,), generator=g)
    ilens[0] = T
    xs = torch.randn(B, T, IDIM, generator=g)
    ys = torch.full((B, S, L), -1, dtype=torch.int64)
    for b in range(B):
        for s in range(S):
            n = int(torch.randint(L - 20, L + 1, (1,), generator=g))
            ys[b, s, :n] = torch.randint(1, ODIM - 1, (n,), generator=g)
    return xs, ilens.tolist(), ys


def pit_reference_structure(acts, ys, il, perms):
    """S^2 eamd_ctc_loss calls, the pair matrix to the host, the choice there (the reference's loop on our kernels)"""
    from espnet_amd import ops
    S, B = acts.shape[:2]
    pair = torch.stack([ops.ctc_loss(acts[i], ys[:, j].contiguous(), il, 0, -1, 1.0 / B)[0] / B
                        for i in range(S) for j in range(S)], 1).cpu()
    out = []
    for b in range(B):
        sc = torch.stack([sum(pair[b, i * S + p[i]] for i in range(S)) for p in perms]) / S
        v, k = torch.min(sc, 0)
        out.append((float(v), perms[int(k)]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=800)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--dec-utts", type=int, default=32)
    ap.add_argument("--dec-T", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asr_mix_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark measures the GPU"
    import seeded_weights as SW
    from espnet_amd import ops, train
    from espnet_amd.nets.e2e_asr_mix_transformer import E2E, pit_permutations

    dev = "cuda:0"
    S = RECIPE["num_spkrs"]
    res = dict(S=S, B=a.B, T=a.T, L=a.L, V=ODIM, adim=256, elayers_sd=4, elayers=8, dlayers=6, units=2048, iters=a.iters)

    # ---- training step ------------------------------------------------------------------------------------------------
    xs, il, ys = train_batch(a.B, a.T, a.L, S)
    olens = (ys != -1).sum(-1).max(-1).values.tolist()

    def make():
        torch.manual_seed(0)
        m = SW.fill_parameters(E2E(IDIM, ODIM, argparse.Namespace(**RECIPE)), salt=3).to(dev).train()
        m.sync_report = False
        flat = train.FlatParams(m)
        return m, flat, train.NoamAdam(flat, mode="const", base_lr=0.0, max_grad_norm=5.0)
    m, flat, opt = make()
    res["train_eager_ms"] = 1e3 * timed(lambda: train.train_step(m, flat, opt, m.prepare(xs, il, ys)), a.iters)
    loss_eager = float(train.train_step(m, flat, opt, m.prepare(xs, il, ys)).detach())
    del m, flat, opt
    bstep = train.BucketedGraphStep(*make(), t_edge=64, l_edge=8)
    bstep(xs, il, ys, olens)                        # first sight: eager; the timed() warm-up captures
    res["train_graph_ms"] = 1e3 * timed(lambda: bstep(xs, il, ys, olens), a.iters)
    res["train_graph_stats"] = bstep.stats()
    res["loss_eager"], res["loss_graph"] = loss_eager, float(bstep(xs, il, ys, olens).detach())
    T1 = (((a.T - 1) // 2 - 1) // 2)
    res["T_enc"] = T1
    del bstep
    torch.cuda.empty_cache()

    # ---- PIT CTC alone ------------------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(1)
    acts = torch.randn(S, a.B, T1, ODIM, generator=g).to(dev)
    hl = torch.tensor([(((v - 1) // 2 - 1) // 2) for v in il], dtype=torch.int32).to(dev)
    ysd = ys.to(dev).contiguous()
    perms = pit_permutations(S)
    scale = 1.0 / (S * a.B * a.B)
    res["pit_ms"] = 1e3 * timed(lambda: ops.ctc_pit_loss(acts, ysd, hl, 0, -1, scale), a.iters)
    res["pit_ref_ms"] = 1e3 * timed(lambda: pit_reference_structure(acts, ysd, hl, perms), a.iters)
    _, perm, pit, _ = ops.ctc_pit_loss(acts, ysd, hl, 0, -1, scale)
    ref = pit_reference_structure(acts, ysd, hl, perms)
    res["pit_same_choice"] = perm.cpu().tolist() == [p for _, p in ref]
    res["pit_max_rel_diff"] = float(max(abs(float(x) - r) / abs(r) for x, (r, _) in zip(pit.cpu(), ref)))

    # ---- decoding -----------------------------------------------------------------------------------------------------
    spec = dict(idim=IDIM, odim=ODIM, salt=4, out_scale=4.0, eos_bias=7.0, blank_bias=12.0, ns=dict(RECIPE, dropout_rate=0.0))
    model = SW.decode_r4_model(E2E, spec).to(dev)
    g = torch.Generator().manual_seed(2)
    utts = [torch.randn(a.dec_T - 8 * (k % 5), IDIM, generator=g) for k in range(a.dec_utts)]
    ra = argparse.Namespace(beam_size=10, penalty=0.0, maxlenratio=0.0, minlenratio=0.0, ctc_weight=0.3, lm_weight=0.0, nbest=1)
    n1 = min(8, len(utts))
    t1 = timed(lambda: [model.recognize(x, ra) for x in utts[:n1]], max(1, a.iters // 5))
    tb = timed(lambda: model.recognize_batch(utts, ra), max(1, a.iters // 5))
    single = [model.recognize(x, ra) for x in utts[:n1]]
    batch = model.recognize_batch(utts, ra)
    res.update(dec_b1_ms_per_utt=1e3 * t1 / n1, dec_b1_utt_per_s=n1 / t1, dec_b32_ms_per_batch=1e3 * tb,
               dec_b32_utt_per_s=len(utts) / tb,
               dec_batch_equals_single=all([h[0]["yseq"] for h in batch[k]] == [h[0]["yseq"] for h in single[k]]
                                           for k in range(n1)),
               dec_mean_len=float(np.mean([len(h[0]["yseq"]) for u in batch for h in u])))
    line = json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
