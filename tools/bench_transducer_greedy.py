#!/usr/bin/env python3
"""Batched greedy transducer decoding (BeamSearchTransducer.greedy_batch, csrc/rnnt_greedy.hip) at the width of BASELINE config 5
as tools/bench_rnn.py builds it: encoder states of T' = 374 frames x 256, one LSTM layer of 512 units behind a 512-wide
embedding, joint space 320, |V| = 5000; B = 1, 16 and 32 utterances per call.  Weights are seeded; lin_out's bias at blank is set
by bisection so that an utterance emits about `--tokens` labels (config 5 trains on 100 labels per 374 frames) - the cost of the
per-utterance search grows with the emitted labels, that of the batched one does not, so the figure is part of the result.

  batched     utt/s of greedy_batch, eager and with graph_steps (host clock around calls that end in their one device-to-host
              copy), the time per frame step, and the kernel launches per frame (counted in the captured graph)
  per_utt     utt/s of B calls of the per-utterance greedy search (BeamSearchTransducer.__call__, beam_size 1) on the same states
  validation  one eval-mode forward of the config 5 model with report_cer (B = 16, T = 1500, 100 labels): ErrorCalculatorTransducer
              decoding all rows with greedy_batch, and with the per-utterance loop it used before

Usage: python tools/bench_transducer_greedy.py [--iters 20] [--out profiles/transducer_greedy_bench.json] [--no-validation]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEV = "cuda"


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def wall(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return median(ts)


def calibrate(search, lin_out, hs, tokens):
    """lin_out.bias[blank] by bisection until greedy_batch emits about `tokens` labels per row of hs"""
    base = float(lin_out.bias.data[0])
    lo, hi = -20.0, 40.0
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        lin_out.bias.data[0] = base + mid
        n = sum(len(h.yseq) - 1 for h in search.greedy_batch(hs)) / hs.shape[0]
        if n > tokens:
            lo = mid
        else:
            hi = mid
    return n


def bench_decoder(a):
    from espnet_amd import graphs
    from espnet_amd.nets.beam_search_transducer import BeamSearchTransducer
    from espnet_amd.nets.transducer.rnn_decoder import DecoderRNNT
    torch.manual_seed(0)
    dec = DecoderRNNT(256, a.V, "lstm", 1, 512, 0, 512, 320, "tanh").to(DEV).eval()
    with torch.no_grad():
        dec.embed.weight.normal_(0, 1)
        dec.embed.weight[0].zero_()
        dec.joint_network.lin_out.weight.normal_(0, 2.0 / 320 ** 0.5)
    g = torch.Generator().manual_seed(1)
    res = {}
    search = BeamSearchTransducer(decoder=dec, beam_size=1)
    hs16 = torch.randn(16, a.T, 256, generator=g).to(DEV)
    res["tokens_per_utt"] = calibrate(search, dec.joint_network.lin_out, hs16, a.tokens)
    for B in (1, 16, 32):
        hs = torch.randn(B, a.T, 256, generator=g).to(DEV)
        eager = BeamSearchTransducer(decoder=dec, beam_size=1)
        graphed = BeamSearchTransducer(decoder=dec, beam_size=1)
        graphed.graph_steps = True
        want = eager.greedy_batch(hs)
        t_e = wall(lambda: eager.greedy_batch(hs), a.iters)
        t_g = wall(lambda: graphed.greedy_batch(hs), a.iters, warm=3)
        assert graphed.graph_steps, "the frame graph was not captured"
        assert [h.yseq for h in graphed.greedy_batch(hs)] == [h.yseq for h in want]
        ws = next(iter(graphed._greedy_graphs.values()))
        kinds = graphs.node_census(ws["graph"])[0]
        one = search(hs[0])
        assert one.yseq == want[0].yseq, "batched and per-utterance searches disagree"
        t_u = wall(lambda: [search(hs[b]) for b in range(B)], max(2, a.iters // 4), warm=1)
        res["B%d" % B] = dict(
            batched_eager=dict(utt_per_s=B / t_e, call_ms=t_e * 1e3, frame_step_us=t_e * 1e6 / a.T),
            batched_graph=dict(utt_per_s=B / t_g, call_ms=t_g * 1e3, frame_step_us=t_g * 1e6 / a.T,
                               launches_per_frame=kinds.get("kernel", 0) / 2, graph_nodes=kinds),
            per_utt=dict(utt_per_s=B / t_u, call_ms=t_u * 1e3),
            speedup_eager=t_u / t_e, speedup_graph=t_u / t_g,
            tokens_per_utt=sum(len(h.yseq) - 1 for h in want) / B)
    return res


def bench_validation(a):
    """eval-mode forward of config 5 with report_cer: greedy_batch inside ErrorCalculatorTransducer against the per-utterance loop"""
    import argparse as ap
    from espnet_amd import ops
    from espnet_amd.nets.e2e_asr_transducer import E2E
    arch = [dict(type="conformer", d_hidden=256, d_ff=2048, heads=4, macaron_style=True, use_conv_mod=True, conv_mod_kernel=31)]
    V, B, T, L = a.V, 16, 1500, 100
    ns = ap.Namespace(etype="transformer", enc_block_arch=arch, enc_block_repeat=12, transformer_enc_input_layer="conv2d",
                      transformer_enc_self_attn_type="rel_self_attn", transformer_enc_positional_encoding_type="rel_pos",
                      transformer_enc_pw_activation_type="swish", transformer_enc_conv_mod_activation_type="swish",
                      dtype="lstm", dlayers=1, dunits=512, dec_embed_dim=512, joint_dim=320, joint_activation_type="tanh",
                      dropout_rate_decoder=0.0, dropout_rate_embed_decoder=0.0, rnnt_mode="rnnt", trans_type="warp-transducer",
                      sym_space="<space>", sym_blank="<blank>", transformer_init="pytorch", report_cer=True, report_wer=False,
                      char_list=["<blank>"] + ["t%d" % i for i in range(1, V - 1)] + ["<eos>"])
    torch.manual_seed(0)
    m = E2E(80, V, ns).to(DEV).eval()
    g = torch.Generator().manual_seed(0)
    xs = torch.randn(B, T, 80, generator=g).to(DEV)
    ilens = [T - 11 * i for i in range(B)]
    ys = torch.randint(1, V - 1, (B, L), generator=g).to(DEV)
    ec = m.error_calculator
    with torch.no_grad():
        m(xs, ilens, ys)
        n = calibrate(ec.beam_search, m.dec.joint_network.lin_out, m.hs_pad.detach(), a.tokens)

        def forward():
            m(xs, ilens, ys)
            return m.cer

        t_new = wall(forward, max(3, a.iters // 4), warm=2)
        cer_new = forward()

        def loop(hs_pad):      # ErrorCalculatorTransducer.hypotheses before greedy_batch: the per-utterance search on every padded row
            ys_hat = [list(ec.beam_search(hs_pad[b]).yseq[1:]) for b in range(int(hs_pad.size(0)))]
            width = max(1, max(len(y) for y in ys_hat))
            host = torch.full((len(ys_hat), width), -1, dtype=torch.int32)
            for b, y in enumerate(ys_hat):
                host[b, : len(y)] = torch.tensor(y, dtype=torch.int32)
            return ops.h2d_async(host, hs_pad.device)

        ec.hypotheses = loop
        t_old = wall(forward, max(3, a.iters // 4), warm=1)
        cer_old = forward()
        del ec.hypotheses
    return dict(B=B, T=T, frames=int(m.hs_pad.shape[1]), tokens_per_utt=n, forward_ms_greedy_batch=t_new * 1e3,
                forward_ms_per_utt_loop=t_old * 1e3, cer_greedy_batch=cer_new, cer_per_utt_loop=cer_old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--T", type=int, default=374)
    ap.add_argument("--V", type=int, default=5000)
    ap.add_argument("--tokens", type=float, default=100.0)
    ap.add_argument("--no-validation", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark measures the GPU"
    import espnet_amd
    espnet_amd.set_precision("fp32")
    res = dict(T=a.T, V=a.V, D_enc=256, dunits=512, embed=512, joint=320)
    res.update(bench_decoder(a))
    if not a.no_validation:
        res["validation"] = bench_validation(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
