#!/usr/bin/env python
"""Times speech-enhancement training on the HIP kernels of csrc/enh.hip at B = 32, 4 s of 16 kHz audio, n_fft 512 / hop 128,
S = 2, and in the same run the reference's formulas composed from torch ops on the device (restated here, not imported),
alternating the two.  Writes one JSON file.

    python tools/bench_enh.py [--out profiles/enh_bench.json] [--B 32 --seconds 4 --S 2]

  istft        ops.istft forward and forward + backward against torch.istft (rectangular synthesis window, as the reference)
  loss paths   labels -> pair matrix -> permutation, forward and forward + backward: mask_mse (IRM, PSM), magnitude,
               spectrum on [B, T, F] and both SI-SNR criteria on [B, L], against the reference's loop over permutations
  train step   one TFMaskingNet (3 x 512 BLSTM) step, forward + backward, per loss type

Times are device events around at least `iters` calls and at least 50 ms of work after `warmup` calls; the best of `rounds`
alternating rounds is reported and every round is kept.  For the streaming kernels the JSON also gives the least traffic of
one read of every operand and one write of every result per pass, and the achieved share of 6.3 TB/s that this traffic over
the measured time amounts to (6.3 TB/s is the HBM rate the chip reaches, not the 8 TB/s peak that older tables of DESIGN.md
divide by: multiply by 0.79 to compare).  The times of the loss paths are those of all their launches (pair, finish, pick),
so the share is an end-to-end figure of the path, not of one kernel."""
import argparse
import json
import os
import sys
from itertools import permutations

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.3e12
WINDOW_MS = 50.0            # the least a timed window lasts: shorter ones measure the clock and the scheduler


def timed(fn, warmup, iters):
    """ms per call over at least `iters` calls and at least WINDOW_MS of work (the call count comes from a first window of
    `iters` calls, so the 25 - 60 us paths are timed over one to two thousand calls)"""
    first = _window(fn, warmup, iters)
    more = int(WINDOW_MS / max(first, 1e-4)) + 1
    return first if more <= iters else _window(fn, 0, more)


def _window(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


# ---- the reference's formulas in torch, on complex tensors -------------------------------------------------------------
def t_label(mix, refs, mask_type):
    eps = 10e-8
    out = []
    for r in refs:
        if mask_type == "IRM":
            m = abs(r) / (sum(abs(n) for n in refs) + eps)
        else:                                                         # PSM
            pr, pm = r / (abs(r) + eps), mix / (abs(mix) + eps)
            m = ((abs(r) / (abs(mix) + eps)) * (pr.real * pm.real + pr.imag * pm.imag)).clamp(min=-1, max=1)
        out.append(m)
    return out


def t_mse(ref, inf):
    return (abs(ref - inf) ** 2).mean(dim=[1, 2])


def t_si_snr(ref, inf):
    ref = ref / torch.norm(ref, p=2, dim=1, keepdim=True)
    inf = inf / torch.norm(inf, p=2, dim=1, keepdim=True)
    s_target = (ref * inf).sum(dim=1, keepdims=True) * ref
    return -20 * torch.log10(torch.norm(s_target, p=2, dim=1) / torch.norm(inf - s_target, p=2, dim=1))


def t_si_snr_zeromean(ref, inf):
    eps = 1e-8
    T = ref.shape[1]
    s = ref - torch.sum(ref, dim=1, keepdim=True) / T
    e = inf - torch.sum(inf, dim=1, keepdim=True) / T
    proj = torch.sum(e * s, dim=1, keepdim=True) * s / (torch.sum(s ** 2, dim=1, keepdim=True) + eps)
    ratio = torch.sum(proj ** 2, dim=1) / (torch.sum((e - proj) ** 2, dim=1) + eps)
    return -10 * torch.log10(ratio + eps)


def t_pit(ref, inf, criterion):
    losses = torch.stack([sum(criterion(ref[s], inf[t]) for s, t in enumerate(p)) / len(p)
                          for p in permutations(range(len(ref)))], dim=1)
    loss, perm = torch.min(losses, dim=1)
    return loss.mean(), perm


def main():
    ap = argparse.ArgumentParser()
    for k, v in dict(B=32, seconds=4, S=2, n_fft=512, hop=128, warmup=3, iters=10, rounds=3).items():
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enh_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_enh.py needs a GPU: a timing taken anywhere else says nothing")
    from espnet_amd import ops
    from espnet_amd.espnet2.enh import ESPnetEnhancementModel, TFMaskingNet
    from espnet_amd.espnet2.frontend import Stft
    dev = "cuda"
    B, S, N, hop = a.B, a.S, a.n_fft, a.hop
    L = 16000 * a.seconds
    F = N // 2 + 1
    T = L // hop + 1
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    fns, traffic = {}, {}

    # ---- istft -------------------------------------------------------------------------------------------------------
    st = Stft(N, None, hop)
    spec = rnd(B, T, F, 2)
    gw = rnd(B, L)
    ones = torch.ones(N, device=dev)

    def hip_istft():
        with torch.no_grad():
            return st.inverse(spec, [L] * B)[0]

    def hip_istft_bwd():
        s = spec.detach().requires_grad_(True)
        st.inverse(s, [L] * B)[0].backward(gw)
        return s.grad

    def torch_istft_of(s):
        return torch.istft(torch.view_as_complex(s).transpose(1, 2), N, hop, N, window=ones, center=True, length=L)

    def torch_istft():
        with torch.no_grad():
            return torch_istft_of(spec)

    def torch_istft_bwd():
        s = spec.detach().requires_grad_(True)
        torch_istft_of(s).backward(gw)
        return s.grad

    agree = dict(istft=float((hip_istft() - torch_istft()).abs().max() / torch_istft().abs().max()),
                 istft_grad=float((hip_istft_bwd() - torch_istft_bwd()).abs().max() / torch_istft_bwd().abs().max()))
    fns.update(hip_istft_fwd=hip_istft, torch_istft_fwd=torch_istft, hip_istft_fwd_bwd=hip_istft_bwd,
               torch_istft_fwd_bwd=torch_istft_bwd)
    frames = 4 * B * T * N
    traffic["hip_istft_fwd"] = 4 * B * T * 2 * F + 2 * frames + 4 * B * L       # spectrum, frames written and read, waveform

    # ---- loss paths ----------------------------------------------------------------------------------------------------
    refs = rnd(S, B, T, F, 2)
    mix = (refs.sum(0) + 0.1 * rnd(B, T, F, 2)).contiguous()
    logits = rnd(S, B, T, F)
    est = (refs.flip(0) + 0.3 * rnd(S, B, T, F, 2)).contiguous()
    wref = rnd(S, B, L)
    west = (wref.flip(0) + 0.3 * rnd(S, B, L)).contiguous()
    cmix, crefs = torch.view_as_complex(mix), [torch.view_as_complex(r) for r in refs]

    def hip_tf(e, ref, mx, mode, label, act, backward):
        def run():
            x = e.detach().requires_grad_(backward)
            loss, perm = ops.EnhTFLossFn.apply(x, ref, mx, mode, label, act, None)
            if backward:
                loss.mean().backward()
                return x.grad
            return loss
        return run

    def torch_tf(kind, backward):
        def run():
            with torch.set_grad_enabled(backward):
                if kind in ("IRM", "PSM"):
                    x = logits.detach().requires_grad_(backward)
                    loss, _ = t_pit(t_label(cmix, crefs, kind), list(torch.sigmoid(x)), t_mse)
                else:
                    x = est.detach().requires_grad_(backward)
                    inf = [torch.view_as_complex(v) for v in x]
                    if kind == "magnitude":
                        loss, _ = t_pit([abs(r) for r in crefs], [abs(v) for v in inf], t_mse)
                    else:
                        loss, _ = t_pit(crefs, inf, t_mse)
                if backward:
                    loss.backward()
                    return x.grad
                return loss
        return run

    n = T * F
    for kind in ("IRM", "PSM", "magnitude", "spectrum"):
        if kind in ("IRM", "PSM"):
            args = (logits, refs, mix, ops.ENH_MASK, ops.ENH_LABELS[kind], ops.ENH_ACTS["sigmoid"])
            read = 4 * B * n * (S + 2 * S + 2)
            write = 4 * B * n * S
        else:
            args = (est, refs, None, ops.ENH_MAG if kind == "magnitude" else ops.ENH_SPEC, 0, 3)
            read = 4 * B * n * 4 * S
            write = 4 * B * n * 2 * S
        for bw in (False, True):
            tag = "%s_%s" % (kind, "fwd_bwd" if bw else "fwd")
            fns["hip_" + tag], fns["torch_" + tag] = hip_tf(*args, bw), torch_tf(kind, bw)
            traffic["hip_" + tag] = read + (read + write if bw else 0)
        a_, b_ = hip_tf(*args, True)(), torch_tf(kind, True)()
        agree[kind + "_grad"] = float((a_ - b_).abs().max() / b_.abs().max())

    def hip_snr(mode, backward):
        def run():
            x = west.detach().requires_grad_(backward)
            loss, _ = ops.EnhSisnrLossFn.apply(x, wref, mode, None)
            if backward:
                loss.mean().backward()
                return x.grad
            return loss
        return run

    def torch_snr(crit, backward):
        def run():
            with torch.set_grad_enabled(backward):
                x = west.detach().requires_grad_(backward)
                loss, _ = t_pit(list(wref), list(x), crit)
                if backward:
                    loss.backward()
                    return x.grad
                return loss
        return run

    for name, mode, crit in (("si_snr_zeromean", ops.ENH_SNR_ZEROMEAN, t_si_snr_zeromean), ("si_snr", ops.ENH_SNR_L2NORM, t_si_snr)):
        for bw in (False, True):
            tag = "%s_%s" % (name, "fwd_bwd" if bw else "fwd")
            fns["hip_" + tag], fns["torch_" + tag] = hip_snr(mode, bw), torch_snr(crit, bw)
            traffic["hip_" + tag] = 4 * B * L * 2 * S + (4 * B * L * 3 * S if bw else 0)
        a_, b_ = hip_snr(mode, True)(), torch_snr(crit, True)()
        agree[name + "_grad"] = float((a_ - b_).abs().max() / b_.abs().max())

    def hip_mask_apply():
        return ops.enh_mask_apply(logits, mix, 0)
    fns["hip_mask_apply"] = hip_mask_apply
    traffic["hip_mask_apply"] = 4 * B * n * (S + 2 + S + 2 * S)

    # ---- one training step per loss type ---------------------------------------------------------------------------------
    batch = dict(speech_mix=rnd(B, L))
    batch.update({"speech_ref%d" % (s + 1): rnd(B, L) for s in range(S)})
    lens = torch.full((B,), L)

    def step_of(loss_type):
        net = TFMaskingNet(n_fft=N, hop_length=hop, num_spk=S, loss_type="spectrum" if loss_type == "si_snr" else loss_type)
        net.loss_type = loss_type
        m = ESPnetEnhancementModel(net).to(dev).train()

        def run():
            m.zero_grad(set_to_none=True)
            loss, _, _ = m(batch["speech_mix"], lens, **{k: v for k, v in batch.items() if k != "speech_mix"})
            loss.backward()
            return loss
        return run
    for lt in ("mask_mse", "magnitude", "spectrum", "si_snr"):
        fns["train_step_" + lt] = step_of(lt)

    times = {k: [] for k in fns}
    for _ in range(a.rounds):                                           # alternate: other work shares the machine
        for k, fn in fns.items():
            times[k].append(timed(fn, a.warmup, a.iters))
    ms = {k: min(v) for k, v in times.items()}
    share = {k: traffic[k] / (ms[k] * 1e-3) / HBM for k in traffic}
    res = dict(shape=dict(B=B, L=L, T=T, F=F, S=S, n_fft=N, hop=hop), device=torch.cuda.get_device_name(0), warmup=a.warmup,
               iters=a.iters, rounds=a.rounds, ms_best=ms, ms_all=times, min_traffic_bytes=traffic, share_of_6p3_TBps=share,
               max_rel_diff_hip_vs_torch=agree,
               speedup_vs_torch={k[4:]: ms["torch_" + k[4:]] / ms[k] for k in ms if k.startswith("hip_") and "torch_" + k[4:] in ms})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "ms_all"}))


if __name__ == "__main__":
    main()
