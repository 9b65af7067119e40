"""Speech enhancement training restated in torch from the formulas (float64 / complex128 by default): the yardstick of
csrc/enh.hip, ops.istft, Stft.inverse and espnet2/enh.py.  Test infrastructure only - the product tree never imports it.

Spectra are torch complex tensors here: mix [B, ...], refs and estimates lists of S such tensors (or stacked [S, B, ...]).
Every function runs in the dtype of its inputs, so the same code in float32 / complex64 on the CPU gives the error an
fp32 evaluation in library order makes.

Restated from: espnet2/layers/stft.py:116-157 over torch.istft's definition (inverse DFT of every frame, synthesis window,
overlap-add, division by the summed squared window, trimming), espnet2/enh/espnet_model.py (labels :47-104, criteria
:312-405, permutation loss :407-434, forward :106-310), espnet2/enh/nets/tf_mask_net.py and beamformer_net.py."""
import itertools
import math

import torch

import beamformer_restatement as R

MASK_EPS = 10e-12        # tf_mask_net.py:95, the literal
LABEL_EPS = 10e-8        # espnet_model.py:64, the literal
SNR_EPS = 1e-8
LABELS = ("IBM", "IRM", "IAM", "PSM", "NPSM", "PSM^2")
ACTS = {"sigmoid": torch.sigmoid, "relu": torch.relu, "tanh": torch.tanh, "none": lambda x: x}

cx, ri, err_vs = R.cx, R.ri, R.err_vs


def cabs(z):
    return (z.real ** 2 + z.imag ** 2) ** 0.5


# ---- STFT and its inverse ------------------------------------------------------------------------------------------------
def full_window(win_length, n_fft, name, dtype=torch.float64):
    """the window of win_length centred in n_fft; name None: ones"""
    w = torch.ones(win_length, dtype=dtype) if name is None else getattr(torch, name + "_window")(win_length, dtype=dtype)
    left = (n_fft - win_length) // 2
    out = torch.zeros(n_fft, dtype=dtype)
    out[left:left + win_length] = w
    return out


def stft(x, n_fft, hop, win_length=None, window="hann", center=True, normalized=False, onesided=True):
    """x [B, L] real -> [B, T, F] complex: reflect padding, frames, window, DFT as a matrix product"""
    win_length = n_fft if win_length is None else win_length
    w = full_window(win_length, n_fft, window, x.dtype)
    if center:
        x = torch.nn.functional.pad(x[:, None], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
    fr = x.unfold(1, n_fft, hop) * w                                             # [B, T, N]
    F = n_fft // 2 + 1 if onesided else n_fft
    ang = -2.0 * math.pi * torch.arange(F, dtype=x.dtype)[:, None] * torch.arange(n_fft, dtype=x.dtype)[None, :] / n_fft
    spec = torch.complex(fr @ torch.cos(ang).T, fr @ torch.sin(ang).T)
    return spec * n_fft ** -0.5 if normalized else spec


def istft(spec, n_fft, hop, win_length=None, window=None, center=True, normalized=False, onesided=True, length=None):
    """spec [B, T, F] complex -> [B, length] real.  window: None = rectangular (the reference passes none), a window
    name, or n_fft values."""
    win_length = n_fft if win_length is None else win_length
    rdt = spec.real.dtype
    w = window.to(rdt) if torch.is_tensor(window) else full_window(win_length, n_fft, window, rdt)
    B, T, F = spec.shape
    k = torch.arange(n_fft, dtype=rdt)
    ang = 2.0 * math.pi * torch.arange(F, dtype=rdt)[:, None] * k[None, :] / n_fft   # [F, N]
    # a real signal is rebuilt from bins 0 .. N/2 alone (a c2r transform): the conjugate half is folded in, the imaginary
    # parts of DC and Nyquist drop out; a two-sided input's upper bins are not read (torch.istft slices them off)
    half = torch.arange(F) <= n_fft // 2
    c = 2.0 * half.to(rdt)
    c[0] = 1.0
    if n_fft % 2 == 0:
        c[n_fft // 2] = 1.0
    scale = c / n_fft * (n_fft ** 0.5 if normalized else 1.0)
    sin = torch.sin(ang)
    sin[0] = 0.0
    if n_fft % 2 == 0:
        sin[n_fft // 2] = 0.0
    frames = (spec.real * scale) @ torch.cos(ang) - (spec.imag * scale) @ sin    # [B, T, N]
    full = hop * (T - 1) + n_fft
    y = torch.zeros(B, full, dtype=rdt)
    env = torch.zeros(full, dtype=rdt)
    for t in range(T):
        y[:, t * hop:t * hop + n_fft] = y[:, t * hop:t * hop + n_fft] + frames[:, t] * w
        env[t * hop:t * hop + n_fft] += w * w
    start = n_fft // 2 if center else 0
    end = full - start if length is None else min(start + length, full)
    if not float(env[start:end].abs().min()) > 1e-11:
        raise RuntimeError("window overlap add min")
    out = y[:, start:end] / env[start:end]
    if length is not None and out.shape[1] < length:
        out = torch.nn.functional.pad(out, (0, length - out.shape[1]))
    return out


# ---- masks ---------------------------------------------------------------------------------------------------------------
def mask_label(mix, refs, mask_type):
    """the ideal-mask labels of the S references (espnet_model.py:47-104).  NPSM is clamped to [-1, 1] like PSM: the
    reference compares the list it is filling, not mask_type, with "NPSM"."""
    assert mask_type in LABELS
    ax = cabs(mix)
    out = []
    for r in refs:
        ar = cabs(r)
        if mask_type == "IBM":
            m = torch.ones_like(ar)
            for n in refs:
                m = m * (ar >= cabs(n)).to(ar.dtype)
        elif mask_type == "IRM":
            m = ar / (sum(cabs(n) for n in refs) + LABEL_EPS)
        elif mask_type == "IAM":
            m = (ar / (ax + LABEL_EPS)).clamp(0, 1)
        else:
            pr, pm = r / (ar + LABEL_EPS), mix / (ax + LABEL_EPS)
            cos = pr.real * pm.real + pr.imag * pm.imag
            m = (ar ** 2 / (ax ** 2 + LABEL_EPS) if mask_type == "PSM^2" else ar / (ax + LABEL_EPS)) * cos
            m = m.clamp(-1, 1)
        out.append(m)
    return out


def mask_apply(logits, mix, act):
    """logits [S, B, ...] -> (masks [S, B, ...], P [S, B, ...] complex = mix / (|mix| + 10e-12) * (|mix| mask))"""
    m = ACTS[act](logits)
    ax = cabs(mix)
    return m, (mix / (ax + MASK_EPS)) * (ax * m)


def mask_apply_bwd(logits, mix, act, gmask, gP):
    """the kernel's closed form: dlogits = act'(logits) (gmask + Re(conj(X) gP) |X| / (|X| + 10e-12))"""
    m = ACTS[act](logits)
    d = {"sigmoid": m * (1 - m), "relu": (logits > 0).to(m.dtype), "tanh": 1 - m * m, "none": torch.ones_like(m)}[act]
    ax = cabs(mix)
    return d * (gmask + ax / (ax + MASK_EPS) * (mix.real * gP.real + mix.imag * gP.imag))


# ---- criteria ------------------------------------------------------------------------------------------------------------
def tf_mse_loss(ref, inf):
    """mean over everything but the batch of |ref - inf|^2; the mean runs over the whole padded extent"""
    d = ref - inf
    sq = d.real ** 2 + d.imag ** 2 if d.is_complex() else d ** 2
    return sq.flatten(1).mean(dim=1)


def tf_l1_loss(ref, inf):
    d = ref - inf
    return (cabs(d) if d.is_complex() else d.abs()).flatten(1).mean(dim=1)


def mag_mse_loss(ref, inf, zero_grad_at_zero=True):
    """(|ref| - |inf|)^2; |inf| takes gradient 0 at inf = 0 (this project's departure: the reference's is NaN)"""
    a = inf.real ** 2 + inf.imag ** 2
    ai = torch.where(a > 0, a, torch.ones_like(a)) ** 0.5 * (a > 0).to(a.dtype) if zero_grad_at_zero else a ** 0.5
    return ((cabs(ref) - ai) ** 2).flatten(1).mean(dim=1)


def si_snr_loss(ref, inf):
    """espnet_model.py:348-364: both L2-normalised, no eps"""
    ref = ref / ref.norm(dim=1, keepdim=True)
    inf = inf / inf.norm(dim=1, keepdim=True)
    s_target = (ref * inf).sum(dim=1, keepdim=True) * ref
    e_noise = inf - s_target
    return -20 * torch.log10(s_target.norm(dim=1) / e_noise.norm(dim=1))


def si_snr_loss_zeromean(ref, inf):
    """espnet_model.py:367-405: means over the full padded length, eps 1e-8 in three places"""
    L = ref.shape[1]
    s = ref - ref.sum(dim=1, keepdim=True) / L
    e = inf - inf.sum(dim=1, keepdim=True) / L
    dot = (e * s).sum(dim=1, keepdim=True)
    energy = (s ** 2).sum(dim=1, keepdim=True) + SNR_EPS
    proj = dot * s / energy
    noise = e - proj
    ratio = (proj ** 2).sum(dim=1) / ((noise ** 2).sum(dim=1) + SNR_EPS)
    return -10 * torch.log10(ratio + SNR_EPS)


def si_snr_sums(ref, inf):
    """what the kernel gathers per utterance: (sum r, sum r^2, sum e, sum e^2, sum r e)"""
    return ref.sum(1), (ref ** 2).sum(1), inf.sum(1), (inf ** 2).sum(1), (ref * inf).sum(1)


def si_snr_closed_form(sums, L, zeromean=True):
    """the criterion and the coefficients of d loss / d e_i = a e_i + b r_i + c from the five sums"""
    sr, srr, se, see, sre = sums
    k10 = 10.0 / math.log(10.0)
    if zeromean:
        D, Er, Ee = sre - sr * se / L, srr - sr * sr / L, see - se * se / L
        te = Er + SNR_EPS
        k = 2 / te - Er / te ** 2
        P, N = D * D * Er / te ** 2, Ee - D * D * k + SNR_EPS
        q = P / N + SNR_EPS
        g = -k10 / q
        a = -g * 2 * P / N ** 2
        b = g * (2 * D * Er / (te ** 2 * N) + 2 * D * k * P / N ** 2)
        return -k10 * torch.log(q), a, b, -(a * se + b * sr) / L
    M = srr * see - sre * sre
    return -k10 * torch.log(sre * sre / M), k10 * 2 * srr / M, -k10 * (2 / sre + 2 * sre / M), torch.zeros_like(M)


# ---- permutation ---------------------------------------------------------------------------------------------------------
def pair_matrix(ref, inf, criterion):
    """[B, S, S]: criterion(reference s, estimate t)"""
    return torch.stack([torch.stack([criterion(r, e) for e in inf], dim=1) for r in ref], dim=1)


def permutation_losses(pair):
    """[B, S!]: sum_s pair[b, s, perm[s]] / S in itertools.permutations order"""
    S = pair.shape[1]
    return torch.stack([sum(pair[:, s, t] for s, t in enumerate(p)) / S for p in itertools.permutations(range(S))], dim=1)


def permutation_loss(ref, inf, criterion, perm=None):
    """espnet_model.py:407-434 per utterance -> (loss [B], perm [B]); the reference returns loss.mean()"""
    losses = permutation_losses(pair_matrix(ref, inf, criterion))
    if perm is None:
        loss, perm = torch.min(losses, dim=1)                                  # the first minimum
    else:
        loss = losses[torch.arange(losses.shape[0]), perm]
    return loss, perm


def permutation_gap(ref, inf, criterion):
    """(second-best - best) / |best| permutation loss, the smallest over the batch (inf for S = 1)"""
    losses = permutation_losses(pair_matrix(ref, inf, criterion))
    if losses.shape[1] == 1:
        return float("inf")
    top = torch.sort(losses.detach(), dim=1).values
    return float(((top[:, 1] - top[:, 0]) / top[:, 0].abs()).min())


# ---- models --------------------------------------------------------------------------------------------------------------
def frame_lens(ilens, n_fft, hop, win_length=None, center=True):
    win_length = n_fft if win_length is None else win_length
    return [(int(n) + (2 * (win_length // 2) if center else 0) - win_length) // hop + 1 for n in ilens]


def stft_masked(x, ilens, n_fft, hop, **kw):
    """Stft.forward: frames past an utterance's frame count are zeroed"""
    spec = stft(x, n_fft, hop, **kw)
    fl = frame_lens(ilens, n_fft, hop, kw.get("win_length"), kw.get("center", True))
    keep = (torch.arange(spec.shape[1])[None, :] < torch.as_tensor(fl)[:, None]).to(spec.real.dtype)
    return spec * keep[:, :, None], fl


def _blstm(sd, prefix, xs, ilens):
    """encoders.RNN: stacked BLSTM over the packed batch, then tanh(Linear); padded frames carry tanh(bias)"""
    w0 = sd[prefix + "nbrnn.weight_ih_l0"]
    layers = len([k for k in sd if k.startswith(prefix + "nbrnn.weight_ih_l") and not k.endswith("_reverse")])
    lstm = torch.nn.LSTM(w0.shape[1], w0.shape[0] // 4, layers, batch_first=True, bidirectional=True).to(w0.dtype)
    names = [n for n, _ in lstm.named_parameters()]
    packed = torch.nn.utils.rnn.pack_padded_sequence(xs, torch.as_tensor(ilens), batch_first=True, enforce_sorted=False)
    ys, _ = torch.func.functional_call(lstm, {n: sd[prefix + "nbrnn." + n] for n in names}, (packed,))
    ys, _ = torch.nn.utils.rnn.pad_packed_sequence(ys, batch_first=True)
    return torch.tanh(torch.nn.functional.linear(ys, sd[prefix + "l_last.weight"], sd[prefix + "l_last.bias"]))


def utterance_mvn(x, lens, eps=1e-20):
    """UtteranceMVN(norm_means=True, norm_vars=True), utterance_mvn.py:62-88 literally: the mean over the utterance's own
    frames is subtracted from every frame, so the padding holds -mean and enters the variance, which is divided by the
    length; the divisor is sqrt(clamp(sqrt(var), eps))"""
    keep = (torch.arange(x.shape[1])[None, :] < torch.as_tensor(lens)[:, None]).to(x.dtype)[:, :, None]
    n = torch.as_tensor(lens, dtype=x.dtype)[:, None, None]
    x = x * keep
    x = x - x.sum(dim=1, keepdim=True) / n
    std = ((x ** 2).sum(dim=1, keepdim=True) / n).sqrt().clamp(min=eps)
    return x / std.sqrt()


def tf_masking_logits(sd, wav, ilens, n_fft, hop, num_spk, utt_mvn=False):
    """TFMaskingNet up to the heads -> (logits [S, B, T, F], mixture spectrum [B, T, F], frame lengths)"""
    spec, fl = stft_masked(wav, ilens, n_fft, hop)
    mag = cabs(spec)
    if utt_mvn:
        mag = utterance_mvn(mag, fl)
    h = _blstm(sd, "rnn.", mag, fl)
    logits = torch.stack([torch.nn.functional.linear(h, sd["linear.%d.weight" % s], sd["linear.%d.bias" % s])
                          for s in range(num_spk)])
    return logits, spec[:, :h.shape[1]], fl


def enh_loss(loss_type, mask_type, act, logits, mix, mix_label, refs_spec, refs_wav, ilens, stft_conf, training=True):
    """ESPnetEnhancementModel.forward on a TF-masking model's logits -> dict(loss, perm, si_snr (eval or si_snr loss)).
    mix: the model's own mixture spectrum, padded frames zeroed; mix_label: the one the labels are formed from, which the
    reference transforms without lengths (espnet_model.py:174), like the references"""
    n_fft, hop = stft_conf
    masks, P = mask_apply(logits, mix, act)
    out = {}
    if loss_type == "si_snr":
        wavs = [istft(p, n_fft, hop, length=max(ilens)) for p in P]
        loss, perm = permutation_loss(refs_wav, wavs, si_snr_loss_zeromean)
        return dict(loss=loss.mean(), perm=perm, si_snr=-loss.mean().detach())
    if loss_type == "mask_mse":
        loss, perm = permutation_loss(mask_label(mix_label, refs_spec, mask_type), list(masks), tf_mse_loss)
    elif loss_type == "magnitude":
        loss, perm = permutation_loss(list(refs_spec), list(P), mag_mse_loss)
    else:
        loss, perm = permutation_loss(list(refs_spec), list(P), tf_mse_loss)
    out.update(loss=loss.mean(), perm=perm)
    if not training:
        wavs = [istft(p, n_fft, hop, length=max(ilens)) for p in P]
        out["si_snr"] = -permutation_loss(refs_wav, wavs, si_snr_loss, perm=perm)[0].mean().detach()
    return out


def tf_masking_model(sd, wav, ilens, refs_wav, conf, training=True):
    """ESPnetEnhancementModel(TFMaskingNet(**conf)) on one batch; conf: n_fft, hop_length, num_spk, nonlinear, utt_mvn,
    mask_type, loss_type"""
    n_fft, hop, S = conf["n_fft"], conf["hop_length"], conf["num_spk"]
    logits, mix, fl = tf_masking_logits(sd, wav, ilens, n_fft, hop, S, conf.get("utt_mvn", False))
    refs_spec = [stft(r, n_fft, hop) for r in refs_wav]                          # transformed without lengths
    return enh_loss(conf["loss_type"], conf.get("mask_type", "IRM"), conf.get("nonlinear", "sigmoid"), logits, mix,
                    stft(wav, n_fft, hop), refs_spec, refs_wav, ilens, (n_fft, hop), training)


def beamformer_model(sd, wav, ilens, ref_wav, noise_wav, conf, training=True):
    """ESPnetEnhancementModel(BeamformerNet(**conf)) with one speaker, a noise mask and the "mvdr" type; wav, ref_wav,
    noise_wav [B, L, C]; sd: the state_dict of BeamformerNet.beamformer.  mask_mse: the speech-mask term and the
    noise-mask term, each a mean over the padded (B, T, C, F) extent"""
    n_fft, hop = conf["n_fft"], conf["hop_length"]
    B, L, C = wav.shape
    spec = lambda x: stft(x.transpose(1, 2).reshape(B * C, L), n_fft, hop).view(B, C, -1, n_fft // 2 + 1).transpose(1, 2)  # noqa: E731
    fl = frame_lens(ilens, n_fft, hop)
    keep = (torch.arange(frame_lens([L], n_fft, hop)[0])[None, :] < torch.as_tensor(fl)[:, None]).to(wav.dtype)
    mix_label = spec(wav)                                                        # espnet_model.py:174: no lengths
    mix = mix_label * keep[:, :, None, None]                                     # Stft.forward zeroes padded frames
    out = R.dnn_beamformer(sd, mix, fl, conf.get("ref_channel", -1))
    T = mix.shape[1]
    masks = [R.masks_full(out["logits"][s], T) for s in range(2)]               # (B, T, C, F), zero past max(fl)
    res = dict(enhanced=out["enhanced"], masks=masks)
    if conf["loss_type"] == "mask_mse":
        lab_s = mask_label(mix_label, [spec(ref_wav)], conf["mask_type"])
        lab_n = mask_label(mix_label, [spec(noise_wav)], conf["mask_type"])
        res["loss"] = tf_mse_loss(lab_s[0], masks[0]).mean() + tf_mse_loss(lab_n[0], masks[1]).mean()
    return res
