"""The espnet1 feature transform (espnet/nets/pytorch_backend/frontends/feature_transform.py) restated in plain torch, in
whatever dtype its inputs have: the float64 ground truth of the kernel tests and the CPU check of the fixture
tests/golden/frontend_e2e.npz.  Test infrastructure only; everything is differentiable by autograd.

A complex spectrum is a complex tensor [B, T, F] here (the fixture and the kernels carry a trailing (re, im) axis: cx / ri).
The reference's quirks are explicit below: its two `masked_fill` calls are not in place and change nothing."""
import numpy as np
import torch


def cx(a):
    t = torch.as_tensor(np.ascontiguousarray(a)) if not torch.is_tensor(a) else a.contiguous()
    return torch.view_as_complex(t)


def ri(t):
    return torch.view_as_real(t.resolve_conj()).contiguous()


def err_vs(a, ref):
    """max |a - ref| / max |ref| (the fixture's err32 measure)"""
    den = float(ref.abs().max())
    return float((a - ref).abs().max()) / den if den > 0 else float((a - ref).abs().max())


def pad_mask(ilens, T):
    return torch.arange(T)[None, :] >= torch.as_tensor([int(v) for v in ilens])[:, None]          # [B, T], True = padded


def mel_sum(x, melmat):
    """complex [B,T,F], melmat [F,M] -> sum_f |x|^2 melmat (feature_transform.py:67,127)"""
    return torch.matmul(x.real ** 2 + x.imag ** 2, melmat)


def logmel(x, melmat, ilens):
    """log(mel + 1e-20), padded frames zeroed (feature_transform.py:129-131)"""
    h = (mel_sum(x, melmat) + 1e-20).log()
    return h.masked_fill(pad_mask(ilens, h.shape[1])[:, :, None], 0.0)


def global_mvn(h, bias, scale):
    """x += bias; masked_fill without the underscore; x *= scale: the padded frames become bias * scale"""
    return (h + bias) * scale


def utterance_mvn(h, ilens, norm_means=True, norm_vars=False, eps=1e-20):
    """feature_transform.py:213-247: the mean sums ALL T frames and divides by the length; without norm_vars the
    mean-subtracted copy comes back whatever norm_means is; with norm_vars h (mean-subtracted only under norm_means) is
    divided by sqrt(clamp(sum_T (h - mean)^2 / len, eps))"""
    n = torch.as_tensor([float(v) for v in ilens], dtype=h.dtype)[:, None]
    mean = h.sum(dim=1) / n
    c = h - mean[:, None, :]
    if not norm_vars:
        return c
    var = torch.clamp((c ** 2).sum(dim=1) / n, min=eps)
    return (c if norm_means else h) / var.sqrt()[:, None, :]


def feature_transform(x, melmat, ilens, bias=None, scale=None, apply_uttmvn=True, norm_means=True, norm_vars=False):
    """x complex [B,T,F], or [B,T,C,F] of which channel 0 is taken (eval mode) -> [B,T,M] on all T frames"""
    if x.dim() == 4:
        x = x[:, :, 0]
    h = logmel(x, melmat, ilens)
    if bias is not None:
        h = global_mvn(h, bias, scale)
    if apply_uttmvn:
        h = utterance_mvn(h, ilens, norm_means, norm_vars)
    return h


def stats_bias_scale(stats, dtype=torch.float64, eps=1e-20):
    """GlobalMVN.__init__ (feature_transform.py:161-172): -> (bias, scale) rounded to float32 as the reference's buffers"""
    stats = np.asarray(stats, dtype=float)
    n = (len(stats) - 1) // 2
    count = stats[-1]
    mean = stats[:n] / count
    var = stats[n:-1] / count - mean * mean
    std = np.maximum(np.sqrt(var), eps)
    return (torch.from_numpy(-mean.astype(np.float32)).to(dtype), torch.from_numpy(1 / std.astype(np.float32)).to(dtype))


def conv3x3_c1_input_grad(dy, w):
    """dy [B,T,F,C], w [C,1,3,3] -> dx [B,T,F] = sum_c sum_ij dy[b,t+1-i,f+1-j,c] w[c,i,j]: the transposed convolution"""
    return torch.nn.functional.conv_transpose2d(dy.permute(0, 3, 1, 2), w, padding=1)[:, 0]
