"""Feature transform between the speech-enhancement front-end and the RNN encoder: power -> mel -> log -> global MVN ->
utterance MVN.  reference: espnet/nets/pytorch_backend/frontends/feature_transform.py (same class and function names,
constructor arguments and buffer names; `forward(x, ilens) -> (h, ilens)`).

A complex spectrum is a float32 tensor with a trailing (re, im) axis - [B, T, F, 2], the beamformer's output, or
[B, T, C, F, 2] when the beamformer was not applied - where the reference carries torch_complex.ComplexTensor.  Both
directions run on the kernels of csrc/feature_transform.hip, so the ASR loss reaches the spectrum and through it the
beamformer's mask estimator.

The reference's quirks are kept: both `masked_fill` calls of GlobalMVN / utterance_mvn are not in place and do nothing,
so GlobalMVN turns the (zeroed) padded log-mel frames into bias * scale, the utterance mean sums ALL T frames and divides
by the length, and padded frames leave the layer non-zero; utterance_mvn(norm_means=False, norm_vars=False) still
returns the mean-subtracted copy.  With norm_vars=True the reference's own backward fails (it divides in place a tensor
that pow's backward needs), so that combination is refused for features that require a gradient.

librosa is absent from this image: the mel matrix is espnet2.frontend.mel_filterbank, the restatement of
librosa.filters.mel (Slaney area normalisation, which the reference's `norm=1` selects).
"""
import numpy as np
import torch

from ... import ops
from ... import rnn_functional as R_


def _lens_dev(ilens, device):
    return ops.h2d_cached("ft_lens", np.asarray([int(v) for v in ilens], dtype=np.int32), device)


def _as_real(x):
    return torch.view_as_real(x) if x.is_complex() else x


def _ranges(nz):
    """nz [R, K] bool -> (first, one past last) True column of each row, (0, 0) for an empty row; int32"""
    any_ = nz.any(1)
    lo = np.where(any_, nz.argmax(1), 0)
    hi = np.where(any_, nz.shape[1] - nz[:, ::-1].argmax(1), 0)
    return torch.from_numpy(lo.astype(np.int32)), torch.from_numpy(hi.astype(np.int32))


def _refuse_norm_vars_grad(x, norm_vars):
    if norm_vars and x.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(
            "uttmvn_norm_vars=True cannot be trained through: the reference's own backward fails there (utterance_mvn "
            "divides x in place by sqrt(var) after x.pow(2) saved it for its backward), so there is no gradient to "
            "reproduce; use norm_vars=False for a jointly trained front-end")


class FeatureTransform(torch.nn.Module):
    def __init__(self, fs: int = 16000, n_fft: int = 512, n_mels: int = 80, fmin: float = 0.0, fmax: float = None,
                 stats_file: str = None, apply_uttmvn: bool = True, uttmvn_norm_means: bool = True,
                 uttmvn_norm_vars: bool = False):
        super().__init__()
        self.apply_uttmvn = apply_uttmvn
        self.logmel = LogMel(fs=fs, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax)
        self.stats_file = stats_file
        self.global_mvn = GlobalMVN(stats_file) if stats_file is not None else None
        if self.apply_uttmvn is not None:           # (sic) feature_transform.py:38
            self.uttmvn = UtteranceMVN(norm_means=uttmvn_norm_means, norm_vars=uttmvn_norm_vars)
        else:
            self.uttmvn = None

    def forward(self, x, ilens):
        """x [B,T,F,2] or [B,T,C,F,2] -> (h [B,T,n_mels], ilens)"""
        x = _as_real(x)
        if x.dim() not in (4, 5):
            raise ValueError(f"Input dim must be 4 or 5 with the trailing (re, im) axis: {x.dim()}")
        if not torch.is_tensor(ilens):
            ilens = torch.from_numpy(np.asarray(ilens))
        if x.dim() == 5:
            # feature_transform.py:54-62: one channel, drawn in training, the first otherwise
            ch = np.random.randint(x.size(2)) if self.training else 0
            h = x[:, :, ch]
        else:
            h = x
        apply_utt = bool(self.apply_uttmvn)
        if apply_utt:
            _refuse_norm_vars_grad(h, self.uttmvn.norm_vars)
        lens = _lens_dev(ilens, h.device)
        h = self.logmel.from_spectrum(h, lens)
        if self.global_mvn is not None or apply_utt:          # both normalisations in one pair of kernels
            bias, scale = self.global_mvn.bias_scale() if self.global_mvn is not None else (None, None)
            u = self.uttmvn
            h = R_.FtMvnFn.apply(h, lens, bias, scale, apply_utt, bool(u.norm_means) if apply_utt else False,
                                 bool(u.norm_vars) if apply_utt else False, u.eps if apply_utt else 0.0)
        return h, ilens


class LogMel(torch.nn.Module):
    """Convert STFT to fbank feats; the arguments are those of librosa.filters.mel"""

    def __init__(self, fs: int = 16000, n_fft: int = 512, n_mels: int = 80, fmin: float = 0.0, fmax: float = None,
                 htk: bool = False, norm=1):
        super().__init__()
        from ...espnet2.frontend import mel_filterbank
        if norm not in (1, "slaney"):
            raise NotImplementedError(f"LogMel(norm={norm!r}): only the Slaney area normalisation (norm=1) is implemented")
        self.mel_options = dict(sr=fs, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax, htk=htk, norm=norm)
        melmat = mel_filterbank(fs, n_fft, n_mels, fmin, fmax, htk)            # (n_mels, F)
        self.register_buffer("melmat", torch.from_numpy(np.ascontiguousarray(melmat.T)).float())
        self.set_ranges()

    def set_ranges(self):
        """the non-zero bin range of each filter and filter range of each bin, from the current `melmat` (call again after
        loading another matrix)"""
        nz = self.melmat.detach().cpu().numpy() != 0                           # [F, M]
        for name, t in zip(("_lo", "_hi", "_mlo", "_mhi"), _ranges(nz.T) + _ranges(nz)):
            self.register_buffer(name, t.to(self.melmat.device), persistent=False)

    def extra_repr(self):
        return ", ".join(f"{k}={v}" for k, v in self.mel_options.items())

    def from_spectrum(self, spec, lens_dev):
        return R_.FtLogMelFn.apply(spec, self.melmat, self._lo, self._hi, self._mlo, self._mhi, lens_dev)

    def forward(self, feat, ilens):
        """feat: the complex spectrum [B,T,F,2] (the kernel takes the power itself; the reference's LogMel receives
        re^2 + im^2) -> (log-mel [B,T,n_mels] with the padded frames zeroed, ilens)"""
        feat = _as_real(feat)
        if feat.dim() != 4 or feat.size(-1) != 2:
            raise ValueError("LogMel takes the complex spectrum [B, T, F, 2], not its power")
        return self.from_spectrum(feat, _lens_dev(ilens, feat.device)), ilens


class GlobalMVN(torch.nn.Module):
    """Apply global mean and variance normalization; stats_file: npy file of [sum (D), sum of squares (D), count]"""

    def __init__(self, stats_file: str, norm_means: bool = True, norm_vars: bool = True, eps: float = 1.0e-20):
        super().__init__()
        self.norm_means = norm_means
        self.norm_vars = norm_vars
        self.stats_file = stats_file
        stats = np.load(stats_file).astype(float)
        assert (len(stats) - 1) % 2 == 0, stats.shape
        count = stats.flatten()[-1]
        mean = stats[: (len(stats) - 1) // 2] / count
        var = stats[(len(stats) - 1) // 2: -1] / count - mean * mean
        std = np.maximum(np.sqrt(var), eps)
        self.register_buffer("bias", torch.from_numpy(-mean.astype(np.float32)))
        self.register_buffer("scale", torch.from_numpy(1 / std.astype(np.float32)))

    def extra_repr(self):
        return f"stats_file={self.stats_file}, norm_means={self.norm_means}, norm_vars={self.norm_vars}"

    def bias_scale(self):
        """(bias, scale) as the kernel takes them: x + 0 and x * 1 are exact for a half that is switched off"""
        if not (self.norm_means or self.norm_vars):
            return None, None
        return (self.bias if self.norm_means else torch.zeros_like(self.bias),
                self.scale if self.norm_vars else torch.ones_like(self.scale))

    def forward(self, x, ilens):
        """x [B,T,D] -> ((x + bias) * scale on every frame, padded ones included; ilens)"""
        bias, scale = self.bias_scale()
        if bias is None:
            return x, ilens
        return R_.FtMvnFn.apply(x, None, bias, scale, False, False, False, 0.0), ilens


class UtteranceMVN(torch.nn.Module):
    def __init__(self, norm_means: bool = True, norm_vars: bool = False, eps: float = 1.0e-20):
        super().__init__()
        self.norm_means = norm_means
        self.norm_vars = norm_vars
        self.eps = eps

    def extra_repr(self):
        return f"norm_means={self.norm_means}, norm_vars={self.norm_vars}"

    def forward(self, x, ilens):
        return utterance_mvn(x, ilens, norm_means=self.norm_means, norm_vars=self.norm_vars, eps=self.eps)


def utterance_mvn(x, ilens, norm_means: bool = True, norm_vars: bool = False, eps: float = 1.0e-20):
    """x [B,T,D], ilens [B] -> (feature_transform.py:213-247 to the letter, ilens)"""
    _refuse_norm_vars_grad(x, norm_vars)
    return R_.FtMvnFn.apply(x, _lens_dev(ilens, x.device), None, None, True, bool(norm_means), bool(norm_vars), eps), ilens


def feature_transform_for(args, n_fft):
    return FeatureTransform(fs=args.fbank_fs, n_fft=n_fft, n_mels=args.n_mels, fmin=args.fbank_fmin, fmax=args.fbank_fmax,
                            stats_file=args.stats_file, apply_uttmvn=args.apply_uttmvn,
                            uttmvn_norm_means=args.uttmvn_norm_means, uttmvn_norm_vars=args.uttmvn_norm_vars)
