"""Log-mel frontend on the device: waveform -> STFT -> power spectrum -> mel filterbank -> log.

reference: espnet2/asr/frontend/default.py:18-133 (DefaultFrontend), espnet2/layers/stft.py:16-111 (Stft over torch.stft),
espnet2/layers/log_mel.py:8-75 (LogMel over librosa.filters.mel).  Same class names, constructor arguments and
`forward(input, input_lengths) -> (feats, lens)`.

frontend_conf with use_beamformer builds the mask-based MVDR beamformer of nets/frontends (default.py:58-94): a
multi-channel waveform (B, L, C) then goes Stft.forward -> Frontend -> power spectrum -> LogMel.  use_wpe in frontend_conf
is refused; WPE dereverberation is attached afterwards (DefaultFrontend(...).frontend.attach_wpe(DNN_WPE(...))) and then
runs in front of the beamformer.  Without an enabled frontend_conf, and for single-channel input, the path below is unchanged.

MI355X mapping: the DFT of all frames is ONE fp32 MFMA GEMM - the reflect-padded waveform is read in place as
overlapping rows (leading dimension = hop length), the window is folded into the [2F, n_fft] basis - followed by one
kernel that squares, applies the (short, triangular) mel filters, clamps, takes the log and zeroes the padded frames.
bf16 is never used here: the power spectrum spans > 100 dB.

librosa is a third-party dependency of the reference that is absent from this image (pinned `librosa>=0.8.0` in the
reference's setup.py); `mel_filterbank` restates its published `filters.mel` algorithm (Slaney / HTK mel scales, Slaney
area normalisation) and is checked against the two values printed in that function's docstring (the CPU test suite).
"""
import math

import numpy as np
import torch

from .. import ops
from ..nets.frontends.frontend import Frontend
from ..nets.modules import make_pad_mask

try:  # pragma: no cover - only when the reference package is importable
    from espnet2.asr.frontend.abs_frontend import AbsFrontend  # type: ignore
except Exception:  # noqa: BLE001
    AbsFrontend = torch.nn.Module


def _hz_to_mel(f, htk):
    f = np.asarray(f, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, mels)


def _mel_to_hz(m, htk):
    m = np.asarray(m, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels=128, fmin=0.0, fmax=None, htk=False):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk, norm='slaney') -> float32 [n_mels, 1 + n_fft//2]"""
    fmax = sr / 2.0 if fmax is None else fmax
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin, htk), _hz_to_mel(fmax, htk), n_mels + 2), htk)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    weights = np.zeros((n_mels, 1 + n_fft // 2), dtype=np.float32)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, None].astype(np.float32)
    return weights


class Stft(torch.nn.Module):
    def __init__(self, n_fft=512, win_length=None, hop_length=128, window="hann", center=True, normalized=False,
                 onesided=True):
        super().__init__()
        self.n_fft = n_fft
        self.win_length = n_fft if win_length is None else win_length
        self.hop_length, self.center, self.normalized, self.onesided = hop_length, center, normalized, onesided
        if window is not None and not hasattr(torch, f"{window}_window"):
            raise ValueError(f"{window} window is not implemented")
        self.window = window
        self._basis = None
        self._inverse = {}

    def extra_repr(self):
        return (f"n_fft={self.n_fft}, win_length={self.win_length}, hop_length={self.hop_length}, "
                f"center={self.center}, normalized={self.normalized}, onesided={self.onesided}")

    @property
    def n_freq(self):
        return self.n_fft // 2 + 1 if self.onesided else self.n_fft

    def basis(self, device):
        """[2F, n_fft]: rows 2j / 2j+1 = w[k] cos(2 pi j k / N) / -w[k] sin(2 pi j k / N) (window centred in n_fft)"""
        if self._basis is None or self._basis.device != torch.device(device):
            N, F = self.n_fft, self.n_freq
            w = np.ones(self.win_length) if self.window is None else \
                getattr(torch, f"{self.window}_window")(self.win_length, dtype=torch.float64).numpy()
            left = (N - self.win_length) // 2
            wf = np.zeros(N)
            wf[left:left + self.win_length] = w
            if self.normalized:
                wf = wf * N ** -0.5
            ang = 2.0 * math.pi * ((np.arange(F)[:, None] * np.arange(N)[None, :]) % N) / N
            b = np.empty((2 * F, N))
            b[0::2] = np.cos(ang) * wf
            b[1::2] = -np.sin(ang) * wf
            self._basis = torch.from_numpy(b.astype(np.float32)).to(device)
        return self._basis

    def frames(self, nsamples):
        pad = self.n_fft // 2 if self.center else 0
        return (nsamples + 2 * pad - self.n_fft) // self.hop_length + 1

    def spectrum(self, x):
        """x [B, L] -> (spec flat [B*rows_per_utt, 2F] interleaved (re, im), rows_per_utt, T)"""
        B, L = x.shape
        pad = self.n_fft // 2 if self.center else 0
        T = self.frames(L)
        if T < 1:
            raise ValueError("input is shorter than one STFT frame")
        rpu = -(-(L + 2 * pad) // self.hop_length)
        xp = ops.reflect_pad(x.contiguous().float(), pad, rpu * self.hop_length, self.n_fft)
        F2 = 2 * self.n_freq
        spec = torch.empty(B * rpu, F2, device=x.device, dtype=torch.float32)
        ops.gemm(xp, self.basis(x.device), spec, B * rpu, F2, self.n_fft, self.hop_length, self.n_fft, F2, precision=0)
        return spec, rpu, T

    def olens(self, ilens):
        """stft.py:104-108 (the length formula uses win_length where the framing uses n_fft)"""
        if self.center:
            ilens = ilens + 2 * (self.win_length // 2)
        return (ilens - self.win_length) // self.hop_length + 1

    def forward(self, input, ilens=None):
        """input (B, Nsamples) or (B, Nsamples, C) -> (B, Frames, [C,] Freq, 2), olens; padded frames zeroed"""
        bs = input.size(0)
        multi = input.dim() == 3
        if multi:
            input = input.transpose(1, 2).reshape(-1, input.size(1))
        spec, rpu, T = self.spectrum(input)
        F = self.n_freq
        out = spec.view(input.size(0), rpu, F, 2)[:, :T].contiguous()
        if multi:
            out = out.view(bs, -1, T, F, 2).transpose(1, 2).contiguous()
        if ilens is None:
            return out, None
        olens = self.olens(torch.as_tensor(ilens))
        keep = (~make_pad_mask(olens.tolist(), T)).to(torch.uint8)              # [B, T]
        if multi:
            keep = keep.unsqueeze(-1).expand(bs, T, out.size(2))
        rows = out.view(-1, (out.numel() // keep.numel()))
        out = ops.mask_rows(rows, ops.h2d_cached("stft_keep", keep.contiguous().numpy().reshape(-1), out.device)).view(out.shape)
        return out, olens

    def inverse_basis(self, device, window=None):
        """-> (inv_basis [n_fft, 2F], bwd_basis [2F, n_fft], synthesis window [n_fft] on the device, the same on the host),
        both matrices in the [N, K] layout of eamd_gemm's right operand.

        inv_basis is the transpose of b [2F, n_fft], the inverse DFT of one frame on the interleaved (re, im) spectrum:
        rows 2j / 2j+1 of b = c_j/N cos(2 pi j k / N) / -c_j/N sin(2 pi j k / N) with c_0 = c_{N/2} = 1 and every other
        c_j = 2; the imaginary parts of DC and Nyquist drop out, as in a c2r transform.  A two-sided spectrum is rebuilt
        from its bins 0 .. N/2 in the same way (c_j = 0 above N/2): torch.istft, which the reference calls, slices the
        upper bins off.  Times N^0.5 with `normalized`.  bwd_basis is b with the synthesis window folded in, the right
        operand of the backward's GEMM.
        window: None = rectangular ones of win_length centred in n_fft (what `inverse` documents), the name of a torch
        window function, or win_length / n_fft values.  The few bases in use are kept, keyed by the device and the
        window's values (a window given as values on the device is copied back to form the key)."""
        N, F = self.n_fft, self.n_freq
        if window is None:
            w = np.ones(self.win_length)
        elif isinstance(window, str):
            w = getattr(torch, f"{window}_window")(self.win_length, dtype=torch.float64).numpy()
        else:
            w = torch.as_tensor(window).detach().double().cpu().numpy()
        key = (str(torch.device(device)), w.tobytes())
        if key not in self._inverse:
            if w.shape == (N,):
                wf = w.copy()
            else:
                if w.shape != (self.win_length,):
                    raise ValueError(f"the synthesis window needs win_length={self.win_length} or n_fft={N} values")
                left = (N - self.win_length) // 2
                wf = np.zeros(N)
                wf[left:left + self.win_length] = w
            j = np.arange(F)
            ang = 2.0 * math.pi * ((j[:, None] * np.arange(N)[None, :]) % N) / N
            c = np.where(j <= N // 2, 2.0, 0.0)              # bins above N/2 of a two-sided spectrum are not read
            c[0] = 1.0
            if N % 2 == 0:
                c[N // 2] = 1.0
            scale = c / N * (N ** 0.5 if self.normalized else 1.0)
            b = np.empty((2 * F, N))
            b[0::2] = np.cos(ang) * scale[:, None]
            b[1::2] = -np.sin(ang) * scale[:, None]
            b[1] = 0.0
            if N % 2 == 0:
                b[2 * (N // 2) + 1] = 0.0
            f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32)).to(device)  # noqa: E731
            if len(self._inverse) >= 8:
                self._inverse.clear()
            self._inverse[key] = (f32(b.T), f32(b * wf[None, :]), f32(wf), wf.astype(np.float32).astype(np.float64))
        return self._inverse[key]

    def inverse(self, input, ilens=None, window=None):
        """input (B, T, F, 2) -> (wavs (B, max(ilens)), ilens); stft.py:116-157 over ops.istft, differentiable in input.

        The reference hands torch.istft NO window, so its synthesis window is rectangular: ones of win_length, centred in
        n_fft, also when the analysis window is Hann.  window=None reproduces that literally: with hop = n_fft / 4 and a
        Hann analysis window the result is 0.5 x, not x (SI-SNR does not see the scale).  window="hann" (or any window
        values) gives the true inverse of `forward`."""
        assert input.dim() == 4 and input.shape[-1] == 2 and input.shape[2] == self.n_freq, tuple(input.shape)
        length = None if ilens is None else int(max(int(v) for v in ilens))
        inv_basis, bwd_basis, w, w_host = self.inverse_basis(input.device, window)
        wavs = ops.istft(input.contiguous().float(), inv_basis, bwd_basis, w, self.hop_length, self.center, length,
                         window_host=w_host)
        return wavs, ilens


class LogMel(torch.nn.Module):
    def __init__(self, fs=16000, n_fft=512, n_mels=80, fmin=None, fmax=None, htk=False, log_base=None):
        super().__init__()
        fmin = 0 if fmin is None else fmin
        fmax = fs / 2 if fmax is None else fmax
        self.mel_options = dict(sr=fs, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax, htk=htk)
        self.log_base = log_base
        melmat = mel_filterbank(**self.mel_options)                              # (n_mels, F)
        self.register_buffer("melmat", torch.from_numpy(np.ascontiguousarray(melmat.T)).float())
        nz = melmat > 0
        lo = np.where(nz.any(1), nz.argmax(1), 0)
        hi = np.where(nz.any(1), melmat.shape[1] - nz[:, ::-1].argmax(1), 0)
        self.register_buffer("_lo", torch.from_numpy(lo.astype(np.int32)), persistent=False)
        self.register_buffer("_hi", torch.from_numpy(hi.astype(np.int32)), persistent=False)

    def extra_repr(self):
        return ", ".join(f"{k}={v}" for k, v in self.mel_options.items())

    @property
    def log_scale(self):
        return 1.0 if self.log_base is None else 1.0 / math.log(self.log_base)

    def from_spectrum(self, spec, rpu, T, B, flens_dev):
        F = self.melmat.shape[0]
        return ops.logmel(spec, spec.shape[1], rpu, self.melmat, self._lo, self._hi, flens_dev, B, T, F, self.log_scale)

    def forward(self, feat, ilens=None):
        """feat (B, T, F) power spectrum -> (log-mel (B, T, n_mels), ilens)"""
        B, T, F = feat.shape
        fl = None
        if ilens is not None:
            fl = ops.h2d_cached("logmel_lens", np.asarray([int(v) for v in ilens], dtype=np.int32), feat.device)
        out = ops.logmel(feat.contiguous().float(), F, T, self.melmat, self._lo, self._hi, fl, B, T, F, self.log_scale,
                         power_input=True)
        if ilens is None:
            ilens = torch.full([B], T, dtype=torch.long)
        return out, ilens


class DefaultFrontend(AbsFrontend):
    """Stft -> [Frontend: MVDR beamformer] -> power spectrum -> LogMel.

    frontend_conf: the keyword arguments of nets.frontends.frontend.Frontend (use_beamformer, btype, blayers, bunits,
    bprojs, bnmask, badim, ref_channel, bdropout_rate, beamformer_type - "mvdr", "mpdr" or the convolutional "wpd" - btaps,
    bdelay); use_wpe=True raises NotImplementedError (attach a DNN_WPE with
    `self.frontend.attach_wpe`: eval then runs WPE and the beamformer, training draws one of them).  With use_beamformer a
    3-D input (B, L, C) is beamformed to one channel (in training mode Frontend draws, as the reference does, between
    beamforming and passing the channels through, of which one is then picked at random).  None or all switches off:
    `frontend` is None and a 3-D input is reduced to one channel before the STFT, as before.

    The features carry no gradient back to the front-end (log-mel, SpecAug, MVN and the subsampling convolution have no
    input gradient), so in training mode an enabled beamformer must be frozen (every parameter requires_grad=False);
    the beamformer by itself (nets.frontends) is differentiable for spectrum-level training."""

    def __init__(self, fs=16000, n_fft=512, win_length=None, hop_length=128, window="hann", center=True,
                 normalized=False, onesided=True, n_mels=80, fmin=None, fmax=None, htk=False, frontend_conf=None):
        super().__init__()
        if isinstance(fs, str):
            mult = {"k": 1000, "m": 1000000}.get(fs[-1].lower())
            fs = int(float(fs[:-1]) * mult) if mult else int(fs)
        self.stft = Stft(n_fft=n_fft, win_length=win_length, hop_length=hop_length, center=center, window=window,
                         normalized=normalized, onesided=onesided)
        if frontend_conf is not None and (frontend_conf.get("use_wpe") or frontend_conf.get("use_beamformer")):
            self.frontend = Frontend(idim=n_fft // 2 + 1, **frontend_conf)
        else:
            self.frontend = None
        self.logmel = LogMel(fs=fs, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax, htk=htk)
        self.n_mels = n_mels

    def output_size(self):
        return self.n_mels

    def _enhanced(self, input, input_lengths):
        """(B, L, C) waveform -> Stft.forward -> Frontend -> one channel -> power spectrum -> LogMel (default.py:76-116)"""
        if self.training and any(p.requires_grad for p in self.frontend.parameters()):
            raise NotImplementedError(
                "training the beamformer jointly from the ASR loss is not implemented: nothing downstream of the front-end "
                "(log-mel, SpecAug, MVN, the subsampling convolution) returns a gradient to the features.  Freeze the "
                "front-end (requires_grad_(False) on DefaultFrontend.frontend) or train it separately at spectrum level")
        spec, feats_lens = self.stft(input, torch.as_tensor(input_lengths).cpu())   # (B, T, C, F, 2), padded frames zero
        with torch.no_grad():
            h, _, _ = self.frontend(spec, feats_lens)
            if h.dim() == 5:                                                         # default.py:96-105
                ch = np.random.randint(h.size(2)) if self.training else 0
                h = h[:, :, ch]
            power = h[..., 0] ** 2 + h[..., 1] ** 2
        feats, _ = self.logmel(power, feats_lens)
        return feats, feats_lens

    def forward(self, input, input_lengths):
        if self.frontend is not None and input.dim() == 3:
            return self._enhanced(input, input_lengths)
        if input.dim() == 3:      # default.py:107-115: one channel, random in training, the first otherwise
            ch = np.random.randint(input.size(2)) if self.training else 0
            input = input[:, :, ch]
        spec, rpu, T = self.stft.spectrum(input)
        feats_lens = self.stft.olens(torch.as_tensor(input_lengths).cpu())
        fl = ops.h2d_cached("frontend_lens", feats_lens.numpy().astype(np.int32), input.device)
        feats = self.logmel.from_spectrum(spec, rpu, T, input.size(0), fl)
        return feats, feats_lens
