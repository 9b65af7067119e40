"""Speech enhancement / separation training: the reference's espnet2/enh task on the kernels of csrc/enh.hip.

reference: espnet2/enh/espnet_model.py (ESPnetEnhancementModel), espnet2/enh/nets/tf_mask_net.py (TFMaskingNet),
espnet2/enh/nets/beamformer_net.py (BeamformerNet): the same class names, constructor arguments, defaults, parameter names
and return conventions.  Spectra are float32 with a trailing (re, im) axis, as everywhere here.

MI355X mapping.  The mask heads' logits go straight to the kernels: eamd_enh_mask_apply forms the masks and the masked
spectra of all speakers in one pass over the mixture; eamd_enh_pair_tf forms the ideal-mask labels on the fly and all S x S
pair losses in one read of every operand; eamd_enh_pair_sisnr gathers the sums of both SI-SNR criteria in one pass;
eamd_enh_pit_pick picks the permutation on the device, so nothing of a training forward visits the host.  The reference
loops over permutations(range(num_spk)) in Python and makes several passes per criterion call.

Reference behaviours reproduced (each marked where it happens): the means run over the whole padded extent; "NPSM" is
clamped to [-1, 1] like "PSM"; 10e-12 and 10e-8 are the literal epsilons; the labels are formed from spectra transformed
without lengths.  Departures: `magnitude` takes the gradient of |P| at P = 0 as 0 where the reference gets
NaN; an unsupported mask_type is refused at construction; Stft.inverse documents the reference's window-less inverse.
"""
from collections import OrderedDict
from itertools import permutations

import torch

from .. import functional as F_
from .. import ops
from ..nets.frontends.dnn_beamformer import DNN_Beamformer
from ..nets.rnn.encoders import RNN
from .frontend import Stft
from .layers import UtteranceMVN

MASK_TYPES = tuple(ops.ENH_LABELS)
LOSS_TYPES = ("mask_mse", "magnitude", "spectrum", "si_snr")


class MaskDict(OrderedDict):
    """the predicted masks by name ("spk1", ..., "noise1"), activated, as the reference returns them; `logits`
    [n, B, ...] are the values in front of the activation `act`, in the order of the names: ESPnetEnhancementModel hands
    them to the loss kernel, which applies the activation itself"""
    logits = None
    act = "none"


def _stacked(ts):
    """list of S tensors [B, ...] -> [S, B, ...] contiguous; no copy when they are the slices of one such tensor"""
    ts = list(ts)
    base = ts[0]._base
    if (base is not None and base.is_contiguous() and base.shape[0] == len(ts) and tuple(base.shape[1:]) == tuple(ts[0].shape)
            and all(t._base is base and t.is_contiguous() and t.storage_offset() == base.storage_offset() + i * t.numel()
                    for i, t in enumerate(ts))):
        return base
    return torch.stack([t.float() for t in ts]).contiguous()


def _lengths(ilens, B, L):
    if ilens is None:
        return [L] * B
    return [int(v) for v in ilens]


class TFMaskingNet(torch.nn.Module):
    """TF Masking Speech Separation Net (tf_mask_net.py:12-157): Stft -> |X| [-> UtteranceMVN] -> BLSTM -> num_spk Linear
    heads -> masks; single-channel input (B, samples)."""

    def __init__(self, n_fft: int = 512, win_length: int = None, hop_length: int = 128, rnn_type: str = "blstm", layer: int = 3,
                 unit: int = 512, dropout: float = 0.0, num_spk: int = 2, nonlinear: str = "sigmoid", utt_mvn: bool = False,
                 mask_type: str = "IRM", loss_type: str = "mask_mse"):
        super().__init__()
        self.num_spk = num_spk
        self.num_bin = n_fft // 2 + 1
        self.mask_type = mask_type
        self.loss_type = loss_type
        if loss_type not in ("mask_mse", "magnitude", "spectrum"):
            raise ValueError("Unsupported loss type: %s" % loss_type)
        self.stft = Stft(n_fft=n_fft, win_length=win_length, hop_length=hop_length)
        self.utt_mvn = UtteranceMVN(norm_means=True, norm_vars=True) if utt_mvn else None
        self.rnn = RNN(idim=self.num_bin, elayers=layer, cdim=unit, hdim=unit, dropout=dropout, typ=rnn_type)
        self.linear = torch.nn.ModuleList([torch.nn.Linear(unit, self.num_bin) for _ in range(self.num_spk)])
        if nonlinear not in ("sigmoid", "relu", "tanh"):
            raise ValueError("Not supporting nonlinear={}".format(nonlinear))
        self.nonlinear = nonlinear

    def mask_logits(self, input, ilens):
        """-> (logits [S, B, T, F] of the heads, the mixture spectrum (B, T, F, 2) with padded frames zeroed, flens)"""
        ilens = torch.as_tensor(_lengths(ilens, input.size(0), input.size(1)))
        spec, flens = self.stft(input, ilens)
        with torch.no_grad():                                   # the mixture is data
            mag = torch.linalg.vector_norm(spec, dim=-1)
            if self.utt_mvn is not None:
                # departure: the reference's utterance_mvn works in place (tf_mask_net.py:99), so with utt_mvn its masks are
                # later applied to |X| - mean instead of |X|, an accident of aliasing.  Here only the network's input is
                # normalised and the masks apply to |X| (EnhMaskFn below); mask* losses, which form no spectrum, are equal.
                mag, _ = self.utt_mvn(mag, flens)
        x, _, _ = self.rnn(mag, flens)
        Tm = x.shape[1]
        logits = torch.stack([F_.LinearFn.apply(x, lin.weight, lin.bias) for lin in self.linear])
        return logits, spec[:, :Tm].contiguous(), flens

    def forward(self, input: torch.Tensor, ilens: torch.Tensor):
        """input (B, samples) -> (separated: list of num_spk (B, T, F, 2) or None, flens, masks: MaskDict 'spk1'..).
        In training with a mask* loss no spectrum is formed, as in the reference (tf_mask_net.py:111-112)."""
        logits, spec, flens = self.mask_logits(input, ilens)
        want_spec = not (self.training and self.loss_type.startswith("mask"))
        m, P = ops.EnhMaskFn.apply(logits, spec if want_spec else None, ops.ENH_ACTS[self.nonlinear], want_spec)
        masks = MaskDict(zip(["spk{}".format(i + 1) for i in range(self.num_spk)], m.unbind(0)))
        masks.logits, masks.act = logits, self.nonlinear
        return (list(P.unbind(0)) if want_spec else None), flens, masks

    def forward_rawwav(self, input: torch.Tensor, ilens: torch.Tensor):
        """-> (list of num_spk waveforms (B, samples) or None, ilens, masks); one inverse STFT for all speakers"""
        predicted_spectrums, flens, masks = self.forward(input, ilens)
        if predicted_spectrums is None:
            return None, ilens, masks
        P = _stacked(predicted_spectrums)
        S, B = P.shape[:2]
        wavs, _ = self.stft.inverse(P.view((S * B,) + tuple(P.shape[2:])), _lengths(ilens, B, input.size(1)))
        return list(wavs.view(S, B, -1).unbind(0)), ilens, masks


class BeamformerNet(torch.nn.Module):
    """TF Masking based beamformer (beamformer_net.py:13-254) over nets.frontends.DNN_Beamformer, every beamformer_type it
    has.  This project's scope: num_spk = 1, use_noise_mask = True, bnonlinear = "sigmoid", use_wpe = False,
    normalize_input = False; anything else raises NotImplementedError naming what is missing."""

    def __init__(self, num_spk: int = 1, normalize_input: bool = False, mask_type: str = "IPM^2", loss_type: str = "mask_mse",
                 n_fft: int = 512, win_length: int = None, hop_length: int = 128, center: bool = True, window="hann",
                 normalized: bool = False, onesided: bool = True, use_wpe: bool = False, wnet_type: str = "blstmp", wlayers: int = 3,
                 wunits: int = 300, wprojs: int = 320, wdropout_rate: float = 0.0, taps: int = 5, delay: int = 3,
                 use_dnn_mask_for_wpe: bool = True, wnonlinear: str = "crelu", use_beamformer: bool = True,
                 bnet_type: str = "blstmp", blayers: int = 3, bunits: int = 300, bprojs: int = 320, badim: int = 320,
                 ref_channel: int = -1, use_noise_mask: bool = True, bnonlinear: str = "sigmoid", beamformer_type="mvdr",
                 bdropout_rate=0.0):
        super().__init__()
        self.mask_type = mask_type
        self.loss_type = loss_type
        if loss_type not in ("mask_mse", "spectrum"):
            raise ValueError("Unsupported loss type: %s" % loss_type)
        if use_wpe:
            raise NotImplementedError("use_wpe=True: the espnet2 DNN_WPE variant (wnonlinear=%r, use_dnn_mask_for_wpe) is not "
                                      "implemented; only the beamformer runs here" % wnonlinear)
        if normalize_input:
            raise NotImplementedError("normalize_input=True (division by the batch's largest magnitude) is not implemented")
        if num_spk != 1:
            raise NotImplementedError("num_spk=%d: the multi-speaker DNN_Beamformer (bnmask > 2) is not implemented" % num_spk)
        if use_beamformer and not use_noise_mask:
            raise NotImplementedError("use_noise_mask=False (bnmask != 2: the noise mask as 1 - speech mask) is not implemented")
        if use_beamformer and bnonlinear != "sigmoid":
            raise NotImplementedError("bnonlinear=%r: the beamformer's PSD kernel applies a sigmoid to the mask logits" % bnonlinear)
        self.num_spk = num_spk
        self.num_bin = n_fft // 2 + 1
        self.stft = Stft(n_fft=n_fft, win_length=win_length, hop_length=hop_length, center=center, window=window,
                         normalized=normalized, onesided=onesided)
        self.normalize_input = normalize_input
        self.use_beamformer = use_beamformer
        self.use_wpe = use_wpe
        self.wpe = None
        self.ref_channel = ref_channel
        if self.use_beamformer:
            self.beamformer = DNN_Beamformer(btype=bnet_type, bidim=self.num_bin, bunits=bunits, bprojs=bprojs, blayers=blayers,
                                             bnmask=num_spk + 1, dropout_rate=bdropout_rate, badim=badim, ref_channel=ref_channel,
                                             beamformer_type=beamformer_type, btaps=taps, bdelay=delay)
        else:
            self.beamformer = None

    def _masks(self, logits, T):
        """logits [2, B, Tm, C, F] -> MaskDict of (B, T, C, F) masks, zero for Tm <= t < T (mask_estimator.py)"""
        m, _ = ops.EnhMaskFn.apply(logits, None, ops.ENH_ACTS["sigmoid"], False)
        masks = MaskDict()
        if m.shape[2] < T:
            m = torch.nn.functional.pad(m, [0, 0, 0, 0, 0, T - m.shape[2]], value=0)
        else:
            masks.logits, masks.act = logits, "sigmoid"
        for spk in range(self.num_spk):
            masks["spk{}".format(spk + 1)] = m[spk]
        masks["noise1"] = m[self.num_spk]
        return masks

    def forward(self, input: torch.Tensor, ilens: torch.Tensor):
        """input (B, samples, channels) or (B, samples) -> (enhanced (B, T, F, 2) or None, flens, masks: MaskDict with
        'spk1' and 'noise1' of (B, T, C, F)).  In training with a mask* loss only the masks are estimated
        (beamformer_net.py:155-179).  A single-channel input passes through (:183-191)."""
        ilens = torch.as_tensor(_lengths(ilens, input.size(0), input.size(1)))
        input_spectrum, flens = self.stft(input, ilens)
        assert input_spectrum.dim() in (4, 5), input_spectrum.dim()
        multi = input_spectrum.dim() == 5
        masks = MaskDict()
        if self.training and self.loss_type.startswith("mask"):
            if self.use_beamformer and multi:
                masks = self._masks(self.beamformer.predict_mask_logits(input_spectrum, flens), input_spectrum.shape[1])
            return None, flens, masks
        enhanced = input_spectrum
        if multi and self.use_beamformer:
            enhanced, _, _, parts = self.beamformer(input_spectrum, flens, return_all=True)
            with torch.no_grad():
                masks = self._masks(parts["logits"].permute(0, 1, 3, 2, 4).contiguous(), input_spectrum.shape[1])
        return enhanced, flens, masks

    def forward_rawwav(self, input: torch.Tensor, ilens: torch.Tensor):
        """-> (waveform (B, samples) or None, ilens, masks)"""
        predicted_spectrums, flens, masks = self.forward(input, ilens)
        if predicted_spectrums is None:
            return None, ilens, masks
        if predicted_spectrums.dim() == 5:                     # no beamformer: the channels pass through; the reference fails here
            raise NotImplementedError("forward_rawwav of a multi-channel spectrum needs use_beamformer=True")
        wavs, _ = self.stft.inverse(predicted_spectrums, _lengths(ilens, input.size(0), input.size(1)))
        return wavs, ilens, masks


def _is_spectrum(t):
    """a trailing axis of 2 on a 4-D or 5-D tensor is (re, im): (B, T, F, 2) or (B, T, C, F, 2); (B, T, F) and (B, T, C, F)
    are real.  A real (B, T, C, F) operand with exactly F = 2 bins cannot be told from a spectrum and is read as one."""
    return t.dim() in (4, 5) and t.shape[-1] == 2


class ESPnetEnhancementModel(torch.nn.Module):
    """Speech enhancement or separation Frontend model (espnet_model.py:16-443)."""

    def __init__(self, enh_model):
        super().__init__()
        self.enh_model = enh_model
        self.num_spk = enh_model.num_spk
        self.num_noise_type = getattr(self.enh_model, "num_noise_type", 1)
        self.mask_type = getattr(self.enh_model, "mask_type", None)
        self.loss_type = getattr(self.enh_model, "loss_type", None)
        assert self.loss_type in LOSS_TYPES, self.loss_type
        if self.loss_type.startswith("mask") and self.mask_type not in MASK_TYPES:
            # the reference only trips over this at the first batch (BeamformerNet's own default "IPM^2" included)
            raise ValueError("mask type {} not supported: one of {}".format(self.mask_type, ", ".join(MASK_TYPES)))
        ops.enh_check_spk(self.num_spk)
        self.ref_channel = getattr(self.enh_model, "ref_channel", -1)

    # ---- criteria (lists of tensors, as in the reference) ------------------------------------------------------------
    @staticmethod
    def tf_mse_loss(ref, inf):
        """time-frequency MSE loss: ref, inf (B, T, F) / (B, T, C, F) real, or spectra with a trailing (re, im) axis -> (B).
        The mean runs over the whole padded extent, padded frames included, as in the reference.  Restriction: a 4-D or
        5-D operand whose last axis has length 2 is read as a spectrum, so a real (B, T, C, F) operand needs F != 2."""
        assert ref.dim() == inf.dim(), (ref.shape, inf.shape)
        if ref.dim() not in (3, 4, 5):
            raise ValueError("Invalid input shape: ref={}, inf={}".format(ref.shape, inf.shape))
        mode = ops.ENH_SPEC if _is_spectrum(ref) else ops.ENH_REAL
        return ops.EnhTFLossFn.apply(inf.float().unsqueeze(0), ref.float().unsqueeze(0).contiguous(), None, mode, 0, 3, None)[0]

    @staticmethod
    def tf_l1_loss(ref, inf):
        """time-frequency L1 loss -> (B); no kernel has an L1 mode: evaluated in torch.  As for tf_mse_loss, a 4-D or 5-D
        operand whose last axis has length 2 is read as a spectrum."""
        assert ref.dim() == inf.dim(), (ref.shape, inf.shape)
        d = ref - inf
        d = torch.linalg.vector_norm(d, dim=-1) if _is_spectrum(ref) else d.abs()
        return d.flatten(1).mean(dim=1)

    @staticmethod
    def si_snr_loss(ref, inf):
        """si-snr loss (espnet_model.py:348-364): ref, inf (B, samples) -> (B)"""
        return ops.EnhSisnrLossFn.apply(inf.float().unsqueeze(0), ref.float().unsqueeze(0).contiguous(), ops.ENH_SNR_L2NORM, None)[0]

    @staticmethod
    def si_snr_loss_zeromean(ref, inf):
        """si_snr loss with zero-mean in pre-processing (espnet_model.py:367-405); the sums run over the full padded length"""
        assert ref.size() == inf.size()
        return ops.EnhSisnrLossFn.apply(inf.float().unsqueeze(0), ref.float().unsqueeze(0).contiguous(), ops.ENH_SNR_ZEROMEAN,
                                        None)[0]

    @staticmethod
    def _permutation_loss(ref, inf, criterion, perm=None):
        """ref, inf: lists of num_spk tensors (B, ...) -> (loss averaged over the batch, perm (B) int64: the index into
        itertools.permutations(range(num_spk)), first minimum).  The four criteria above run as one pair kernel and one
        pick kernel; any other callable is evaluated in torch over the permutations, as the reference does.  With
        tf_mse_loss, 4-D or 5-D operands whose last axis has length 2 are read as spectra (real operands need F != 2)."""
        E = ESPnetEnhancementModel
        if perm is not None:
            perm = perm.to(torch.int64).contiguous()
        if criterion is E.tf_mse_loss:
            mode = ops.ENH_SPEC if _is_spectrum(ref[0]) else ops.ENH_REAL
            loss, perm = ops.EnhTFLossFn.apply(_stacked(inf), _stacked(ref), None, mode, 0, 3, perm)
        elif criterion is E.si_snr_loss or criterion is E.si_snr_loss_zeromean:
            mode = ops.ENH_SNR_L2NORM if criterion is E.si_snr_loss else ops.ENH_SNR_ZEROMEAN
            loss, perm = ops.EnhSisnrLossFn.apply(_stacked(inf), _stacked(ref), mode, perm)
        else:
            num_spk = len(ref)
            losses = torch.stack([sum(criterion(ref[s], inf[t]) for s, t in enumerate(p)) / len(p)
                                  for p in permutations(range(num_spk))], dim=1)
            if perm is None:
                loss, perm = torch.min(losses, dim=1)
            else:
                loss = losses[torch.arange(losses.shape[0]), perm]
        return loss.mean(), perm

    def _mask_loss(self, mask_pre, names, spectrum_mix, spectrum_ref):
        """the permutation loss between the ideal-mask labels of spectrum_ref [n, B, ..., 2] and the predicted masks
        `names`; the labels are never stored"""
        first = list(mask_pre).index(names[0])
        logits = getattr(mask_pre, "logits", None)
        if logits is not None:
            est, act = logits[first:first + len(names)], mask_pre.act
        else:
            est, act = _stacked([mask_pre[k] for k in names]), "none"
        loss, perm = ops.EnhTFLossFn.apply(est, spectrum_ref, spectrum_mix, ops.ENH_MASK, ops.ENH_LABELS[self.mask_type],
                                           ops.ENH_ACTS[act], None)
        return loss.mean(), perm

    def _spectra(self, wavs):
        """[n, B, samples(, C)] -> [n, B, T, (C,) F, 2]: one STFT for all of them, without lengths (espnet_model.py:168)"""
        n, B = wavs.shape[:2]
        spec, _ = self.enh_model.stft(wavs.reshape((n * B,) + tuple(wavs.shape[2:])))
        return spec.view((n, B) + tuple(spec.shape[1:]))

    def forward(self, speech_mix: torch.Tensor, speech_mix_lengths: torch.Tensor = None, **kwargs):
        """speech_mix (B, samples) or (B, samples, channels); speech_ref1.. (and noise_ref1) alike
        -> (loss, stats{si_snr, loss}, weight)"""
        speech_ref = torch.stack([kwargs["speech_ref{}".format(spk + 1)] for spk in range(self.num_spk)], dim=0)   # [S, B, ...]
        noise_ref = None
        if "noise_ref1" in kwargs:
            noise_ref = torch.stack([kwargs["noise_ref{}".format(n + 1)] for n in range(self.num_noise_type)], dim=0)
        if kwargs.get("dereverb_ref", None) is not None:
            raise NotImplementedError("dereverb_ref: the WPE branch of BeamformerNet (use_wpe=True) is not implemented")
        batch_size = speech_mix.shape[0]
        lengths = _lengths(speech_mix_lengths, batch_size, speech_mix.shape[1])
        assert len(lengths) == batch_size == speech_ref.shape[1], (speech_mix.shape, speech_ref.shape, len(lengths))
        Lmax = max(lengths)
        speech_ref = speech_ref[:, :, :Lmax].float()                    # for data-parallel
        speech_mix = speech_mix[:, :Lmax]

        if self.loss_type != "si_snr":
            spectrum_ref = self._spectra(speech_ref)
            spectrum_pre, tf_length, mask_pre = self.enh_model(speech_mix, lengths)
            if self.loss_type in ("magnitude", "spectrum"):
                if spectrum_pre is None:
                    raise ValueError("the model returned no spectrum for loss type %s" % self.loss_type)
                if torch.is_tensor(spectrum_pre):
                    # BeamformerNet returns one single-channel tensor against multi-channel references: the reference
                    # iterates over its batch axis and fails on the shapes
                    raise NotImplementedError("loss_type=%r needs a model that returns one spectrum per speaker in the "
                                              "references' layout" % self.loss_type)
                # magnitude: |P| is differentiated as 0 at P = 0 (every padded frame); the reference gets inf * 0 = NaN
                mode = ops.ENH_MAG if self.loss_type == "magnitude" else ops.ENH_SPEC
                loss, perm = ops.EnhTFLossFn.apply(_stacked(spectrum_pre), spectrum_ref, None, mode, 0, 3, None)
                tf_loss = loss.mean()
            else:
                assert mask_pre is not None
                spectrum_mix, _ = self.enh_model.stft(speech_mix.float())          # without lengths, as the reference
                tf_loss, perm = self._mask_loss(mask_pre, ["spk{}".format(s + 1) for s in range(self.num_spk)], spectrum_mix,
                                                spectrum_ref)
                if "noise1" in mask_pre:
                    if noise_ref is None:
                        raise ValueError("No noise reference for training!\n"
                                         'Please specify "--use_noise_ref true" in run.sh')
                    noise_spectrum_ref = self._spectra(noise_ref[:, :, :Lmax].float())
                    tf_noise_loss, _ = self._mask_loss(mask_pre, ["noise{}".format(n + 1) for n in range(self.num_noise_type)],
                                                       spectrum_mix, noise_spectrum_ref)
                    tf_loss = tf_loss + tf_noise_loss
            if self.training or spectrum_pre is None:
                si_snr = None
            else:
                with torch.no_grad():
                    pre = [spectrum_pre] if torch.is_tensor(spectrum_pre) else spectrum_pre
                    P = _stacked(pre)
                    S = P.shape[0]
                    wavs, _ = self.enh_model.stft.inverse(P.view((S * batch_size,) + tuple(P.shape[2:])), lengths)
                    ref = speech_ref[..., self.ref_channel] if speech_ref.dim() == 4 else speech_ref
                    # the statistic re-uses the TF loss's permutation (espnet_model.py:276-279)
                    si_snr_loss, _ = ops.EnhSisnrLossFn.apply(wavs.view(S, batch_size, -1), ref.contiguous(), ops.ENH_SNR_L2NORM, perm)
                    si_snr = -si_snr_loss.mean()
            loss = tf_loss
            stats = dict(si_snr=si_snr, loss=loss.detach())
        else:
            if speech_ref.dim() == 4:
                speech_ref = speech_ref[..., self.ref_channel]
            speech_pre, _, *__ = self.enh_model.forward_rawwav(speech_mix, lengths)
            if torch.is_tensor(speech_pre):
                speech_pre = [speech_pre]
            assert speech_pre[0].dim() == 2, speech_pre[0].dim()
            si_snr_loss, perm = ops.EnhSisnrLossFn.apply(_stacked(speech_pre), speech_ref.contiguous(), ops.ENH_SNR_ZEROMEAN, None)
            loss = si_snr_loss.mean()
            stats = dict(si_snr=-loss.detach(), loss=loss.detach())
        self.last_perm = perm
        weight = torch.as_tensor(batch_size, device=loss.device)
        return loss, stats, weight

    def collect_feats(self, speech_mix: torch.Tensor, speech_mix_lengths: torch.Tensor, **kwargs):
        speech_mix = speech_mix[:, :int(max(int(v) for v in speech_mix_lengths))]
        return {"feats": speech_mix, "feats_lengths": speech_mix_lengths}
