"""DNN mask based MVDR beamformer (Ochiai et al. 2017, https://arxiv.org/abs/1703.04783).
reference: espnet/nets/pytorch_backend/frontends/dnn_beamformer.py (same class names, constructor arguments and
parameter names); the "mpdr" and "wpd" types, btaps, bdelay and eps are those of espnet2/enh/layers/dnn_beamformer.py.
Spectra are float32 [B, T, C, F, 2] (Stft.forward's layout), see beamformer.py and conv_beamformer.py."""
import torch

from ... import functional as F_
from ... import ops
from ... import rnn_functional as R_
from .beamformer import apply_beamforming_vector, get_mvdr_vector, get_power_spectral_density_matrix
from .conv_beamformer import get_covariances, get_covariances_from_power, get_WPD_filter_v2, perform_WPD_filtering
from .dnn_wpe import MaskedPowerFn
from .mask_estimator import MaskEstimator

BEAMFORMER_TYPES = ("mvdr", "mpdr", "wpd")


class DNN_Beamformer(torch.nn.Module):
    def __init__(self, bidim, btype="blstmp", blayers=3, bunits=300, bprojs=320, bnmask=2, dropout_rate=0.0, badim=320,
                 ref_channel: int = -1, beamformer_type="mvdr", btaps: int = 5, bdelay: int = 3, eps: float = 1e-6):
        """beamformer_type: "mvdr" (noise PSD from the noise mask), "mpdr" (the observation's own covariance
        sum_{t < n} y_t y_t^H in its place; the noise mask is not used) or "wpd" (the convolutional beamformer of
        conv_beamformer.py with btaps taps after a delay of bdelay frames, weights 1 / clamp(power, eps) with
        power = mean_c |y|^2 mask_speech; the noise mask is not used).  btaps = 0 forces bdelay = 1, as in the reference.
        The reference floors the masks at eps (active only for logits below -13.8); this class, like its MVDR path,
        does not."""
        super().__init__()
        if bnmask != 2:
            raise NotImplementedError("bnmask=%d: the multi-speaker beamformer (one MVDR filter per speaker mask) is not "
                                      "implemented, only (speech, noise) masks" % bnmask)
        self.mask = MaskEstimator(btype, bidim, blayers, bunits, bprojs, dropout_rate, nmask=bnmask)
        self.ref = AttentionReference(bidim, badim)
        self.ref_channel = ref_channel
        self.nmask = bnmask
        if beamformer_type not in BEAMFORMER_TYPES:
            raise ValueError("Not supporting beamformer_type={}".format(beamformer_type))
        if btaps < 0 or bdelay < 1:
            raise ValueError("btaps >= 0 and bdelay >= 1 (btaps=%d, bdelay=%d)" % (btaps, bdelay))
        self.beamformer_type = beamformer_type
        self.btaps = btaps
        self.bdelay = bdelay if btaps > 0 else 1
        self.eps = eps

    def forward(self, data, ilens, return_all=False):
        """data [B,T,C,F,2], ilens [B] -> (enhanced [B,T,F,2], ilens, mask_speech [B,T,C,F]);
        return_all: a dict of the intermediate results (psd_speech, psd_noise, u, ws) as a fourth value; "mpdr" gives its
        covariance as psd_n, "wpd" its covariance as Rf [B,F,N,N,2] float64 and power [B,T,F], both in place of psd_noise"""
        B, T, C, F, _ = data.shape
        if self.beamformer_type == "wpd":                                            # refused before the first launch
            ops.wpd_check_shape(C, self.btaps, self.bdelay)
        logits = self.mask.logits(data, ilens)                                       # [2, B, C, Tm, F]
        psd, feat = get_power_spectral_density_matrix(data, logits, return_feature=True)
        if self.ref_channel < 0:
            u, _ = self.ref(feat, ilens)
        else:                                                                        # fixed reference microphone
            u = torch.zeros(B, C, device=data.device, dtype=torch.float32)
            u[:, self.ref_channel] = 1.0
        if self.beamformer_type == "mvdr":
            extra = dict(psd_noise=psd[1])
            ws = get_mvdr_vector(psd[0], psd[1], u)
            enhanced = apply_beamforming_vector(ws, data)
        elif self.beamformer_type == "mpdr":
            psd_n = get_covariances(data, None, 1, 0, ilens).float()                 # data alone: no gradient
            extra = dict(psd_n=psd_n)
            ws = get_mvdr_vector(psd[0], psd_n, u)
            enhanced = apply_beamforming_vector(ws, data)
        else:
            power = MaskedPowerFn.apply(data, logits[:1])
            Rf = get_covariances_from_power(data, power, self.bdelay, self.btaps, ilens, eps=self.eps)
            extra = dict(Rf=Rf, power=power)
            ws = get_WPD_filter_v2(psd[0], Rf, u)
            enhanced = perform_WPD_filtering(ws, data, self.bdelay, self.btaps, ilens)
        with torch.no_grad():                                                        # the caller's view of the speech mask
            mask_speech = torch.sigmoid(logits[0]).permute(0, 2, 1, 3)
            if mask_speech.size(1) < T:
                mask_speech = torch.nn.functional.pad(mask_speech, [0, 0, 0, 0, 0, T - mask_speech.size(1)], value=0)
        if return_all:
            return enhanced, ilens, mask_speech, dict(psd_speech=psd[0], u=u, ws=ws, logits=logits, **extra)
        return enhanced, ilens, mask_speech

    def predict_mask_logits(self, data, ilens):
        """data [B,T,C,F,2], ilens [B] -> the mask estimator's logits [nmask, B, Tm, C, F], Tm = max(ilens), in the
        layout of the masks the reference's predict_mask returns"""
        return self.mask.logits(data, ilens).permute(0, 1, 3, 2, 4).contiguous()

    def predict_mask(self, data, ilens):
        """espnet2/enh/layers/dnn_beamformer.py:272-287: only the masks, for training them against ideal-mask labels
        -> (tuple of nmask masks (B, T, C, F), zero for Tm <= t < T, ilens)"""
        logits = self.predict_mask_logits(data, ilens)
        masks, _ = ops.EnhMaskFn.apply(logits, None, ops.ENH_ACTS["sigmoid"], False)
        T = data.shape[1]
        if masks.shape[2] < T:
            masks = torch.nn.functional.pad(masks, [0, 0, 0, 0, 0, T - masks.shape[2]], value=0)
        return tuple(masks.unbind(0)), ilens


class AttentionReference(torch.nn.Module):
    def __init__(self, bidim, att_dim):
        super().__init__()
        self.mlp_psd = torch.nn.Linear(bidim, att_dim)
        self.gvec = torch.nn.Linear(att_dim, 1)

    def forward(self, psd_feat, ilens, scaling: float = 2.0):
        """psd_feat [B,C,F]: the amplitude of the speech PSD's off-diagonal row means, which the reference forms from
        psd_in (dnn_beamformer.py:163-170) and eamd_bf_psd writes next to the PSD -> (u [B,C], ilens)"""
        mlp_psd = F_.LinearFn.apply(psd_feat, self.mlp_psd.weight, self.mlp_psd.bias)
        e = F_.LinearFn.apply(R_.ActFn.apply(mlp_psd, ops.ACT_TANH), self.gvec.weight, self.gvec.bias).squeeze(-1)
        u = torch.softmax(scaling * e, dim=-1)                                       # [B, C]: C <= 8 numbers per utterance
        return u, ilens
