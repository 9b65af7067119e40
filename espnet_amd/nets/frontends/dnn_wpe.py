"""DNN-supported WPE dereverberation (Kinoshita et al. 2017).  reference:
espnet/nets/pytorch_backend/frontends/dnn_wpe.py (same class name, constructor arguments, defaults and parameter names).
Spectra are float32 [B, T, C, F, 2] (Stft.forward's layout), see wpe.py."""
import torch

from ... import ops
from .mask_estimator import MaskEstimator
from .wpe import _lengths, wpe_one_iteration


class MaskedPowerFn(torch.autograd.Function):
    """(data, mask logits [1,B,C,Tm,F]) -> power [B,T,F] = mean_c |data|^2 sigmoid(logits); data gets no gradient.  The
    reference's (B, F, C, T) mask is never written."""

    @staticmethod
    def forward(ctx, data, logits):
        data, logits = data.contiguous(), logits.contiguous()
        ctx.save_for_backward(data, logits)
        return ops.wpe_power(data, logits)

    @staticmethod
    def backward(ctx, gpower):
        data, logits = ctx.saved_tensors
        return None, ops.wpe_power_bwd(data, logits, gpower.contiguous())


class DNN_WPE(torch.nn.Module):
    def __init__(self, wtype="blstmp", widim=257, wlayers=3, wunits=300, wprojs=320, dropout_rate=0.0, taps=5, delay=3,
                 use_dnn_mask=True, iterations=1, normalization=False):
        super().__init__()
        if normalization:
            raise NotImplementedError("normalization=True (the mask divided by its sum over time) is not implemented: the "
                                      "reference's Frontend never sets it, and its sum runs over padded frames too")
        ops.wpe_check_shape(1, taps, delay)
        self.iterations = iterations
        self.taps = taps
        self.delay = delay
        self.normalization = normalization
        self.use_dnn_mask = use_dnn_mask
        self.inverse_power = True
        if self.use_dnn_mask:
            self.mask_est = MaskEstimator(wtype, widim, wlayers, wunits, wprojs, dropout_rate, nmask=1)

    def forward(self, data, ilens):
        """data [B,T,C,F,2], ilens [B] -> (enhanced [B,T,C,F,2], ilens, mask [B,T,C,F] or None without the DNN mask).
        Every iteration filters `data`; only the power estimate comes from the previous iteration's output."""
        B, T, C, F, _ = data.shape
        _lengths(ilens, B, T, C, self.taps, self.delay)                              # refusals before the first launch
        enhanced = data
        logits = None
        for i in range(self.iterations):
            if i == 0 and self.use_dnn_mask:
                logits = self.mask_est.logits(data, ilens)                           # [1, B, C, Tm, F]
                power = MaskedPowerFn.apply(data, logits)
            elif i == 0:
                power = ops.wpe_power(data.contiguous())
            else:                                                                    # carries the gradient to iteration i - 1
                power = enhanced.square().sum(-1).mean(dim=2)
            enhanced = wpe_one_iteration(data, power, ilens, taps=self.taps, delay=self.delay,
                                         inverse_power=self.inverse_power)
        mask = None
        if logits is not None:
            with torch.no_grad():                                                    # the caller's view of the mask
                mask = torch.sigmoid(logits[0]).permute(0, 2, 1, 3)
                if mask.size(1) < T:
                    mask = torch.nn.functional.pad(mask, [0, 0, 0, 0, 0, T - mask.size(1)], value=0)
        return enhanced, ilens, mask

    def predict_mask(self, data, ilens):
        """-> (mask [B,T,C,F], ilens), or (None, ilens) without the DNN mask (dnn_wpe.py of espnet2 has the same method)"""
        if not self.use_dnn_mask:
            return None, ilens
        with torch.no_grad():
            mask = torch.sigmoid(self.mask_est.logits(data, ilens)[0]).permute(0, 2, 1, 3)
            if mask.size(1) < data.shape[1]:
                mask = torch.nn.functional.pad(mask, [0, 0, 0, 0, 0, data.shape[1] - mask.size(1)], value=0)
        return mask, ilens
