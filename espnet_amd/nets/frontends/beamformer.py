"""PSD matrices, MVDR filter and filter application.  reference: espnet/nets/pytorch_backend/frontends/beamformer.py
(same function names).  A complex tensor is a float32 tensor with a trailing (re, im) axis, frequency the fastest
axis before it - the layout of Stft.forward - where the reference carries torch_complex.ComplexTensor (..., F, C, T):

    spectrum  xs   [B, T, C, F, 2]
    PSD            [B, F, C, C, 2]     (stacked over the S masks: [S, B, F, C, C, 2])
    filter    ws   [B, F, C, 2]
    enhanced       [B, T, F, 2]

Each function is one autograd.Function over the kernels of csrc/beamformer.hip; the gradient of a complex tensor is
PyTorch's (the (re, im) view of the conjugate Wirtinger derivative), so these compose with ordinary torch code."""
import torch

from ... import ops


class PsdFn(torch.autograd.Function):
    """(xs, mask logits) -> (psd [S,B,F,C,C,2], feat [B,C,F]); xs is data: no gradient"""

    @staticmethod
    def forward(ctx, xs, logits):
        xs, logits = xs.contiguous(), logits.contiguous()
        ctx.set_materialize_grads(False)
        psd, feat, nrm = ops.bf_psd(xs, logits)
        ctx.save_for_backward(xs, logits, psd, nrm)
        return psd, feat

    @staticmethod
    def backward(ctx, gpsd, gfeat):
        xs, logits, psd, nrm = ctx.saved_tensors
        if gpsd is None and gfeat is None:
            return None, None
        gpsd = None if gpsd is None else gpsd.contiguous()
        gfeat = None if gfeat is None else gfeat.contiguous()
        return None, ops.bf_psd_bwd(xs, logits, psd, nrm, gpsd, gfeat)


class MvdrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, psd_s, psd_n, u):
        psd_s, psd_n, u = psd_s.contiguous(), psd_n.contiguous(), u.contiguous()
        ctx.save_for_backward(psd_s, psd_n, u)
        return ops.bf_mvdr(psd_s, psd_n, u)

    @staticmethod
    def backward(ctx, gw):
        psd_s, psd_n, u = ctx.saved_tensors
        gs, gn, gu = ops.bf_mvdr_bwd(psd_s, psd_n, u, gw.contiguous())
        return gs, gn, gu


class ApplyFn(torch.autograd.Function):
    """(ws, mix) -> enhanced; mix is data: no gradient"""

    @staticmethod
    def forward(ctx, ws, mix):
        ws, mix = ws.contiguous(), mix.contiguous()
        ctx.save_for_backward(mix)
        return ops.bf_apply(ws, mix)

    @staticmethod
    def backward(ctx, gy):
        (mix,) = ctx.saved_tensors
        return ops.bf_apply_bwd(gy.contiguous(), mix), None


def get_power_spectral_density_matrix(xs, mask_logits, return_feature=False):
    """Cross-channel PSD matrices of xs [B,T,C,F,2] under S masks, beamformer.py:6-37 with normalization=True, eps 1e-15.

    `mask_logits` [S,B,C,Tm,F] are the mask estimator's LOGITS, not masks: the sigmoid is taken inside the kernel, so the
    reference's (B, F, C, T) masks are never written.  Tm <= T; frames Tm..T-1 carry mask 0 (mask_estimator.py:73-74).
    As in the reference, the normaliser sums the channel-averaged mask over all Tm frames - also those past an
    utterance's own length, whose masks the reference leaves at sigmoid(bias) (`masked_fill` without the underscore,
    mask_estimator.py:67).

    -> psd [S,B,F,C,C,2]; with return_feature also the attention reference's input of the first (speech) mask,
    feat [B,C,F] = |sum_{e != c} psd[0,b,f,c,e]| / (C - 1) (dnn_beamformer.py:163-170)."""
    psd, feat = PsdFn.apply(xs, mask_logits)
    return (psd, feat) if return_feature else psd


def get_mvdr_vector(psd_s, psd_n, reference_vector):
    """h = (Npsd^-1 Spsd) / (Tr(Npsd^-1 Spsd) + eps) u with Npsd + eps I, eps = 1e-15 (beamformer.py:40-76).
    psd_s, psd_n [B,F,C,C,2], reference_vector [B,C] -> [B,F,C,2].  psd_n is not modified."""
    return MvdrFn.apply(psd_s, psd_n, reference_vector)


def apply_beamforming_vector(beamform_vector, mix):
    """es[b,t,f] = sum_c conj(beamform_vector[b,f,c]) mix[b,t,c,f] (beamformer.py:79-84) -> [B,T,F,2]"""
    return ApplyFn.apply(beamform_vector, mix)
