"""The WPD convolutional beamformer (Nakatani and Kinoshita, "A Unified Convolutional Beamformer for Simultaneous Denoising
and Dereverberation", IEEE SPL 26, 2019).  reference: espnet2/enh/layers/conv_beamformer.py (same function names), in this
project's layouts, over the kernels of csrc/wpd.hip:

    spectrum  Y              [B, T, C, F, 2]     float32, frequency the fastest axis before (re, im), padded frames zero
    inverse_power            [B, T, F]           the weights w_t (the reference's (B, F, T))
    covariance  Rf           [B, F, N, N, 2]     float64, N = (btaps + 1) C
    speech PSD  Phi          [B, F, C, C, 2]
    filter      h            [B, F, N, 2]
    enhanced                 [B, T, F, 2]

Per utterance b of n = ilens[b] frames and bin f, with K = btaps, D = bdelay, t0 = D + K - 1 and the current frame stacked
on the K delayed ones, v_t = [y_t; y_{t-D}; y_{t-D-1}; ...; y_{t-D-K+1}] (zero before frame 0):

    Rf = sum_{t0 <= t < n} w_t v_t v_t^H
    h  = (Rf^-1 E Phi) u / (tr((Rf^-1 E Phi)[:C]) + 1e-15),   E the first C columns of the identity
    enhanced_t = h^H v_t  for t < n,   0  for t >= n

Each function takes an extra `ilens` and is one autograd.Function; Y is data and gets no gradient.  The sums stop at the
utterance's own length, where the reference sums over all T frames of the padded batch; there the padded frames of a
shorter utterance carry weight 1 / eps on delayed taps that are still speech.  An utterance that fills the batch gives
what the reference gives, and a shorter one what the reference gives on that utterance alone.
The reference's retry with random regularisation when the inverse fails is not reproduced: the solve never fails, a
pivot that is zero, negative or not finite takes reciprocal 0."""
import torch

from ... import ops


def _lengths(ilens, B, T, Cn, btaps, bdelay):
    """ilens (None, a sequence or a tensor) -> list of ints, after the host-side refusals"""
    ops.wpd_check_shape(Cn, btaps, bdelay)
    lens = [T] * B if ilens is None else [int(v) for v in ilens]
    if len(lens) != B:
        raise ValueError(f"{len(lens)} lengths for a batch of {B}")
    for n in lens:
        if n > T:
            raise ValueError(f"an utterance of {n} frames in a batch of {T}")
    return lens


def _device_lens(ilens, Y, btaps, bdelay):
    B, T, Cn = Y.shape[:3]
    lens = _lengths(ilens, B, T, Cn, btaps, bdelay)
    return None if ilens is None else torch.tensor(lens, dtype=torch.int32, device=Y.device)


class CovarianceFn(torch.autograd.Function):
    """(Y, power or weights, lens) -> Rf; the gradient goes to the second argument only"""

    @staticmethod
    def forward(ctx, Y, power, lens, btaps, bdelay, eps, inverse_power):
        Y = Y.contiguous()
        power = None if power is None else power.contiguous()
        ctx.save_for_backward(Y, power, lens)
        ctx.conf = (btaps, bdelay, eps, inverse_power)
        return ops.wpd_cov(Y, power, lens, btaps, bdelay, eps, inverse_power)

    @staticmethod
    def backward(ctx, gRf):
        Y, power, lens = ctx.saved_tensors
        btaps, bdelay, eps, inverse_power = ctx.conf
        if power is None or not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None, None
        gpower = ops.wpd_cov_bwd(Y, gRf.contiguous(), power, lens, btaps, bdelay, eps, inverse_power)
        return None, gpower, None, None, None, None, None


class FilterVectorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Phi, Rf, u):
        Phi, Rf, u = Phi.contiguous(), Rf.contiguous(), u.contiguous()
        keep = any(ctx.needs_input_grad)               # the factor of Rf (B F N^2 complex doubles) only when it will be used
        h, fac, xk = ops.wpd_vector(Rf, Phi, u, keep=keep)
        if keep:
            ctx.save_for_backward(Phi, u, fac, xk)
        return h

    @staticmethod
    def backward(ctx, gh):
        Phi, u, fac, xk = ctx.saved_tensors
        gphi, gu, gRf = ops.wpd_vector_bwd(fac, xk, Phi, u, gh.contiguous())
        return gphi, gRf, gu


class FilteringFn(torch.autograd.Function):
    """(h, Y, lens) -> enhanced; Y is data: no gradient"""

    @staticmethod
    def forward(ctx, h, Y, lens, btaps, bdelay):
        h, Y = h.contiguous(), Y.contiguous()
        ctx.save_for_backward(Y, lens)
        ctx.conf = (btaps, bdelay)
        return ops.wpd_apply(h, Y, lens, btaps, bdelay)

    @staticmethod
    def backward(ctx, ge):
        Y, lens = ctx.saved_tensors
        return ops.wpd_apply_bwd(ge.contiguous(), Y, lens, *ctx.conf), None, None, None, None


def get_covariances(Y, inverse_power, bdelay, btaps, ilens=None):
    """The power-normalised spatio-temporal covariance of the stacked frames (conv_beamformer.py:99-151 without
    get_vector).  Y [B,T,C,F,2], inverse_power [B,T,F] the weights themselves (None: unit weights, the MPDR covariance
    when btaps = 0) -> Rf [B,F,N,N,2] float64, differentiable in inverse_power."""
    lens = _device_lens(ilens, Y, btaps, bdelay)
    return CovarianceFn.apply(Y, inverse_power, lens, int(btaps), int(bdelay), 0.0, False)


def get_covariances_from_power(Y, power, bdelay, btaps, ilens=None, eps=1e-6):
    """get_covariances with the weights 1 / clamp(power, eps) formed inside the kernel, so that the (B, T, F) weights are
    never written; differentiable in power (zero gradient where power <= eps, as clamp gives)"""
    lens = _device_lens(ilens, Y, btaps, bdelay)
    return CovarianceFn.apply(Y, power, lens, int(btaps), int(bdelay), float(eps), True)


def get_WPD_filter_v2(Phi, Rf, reference_vector, eps=1e-15):
    """h = (Rf^-1 E Phi) u / (tr((Rf^-1 E Phi)[:C]) + eps) (conv_beamformer.py:216-280).  Phi [B,F,C,C,2], Rf [B,F,N,N,2]
    float64, reference_vector [B,C] -> [B,F,N,2]; differentiable in all three"""
    if eps != 1e-15:
        raise NotImplementedError("the trace's eps is the reference's default 1e-15, fixed in csrc/wpd.hip")
    return FilterVectorFn.apply(Phi, Rf, reference_vector)


def perform_WPD_filtering(filter_matrix, Y, bdelay, btaps, ilens=None):
    """enhanced[b,t,f] = h^H v_t (conv_beamformer.py:283-304).  filter_matrix [B,F,N,2], Y [B,T,C,F,2] -> [B,T,F,2], exactly
    zero past each length"""
    lens = _device_lens(ilens, Y, btaps, bdelay)
    return FilteringFn.apply(filter_matrix, Y, lens, int(btaps), int(bdelay))
