"""WPE dereverberation (Nakatani et al. 2010): one iteration of the weighted-prediction-error filter.  The reference's
DNN_WPE (espnet/nets/pytorch_backend/frontends/dnn_wpe.py) takes `wpe_one_iteration` from the pytorch_wpe package; this
is that function (same name and defaults) in this project's layouts, over the kernels of csrc/wpe.hip:

    spectrum  Y      [B, T, C, F, 2]   float32, frequency the fastest axis before (re, im), padded frames zero
    power            [B, T, F]         the time-varying variance estimate (already averaged over the channels)
    enhanced         [B, T, C, F, 2]

Per utterance b of n = ilens[b] frames and bin f, with K = taps, D = delay and the K delayed frames stacked into
h_t = [y_{t-D}; y_{t-D-1}; ...; y_{t-D-K+1}] (zero before frame 0), t0 = D + K - 1:

    w_t = 1 / max(power_t, eps)                (inverse_power=False: w_t = power_t as given)
    R = sum_{t0 <= t < n} w_t h_t h_t^H,    P = sum_{t0 <= t < n} w_t h_t y_t^H,    G = R^-1 P
    x_t = y_t - G^H h_t  for t < n,   x_t = 0  for t >= n

The sums stop at the utterance's own length; pytorch_wpe sums over all T frames of the padded batch, which lets the
first t0 padded frames of a shorter utterance (power 0, so weight 1 / eps, and a history that is still speech) dominate
R.  An utterance in a batch therefore gives what the same utterance gives alone."""
import torch

from ... import ops


def _lengths(ilens, B, T, Cn, taps, delay):
    """ilens (None, a sequence or a tensor) -> list of ints, after the host-side refusals"""
    ops.wpe_check_shape(Cn, taps, delay)
    lens = [T] * B if ilens is None else [int(v) for v in ilens]
    if len(lens) != B:
        raise ValueError(f"{len(lens)} lengths for a batch of {B}")
    for n in lens:
        if n > T:
            raise ValueError(f"an utterance of {n} frames in a batch of {T}")
        if n - (delay + taps - 1) < Cn * taps:
            raise ValueError(f"utterance too short for WPE: {n} frames leave {n - (delay + taps - 1)} usable ones, fewer than "
                             f"the C * taps = {Cn * taps} unknowns (taps={taps}, delay={delay})")
    return lens


class WpeFn(torch.autograd.Function):
    """(Y, power, lens) -> enhanced; Y is data: the gradient goes to power only"""

    @staticmethod
    def forward(ctx, Y, power, lens, taps, delay, eps, inverse_power):
        Y, power = Y.contiguous(), power.contiguous()
        keep = ctx.needs_input_grad[1]                     # the factor of R (B F N^2 complex doubles) only when it will be used
        G, fac = ops.wpe_taps(Y, power, lens, taps, delay, eps, inverse_power, keep_factor=keep)
        x = ops.wpe_filter(Y, G, lens, taps, delay)
        if keep:
            ctx.save_for_backward(Y, power, lens, fac, x)
            ctx.conf = (taps, delay, eps, inverse_power)
        return x

    @staticmethod
    def backward(ctx, gx):
        Y, power, lens, fac, x = ctx.saved_tensors
        taps, delay, eps, inverse_power = ctx.conf
        gpower = ops.wpe_bwd(Y, x, gx.contiguous(), power, lens, fac, taps, delay, eps, inverse_power)
        return None, gpower, None, None, None, None, None


def wpe_one_iteration(Y, power, ilens=None, taps=10, delay=3, eps=1e-10, inverse_power=True):
    """Y [B,T,C,F,2], power [B,T,F], ilens [B] (None: every utterance fills the batch) -> enhanced [B,T,C,F,2]"""
    B, T, Cn, F, _ = Y.shape
    lens = _lengths(ilens, B, T, Cn, taps, delay)
    dev = None if ilens is None else torch.tensor(lens, dtype=torch.int32, device=Y.device)
    return WpeFn.apply(Y, power, dev, int(taps), int(delay), float(eps), bool(inverse_power))


def get_filter_matrix(Y, power, ilens=None, taps=10, delay=3, eps=1e-10, inverse_power=True):
    """The prediction filter G alone, without a gradient -> [B, F, taps, C, C, 2]: G[b,f,k,c,e] multiplies (conjugated)
    y[t - delay - k, c] in the estimate of the reverberation of channel e"""
    B, T, Cn, F, _ = Y.shape
    lens = _lengths(ilens, B, T, Cn, taps, delay)
    dev = None if ilens is None else torch.tensor(lens, dtype=torch.int32, device=Y.device)
    with torch.no_grad():
        G, _ = ops.wpe_taps(Y.contiguous(), power.contiguous(), dev, int(taps), int(delay), float(eps), bool(inverse_power),
                            keep_factor=False)
    return G.view(B, taps, Cn, Cn, F, 2).permute(0, 4, 1, 2, 3, 5).contiguous()
