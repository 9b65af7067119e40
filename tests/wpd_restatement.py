"""The WPD convolutional beamformer (and the MPDR covariance) restated on torch's native complex tensors (complex128 by
default): the yardstick of the kernels of csrc/wpd.hip and of DNN_Beamformer("wpd" / "mpdr").  Test infrastructure only -
the product tree never imports it.  tests/test_wpd.py pins it to tests/golden/wpd.npz, recorded from the reference's
espnet2/enh/layers/conv_beamformer.py by tools/gen_golden_wpd.py.

Layouts are those of espnet_amd.nets.frontends with the (re, im) axis folded into the dtype:
    y [B,T,C,F] complex, power [B,T,F] real, Phi [B,F,C,C] complex, u [B,C] real, Rf [B,F,N,N], h [B,F,N], e [B,T,F].
For utterance b of n = ilens[b] frames, K = btaps, D = bdelay, N = (K + 1) C, t0 = D + K - 1 and the stacked vector
v_t = [y_t; y_{t-D}; ...; y_{t-D-K+1}] (0 before frame 0):
    Rf = sum_{t0<=t<n} w_t v_t v_t^H,  X = Rf^-1 E,  M = X Phi,  tau = tr(M[:C]) + 1e-15,  h = M u / tau,  e_t = h^H v_t (0 for t >= n).
Every function runs in the dtype of its inputs, so the same code in float32 / complex64 on the CPU gives the error an fp32
evaluation in library order makes (`err_vs`)."""
import torch

import beamformer_restatement as R
from beamformer_restatement import cx, err_vs, ri  # noqa: F401
from wpe_restatement import masked_power, synth  # noqa: F401

EPS = 1e-6            # DNN_Beamformer's floor of the power
TRACE_EPS = 1e-15
# (C, btaps, bdelay, T, ilens): the cases of the issue; the last has N = 64, the kernels' limit, and three time chunks
CASES = ((1, 5, 3, 40, (40, 31)), (2, 5, 3, 64, (64, 50)), (3, 2, 1, 33, (33, 20)), (4, 0, 1, 40, (40, 31)),
         (8, 5, 3, 96, (96, 80)), (8, 7, 2, 130, (130, 121)))
IDS = ["C%dK%dD%d" % c[:3] for c in CASES]


def inputs(ci, F, seed=0, zero_bin=False):
    """seeded float32-valued inputs of case ci -> (y [B,T,C,F] complex64, speech-mask logits z [1,B,C,T,F], Phi [B,F,C,C]
    complex64 = the speech PSD of y under z rounded to float32, u [B,C] float32 summing to 1)"""
    C, K, D, T, ilens = CASES[ci]
    y, z = synth(C, T, ilens, F, seed=seed, zero_bin=zero_bin)
    phi = R.psd_matrices(y.to(torch.complex128), z.double())[0].to(torch.complex64)
    g = torch.Generator().manual_seed(77 + ci)
    u = torch.softmax(torch.randn(len(ilens), C, generator=g), dim=-1)
    return y, z, phi, u


def stacked(yb, btaps, bdelay):
    """yb [n,C,F] -> v [n, (K+1)*C, F]: v[t, c] = yb[t, c], v[t, (k+1)*C + c] = yb[t - bdelay - k, c], zero before frame 0"""
    n, C, F = yb.shape
    pad = torch.cat([yb.new_zeros(bdelay + btaps, C, F), yb])
    rows = [yb] + [pad[btaps - k:btaps - k + n] for k in range(btaps)]
    return torch.stack(rows, dim=1).reshape(n, (btaps + 1) * C, F)


def weights(power_b, btaps, bdelay, eps=EPS, inverse_power=True):
    """power_b [n,F] (None: ones) -> w [n,F], zero for t < t0"""
    w = 1.0 / torch.clamp(power_b, min=eps) if inverse_power else power_b
    keep = (torch.arange(w.shape[0]) >= bdelay + btaps - 1).to(w.dtype)
    return w * keep[:, None]


def covariance(yb, power_b, btaps, bdelay, eps=EPS, inverse_power=True):
    """-> (v [n,N,F], Rf [F,N,N])"""
    v = stacked(yb, btaps, bdelay)
    w = weights(power_b, btaps, bdelay, eps, inverse_power).to(yb.dtype)
    return v, torch.einsum("tf,tif,tjf->fij", w, v, v.conj())


def filter_vector(phi_b, Rf, u_b, return_parts=False):
    """phi_b [F,C,C], Rf [F,N,N], u_b [C] -> h [F,N] (and X, M, tau)"""
    C, N = phi_b.shape[-1], Rf.shape[-1]
    E = torch.eye(N, C, dtype=Rf.dtype).expand(Rf.shape[0], N, C)
    X = torch.linalg.solve(Rf, E)
    M = X @ phi_b
    tau = M[:, :C].diagonal(dim1=-2, dim2=-1).sum(-1) + TRACE_EPS
    h = torch.einsum("fic,c->fi", M, u_b.to(M.dtype)) / tau[:, None]
    return (h, X, M, tau) if return_parts else h


def wpd(y, power, phi, u, ilens, btaps, bdelay, eps=EPS, inverse_power=True):
    """-> dict(Rf [B,F,N,N], h [B,F,N], e [B,T,F]); differentiable in power, phi and u.  power None: unit weights"""
    B, T, C, F = y.shape
    Rfs, hs, es = [], [], []
    for b in range(B):
        n = int(ilens[b])
        pb = torch.ones(n, F, dtype=y.real.dtype) if power is None else power[b, :n]
        v, Rf = covariance(y[b, :n], pb, btaps, bdelay, eps, inverse_power and power is not None)
        h = filter_vector(phi[b], Rf, u[b])
        e = torch.einsum("fi,tif->tf", h.conj(), v)
        Rfs.append(Rf), hs.append(h), es.append(torch.cat([e, e.new_zeros(T - n, F)]))
    return dict(Rf=torch.stack(Rfs), h=torch.stack(hs), e=torch.stack(es))


def wpd_backward(y, power, phi, u, ilens, btaps, bdelay, ge, eps=EPS, inverse_power=True):
    """the closed-form gradients of L at (u, phi, power), given ge = the cotangent of e (dL = Re sum conj(ge) de); no
    autograd -> dict(gu [B,C], gphi [B,F,C,C], gpower [B,T,F]):
    gh = sum_{t<n} conj(ge_t) v_t, gv = gh / conj(tau), gtau = -(sum_i gh_i conj(h_i)) / conj(tau), gM = gv u^T + gtau E,
    gu = Re(M^H gv) summed over f, gphi = X^H gM, gX = gM phi^H, Z = Rf^-1 gX, gw_t = -Re((v_t^H Z)(X^H v_t)) for t0 <= t < n,
    gpower = -gw / power^2 where power > eps (inverse_power=False: gw)"""
    B, T, C, F = y.shape
    gu, gphi, gpower = torch.zeros_like(u), torch.zeros_like(phi), torch.zeros_like(power)
    with torch.no_grad():
        for b in range(B):
            n = int(ilens[b])
            v, Rf = covariance(y[b, :n], power[b, :n], btaps, bdelay, eps, inverse_power)
            h, X, M, tau = filter_vector(phi[b], Rf, u[b], return_parts=True)
            N = Rf.shape[-1]
            gh = torch.einsum("tf,tif->fi", ge[b, :n].conj(), v)
            gv = gh / tau.conj()[:, None]
            gtau = -(gh * h.conj()).sum(-1) / tau.conj()
            gM = gv[:, :, None] * u[b].to(gv.dtype)[None, None, :] + gtau[:, None, None] * torch.eye(N, C, dtype=gv.dtype)
            gu[b] = torch.einsum("fic,fi->c", M.conj(), gv).real
            gphi[b] = X.conj().transpose(-1, -2) @ gM
            Z = torch.linalg.solve(Rf, gM @ phi[b].conj().transpose(-1, -2))
            gw = -(torch.einsum("tif,fic->tfc", v.conj(), Z) * torch.einsum("fic,tif->tfc", X.conj(), v)).sum(-1).real
            gw[:bdelay + btaps - 1] = 0
            p = power[b, :n]
            gpower[b, :n] = torch.where(p > eps, -gw / (p * p), torch.zeros_like(gw)) if inverse_power else gw
    return dict(gu=gu, gphi=gphi, gpower=gpower)


def dnn_beamformer(sd, x, ilens, beamformer_type="wpd", btaps=5, bdelay=3, ref_channel=-1, eps=EPS):
    """DNN_Beamformer.forward of the "wpd" and "mpdr" types restated; sd: the module's state_dict in the dtype to compute
    in -> dict of every stage (beamformer_restatement.dnn_beamformer is the "mvdr" type)"""
    B, T, C, F = x.shape
    z = R.mask_logits(sd, x, ilens)
    psd = R.psd_matrices(x, z)
    if ref_channel < 0:
        u = R.attention_reference(sd, R.psd_feature(psd[0]))
    else:
        u = torch.zeros(B, C, dtype=x.real.dtype)
        u[:, ref_channel] = 1.0
    out = dict(logits=z, psd_speech=psd[0], u=u, mask_speech=R.masks_full(z[0], T).detach())
    if beamformer_type == "mpdr":
        psd_n = wpd(x, None, psd[0], u, ilens, 0, 1)["Rf"]
        ws = R.mvdr_vector(psd[0], psd_n, u)
        out.update(psd_n=psd_n, ws=ws, enhanced=R.apply_vector(ws, x))
    else:
        if btaps == 0:
            bdelay = 1
        power = masked_power(x, z[:1])
        r = wpd(x, power, psd[0], u, ilens, btaps, bdelay, eps)
        out.update(power=power, Rf=r["Rf"], ws=r["h"], enhanced=r["e"])
    return out
