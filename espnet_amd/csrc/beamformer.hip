// Mask-based MVDR beamforming front-end (reference: espnet/nets/pytorch_backend/frontends/beamformer.py:6-84 and
// dnn_beamformer.py:163-170): masked cross-channel PSD matrices, the MVDR solve and the filter application, forward and
// backward, on interleaved (re, im) fp32 spectra x [B, T, C, F, 2] exactly as Stft.forward lays them out.
//
// Layout decision shared by all kernels: ONE LANE OWNS ONE FREQUENCY BIN.  Frequency is the fastest axis of x, of the mask
// logits z [S, B, C, Tm, F] and of every output over (t, f), so a wave reads 64 consecutive bins of one (b, t, c) row:
// 512 contiguous bytes of x, 256 of z.  Everything that couples channels (the C x C Hermitian matrices, the solve, the
// filter) is private to a lane: no cross-lane traffic, no LDS in the streaming kernels.
//
//   psd        (b, 64-bin tile, 64-frame chunk, pair of masks) per one-wave workgroup.  The lane keeps, per mask, the upper
//              triangle of sum_t m[t] x_t x_t^H (C real diagonals + C(C-1)/2 complex) and sum_t m[t] in registers; x is read
//              ONCE for both masks; the sigmoid of the logits is taken in the loop, the [B, F, C, T] masks never exist.
//              The chunk partials go to a workspace; a second kernel adds them in chunk order (deterministic, no atomics),
//              divides by n = sum_t m[t] + 1e-15, mirrors the triangle and forms the attention feature from mask 0.
//   psd_bwd    a per-(s, b, f) preparation (Hermitian part H of the incoming gradient incl. the feature's, over n) and two
//              streaming passes: chunk partials of q = sum_t m[t] x_t^H H x_t / n, then dz = sigmoid'(z) / C * (x_t^H H x_t - q).
//   mvdr       one lane per (b, f): Gauss-Jordan with partial pivoting on [A | S] (A = psd_n + 1e-15 I) in LDS, laid out
//              [element][lane] (a lane's own column: bank = lane, conflict-free whatever row a lane pivots on).
//   mvdr_bwd   the same elimination on [A | S | I], then the adjoint of  w = (N / (tr N + eps)) u,  N = A^-1 S.
//   apply      y[b,t,f] = sum_c conj(w[b,f,c]) x[b,t,c,f];  apply_bwd: dw = sum_t conj(dy) x, chunk partials + ordered sum.
//
// Complex cotangents follow PyTorch: g is the tensor with dL = Re sum conj(g) dv, stored (re, im) like the value.
#include "common.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int kLanes = 64;                  // frequency bins per workgroup = one wave
constexpr int kTChunk = EAMD_BF_TCHUNK;     // frames per workgroup of the T-split kernels
constexpr int kMinC = 2, kMaxC = 8;
constexpr float kEps = 1e-15f;

__host__ __device__ constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }

// IEEE division and libm's expf, not common.h's v_rcp / v_exp sigmoid: a mask near 1 enters the backward as 1 - m, where
// an error of a few ulp of m is a large relative one; the tests hold these kernels to the fp32 reference's own error
__device__ __forceinline__ float bf_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// sigmoid'(x) = e / (1 + e)^2 with e = exp(-|x|): no cancellation in 1 - m, no overflow
__device__ __forceinline__ float bf_dsigmoid(float x) {
  const float e = expf(-fabsf(x)), s = 1.0f / (1.0f + e);
  return e * s * s;
}

// ---------------------------------------------------------------------------------------------------------------------
// PSD forward
// ---------------------------------------------------------------------------------------------------------------------
// plane k of a (s, b) slab of K = C*C + 1 planes [K][F]: 0..C-1 the real diagonal, then (re, im) of the upper triangle in
// row-major (c < e) order, last the mask sum
template <int C>
__global__ __launch_bounds__(kLanes) void psd_partial_kernel(const float2* __restrict__ x, const float* __restrict__ z,
                                                             float* __restrict__ part, int S, int B, int T, int Tm, int F) {
  constexpr int NU = C * (C - 1) / 2, K = C * C + 1;
  const int f = blockIdx.x * kLanes + threadIdx.x;
  if (f >= F) return;
  const int chunk = blockIdx.y;
  const int b = blockIdx.z % B, s0 = 2 * (blockIdx.z / B);
  const bool two = s0 + 1 < S;
  float dg[2][C], ur[2][NU], ui[2][NU], ms[2] = {0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int c = 0; c < C; ++c) dg[s][c] = 0.f;
#pragma unroll
    for (int k = 0; k < NU; ++k) ur[s][k] = ui[s][k] = 0.f;
  }
  const int t0 = chunk * kTChunk;
  const int t1 = t0 + kTChunk < Tm ? t0 + kTChunk : Tm;     // frames >= Tm carry mask 0: nothing to add
  const long zs = (long)B * C * Tm * F;                      // stride between masks
  for (int t = t0; t < t1; ++t) {
    const float2* xp = x + ((long)b * T + t) * C * F + f;
    const float* zp = z + (((long)s0 * B + b) * C * Tm + t) * F + f;
    float2 xv[C];
    float m0 = 0.f, m1 = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      xv[c] = xp[(long)c * F];
      m0 += bf_sigmoid(zp[(long)c * Tm * F]);
      if (two) m1 += bf_sigmoid(zp[zs + (long)c * Tm * F]);
    }
    m0 *= 1.0f / C;
    m1 *= 1.0f / C;
    ms[0] += m0;
    ms[1] += m1;
    int k = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float p = xv[c].x * xv[c].x + xv[c].y * xv[c].y;
      dg[0][c] += m0 * p;
      dg[1][c] += m1 * p;
#pragma unroll
      for (int e = c + 1; e < C; ++e, ++k) {                 // x_c conj(x_e)
        const float re = xv[c].x * xv[e].x + xv[c].y * xv[e].y;
        const float im = xv[c].y * xv[e].x - xv[c].x * xv[e].y;
        ur[0][k] += m0 * re; ui[0][k] += m0 * im;
        ur[1][k] += m1 * re; ui[1][k] += m1 * im;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s == 1 && !two) break;
    float* o = part + (((long)chunk * S + (s0 + s)) * B + b) * K * F + f;
#pragma unroll
    for (int c = 0; c < C; ++c) o[(long)c * F] = dg[s][c];
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      o[(long)(C + 2 * k) * F] = ur[s][k];
      o[(long)(C + 2 * k + 1) * F] = ui[s][k];
    }
    o[(long)(K - 1) * F] = ms[s];
  }
}

template <int C>
__global__ __launch_bounds__(256) void psd_final_kernel(const float* __restrict__ part, float2* __restrict__ psd,
                                                        float* __restrict__ feat, float* __restrict__ nrm, int S, int B,
                                                        int F, int nchunk) {
  constexpr int NU = C * (C - 1) / 2, K = C * C + 1;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;       // (s, b, f), f fastest
  if (i >= (long)S * B * F) return;
  const int f = (int)(i % F);
  const long sb = i / F;
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.f;
  const long slab = (long)S * B * K * F;
  const float* p = part + sb * K * F + f;
  for (int ch = 0; ch < nchunk; ++ch) {                             // chunk order: the same bits on every launch
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += p[(long)ch * slab + (long)k * F];
  }
  const float n = acc[K - 1] + kEps;
  const float inv = 1.0f / n;
  nrm[i] = n;
  float2* o = psd + i * C * C;
  float rr[C], ri[C];
#pragma unroll
  for (int c = 0; c < C; ++c) rr[c] = ri[c] = 0.f;
  int k = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    o[c * C + c] = make_float2(acc[c] * inv, 0.f);
#pragma unroll
    for (int e = c + 1; e < C; ++e, ++k) {
      const float re = acc[C + 2 * k] * inv, im = acc[C + 2 * k + 1] * inv;
      o[c * C + e] = make_float2(re, im);
      o[e * C + c] = make_float2(re, -im);
      rr[c] += re; ri[c] += im;
      rr[e] += re; ri[e] -= im;
    }
  }
  if (sb < B) {                                                     // mask 0 = speech: the attention reference's input
    const int b = (int)sb;
#pragma unroll
    for (int c = 0; c < C; ++c)
      feat[((long)b * C + c) * F + f] = sqrtf(rr[c] * rr[c] + ri[c] * ri[c]) * (1.0f / (C - 1));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// PSD backward
// ---------------------------------------------------------------------------------------------------------------------
// coef planes of a (s, b) slab [C*C][F]: H_cc / n (C), then 2 H_ce / n as (re, im) for c < e;  H = (G + G^H) / 2
template <int C>
__global__ __launch_bounds__(256) void psd_bwd_prep_kernel(const float2* __restrict__ gpsd, const float* __restrict__ gfeat,
                                                           const float2* __restrict__ psd, const float* __restrict__ nrm,
                                                           float* __restrict__ coef, int S, int B, int F) {
  constexpr int K = C * C;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)S * B * F) return;
  const int f = (int)(i % F);
  const long sb = i / F;
  float2 G[C * C];
#pragma unroll
  for (int k = 0; k < C * C; ++k) G[k] = gpsd ? gpsd[i * C * C + k] : make_float2(0.f, 0.f);
  if (sb < B && gfeat) {          // feat_c = |r_c| / (C - 1), r_c = sum_{e != c} psd[c, e]:  G[c, e] += gfeat_c r_c / (|r_c| (C - 1))
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float rr = 0.f, ri = 0.f;
#pragma unroll
      for (int e = 0; e < C; ++e)
        if (e != c) { const float2 p = psd[i * C * C + c * C + e]; rr += p.x; ri += p.y; }
      const float a = sqrtf(rr * rr + ri * ri);
      const float g = a > 0.f ? gfeat[((long)sb * C + c) * F + f] / (a * (C - 1)) : 0.f;
#pragma unroll
      for (int e = 0; e < C; ++e)
        if (e != c) { G[c * C + e].x += g * rr; G[c * C + e].y += g * ri; }
    }
  }
  const float inv = 1.0f / nrm[i];
  float* o = coef + sb * K * F + f;
  int k = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    o[(long)c * F] = G[c * C + c].x * inv;
#pragma unroll
    for (int e = c + 1; e < C; ++e, ++k) {                            // 2 H_ce = G_ce + conj(G_ec)
      o[(long)(C + 2 * k) * F] = (G[c * C + e].x + G[e * C + c].x) * inv;
      o[(long)(C + 2 * k + 1) * F] = (G[c * C + e].y - G[e * C + c].y) * inv;
    }
  }
}

// dL/dm[t] = gw[t] - q,  gw[t] = x_t^H (H / n) x_t,  q = sum_t m[t] gw[t] / n  (= <G, psd> / n).  q is formed from the SAME
// fp32 values gw[t] and m[t] that it is subtracted from, in a pass of its own (WRITE = false: chunk partials of
// sum_t m[t] gw[t] and sum_t m[t]; WRITE = true: dz), and these two sums, their quotient and the subtraction are carried in
// double (four scalar operations per frame; everything per channel pair stays fp32).  The reason: any error of q is common
// to all frames, and a gradient that sums dz over time - the bias of the mask Linear, where gw[t] - q cancels to 1e-3 of its
// terms - amplifies it a thousandfold.  With q from the rounded fp32 psd that gradient came out ten to thirty times less
// accurate than an fp32 autograd of the reference, with fp32 sums still four to five times (both measured on an MI355X).
template <int C, bool WRITE>
__global__ __launch_bounds__(kLanes) void psd_bwd_kernel(const float2* __restrict__ x, const float* __restrict__ z,
                                                         const float* __restrict__ coef, const float* __restrict__ nrm,
                                                         double* __restrict__ qpart, float* __restrict__ dz, int S, int B, int T,
                                                         int Tm, int F, int nchunk) {
  constexpr int NU = C * (C - 1) / 2, K = C * C;
  const int f = blockIdx.x * kLanes + threadIdx.x;
  if (f >= F) return;
  const int b = blockIdx.z % B, s0 = 2 * (blockIdx.z / B);
  const bool two = s0 + 1 < S;
  float hd[2][C], hr[2][NU], hi[2][NU];
  double q[2] = {0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bool live = s == 0 || two;
    const long sb = (long)(s0 + (live ? s : 0)) * B + b;
    const float* p = coef + sb * K * F + f;
#pragma unroll
    for (int c = 0; c < C; ++c) hd[s][c] = live ? p[(long)c * F] : 0.f;
#pragma unroll
    for (int k = 0; k < NU; ++k) {
      hr[s][k] = live ? p[(long)(C + 2 * k) * F] : 0.f;
      hi[s][k] = live ? p[(long)(C + 2 * k + 1) * F] : 0.f;
    }
    if (WRITE && live) {
      double num = 0.0, den = (double)kEps;
      for (int ch = 0; ch < nchunk; ++ch) {                                                  // chunk order
        num += qpart[(((long)ch * S * B + sb) * F + f) * 2];
        den += qpart[(((long)ch * S * B + sb) * F + f) * 2 + 1];
      }
      q[s] = num / den;
    }
  }
  const int t0 = blockIdx.y * kTChunk;
  const int t1 = t0 + kTChunk < Tm ? t0 + kTChunk : Tm;
  const long zs = (long)B * C * Tm * F;
  double a0 = 0.0, a1 = 0.0, n0 = 0.0, n1 = 0.0;
  for (int t = t0; t < t1; ++t) {
    const float2* xp = x + ((long)b * T + t) * C * F + f;
    float2 xv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) xv[c] = xp[(long)c * F];
    float v0 = 0.f, v1 = 0.f;
    int k = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float p = xv[c].x * xv[c].x + xv[c].y * xv[c].y;
      v0 += hd[0][c] * p;
      v1 += hd[1][c] * p;
#pragma unroll
      for (int e = c + 1; e < C; ++e, ++k) {
        const float re = xv[c].x * xv[e].x + xv[c].y * xv[e].y;
        const float im = xv[c].y * xv[e].x - xv[c].x * xv[e].y;
        v0 += hr[0][k] * re + hi[0][k] * im;
        v1 += hr[1][k] * re + hi[1][k] * im;
      }
    }
    const long o = (((long)s0 * B + b) * C * Tm + t) * F + f;
    if (!WRITE) {
      float m0 = 0.f, m1 = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        m0 += bf_sigmoid(z[o + (long)c * Tm * F]);
        if (two) m1 += bf_sigmoid(z[o + (long)c * Tm * F + zs]);
      }
      m0 *= 1.0f / C;
      m1 *= 1.0f / C;
      a0 += (double)m0 * v0; n0 += m0;
      a1 += (double)m1 * v1; n1 += m1;
    } else {
      v0 = (float)((double)v0 - q[0]) * (1.0f / C);
      v1 = (float)((double)v1 - q[1]) * (1.0f / C);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const long oc = o + (long)c * Tm * F;
        dz[oc] = bf_dsigmoid(z[oc]) * v0;
        if (two) dz[oc + zs] = bf_dsigmoid(z[oc + zs]) * v1;
      }
    }
  }
  if (!WRITE) {
    double* o = qpart + ((((long)blockIdx.y * S + s0) * B + b) * F + f) * 2;
    o[0] = a0; o[1] = n0;
    if (two) { o[(long)B * F * 2] = a1; o[(long)B * F * 2 + 1] = n1; }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// MVDR
// ---------------------------------------------------------------------------------------------------------------------
struct Cx { float re, im; };
__device__ __forceinline__ Cx cmul(Cx a, Cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ Cx cconj(Cx a) { return {a.re, -a.im}; }
// 1 / a; 0 for a == 0 (a singular pivot gives a finite, meaningless answer, never NaN)
__device__ __forceinline__ Cx cinv(Cx a) {
  const float d = a.re * a.re + a.im * a.im;
  if (!(d > 0.f)) return {0.f, 0.f};
  const float r = 1.0f / d;
  return {a.re * r, -a.im * r};
}

// a lane's private C x W complex matrix in LDS: element (r, c) at m[((r * W + c) * 2 + part) * 64]
struct LMat {
  float* m; int W;
  __device__ __forceinline__ Cx get(int r, int c) const {
    const float* p = m + (r * W + c) * 2 * kLanes;
    return {p[0], p[kLanes]};
  }
  __device__ __forceinline__ void set(int r, int c, Cx v) const {
    float* p = m + (r * W + c) * 2 * kLanes;
    p[0] = v.re; p[kLanes] = v.im;
  }
};

// Gauss-Jordan with partial (row) pivoting on the C x W system [A | right-hand sides]: A -> I, the rest -> A^-1 (rest)
__device__ void gauss_jordan(const LMat a, int C) {
  const int W = a.W;
  for (int k = 0; k < C; ++k) {
    int best = k;
    Cx p = a.get(k, k);
    float bv = p.re * p.re + p.im * p.im;
    for (int r = k + 1; r < C; ++r) {
      const Cx v = a.get(r, k);
      const float m = v.re * v.re + v.im * v.im;
      if (m > bv) { bv = m; best = r; }
    }
    if (best != k)
      for (int c = k; c < W; ++c) {
        const Cx u = a.get(k, c), v = a.get(best, c);
        a.set(k, c, v);
        a.set(best, c, u);
      }
    const Cx ip = cinv(a.get(k, k));
    for (int c = k; c < W; ++c) a.set(k, c, cmul(a.get(k, c), ip));
    for (int r = 0; r < C; ++r) {
      if (r == k) continue;
      const Cx fct = a.get(r, k);
      for (int c = k; c < W; ++c) {
        const Cx v = a.get(r, c), w = cmul(fct, a.get(k, c));
        a.set(r, c, {v.re - w.re, v.im - w.im});
      }
    }
  }
}

__device__ __forceinline__ void load_system(const LMat a, const float2* __restrict__ ps, const float2* __restrict__ pn,
                                            long i, int C, bool identity) {
  for (int r = 0; r < C; ++r)
    for (int c = 0; c < C; ++c) {
      const float2 n = pn[i * C * C + r * C + c], s = ps[i * C * C + r * C + c];
      a.set(r, c, {n.x + (r == c ? kEps : 0.f), n.y});
      a.set(r, C + c, {s.x, s.y});
      if (identity) a.set(r, 2 * C + c, {r == c ? 1.f : 0.f, 0.f});
    }
}

__global__ __launch_bounds__(kLanes) void mvdr_kernel(const float2* __restrict__ ps, const float2* __restrict__ pn,
                                                      const float* __restrict__ u, float2* __restrict__ w, int B, int F, int C) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const long i = (long)blockIdx.x * kLanes + threadIdx.x;          // (b, f)
  if (i >= (long)B * F) return;
  const LMat a{lds + threadIdx.x, 2 * C};
  load_system(a, ps, pn, i, C, false);
  gauss_jordan(a, C);
  Cx d = {kEps, 0.f};
  for (int c = 0; c < C; ++c) { const Cx v = a.get(c, C + c); d.re += v.re; d.im += v.im; }
  const Cx invd = cinv(d);
  const float* ub = u + (i / F) * C;
  for (int e = 0; e < C; ++e) {
    Cx acc = {0.f, 0.f};
    for (int c = 0; c < C; ++c) { const Cx v = a.get(e, C + c); acc.re += v.re * ub[c]; acc.im += v.im * ub[c]; }
    acc = cmul(acc, invd);
    w[i * C + e] = make_float2(acc.re, acc.im);
  }
}

// w = W u, W = N / d, d = tr N + eps, N = A^-1 S.  With gW = gw u^T:  gN = gW / conj(d) + gd I,
// gd = -sum gW conj(N) / conj(d)^2,  gS = A^-H gN,  gA = -gS N^H,  gu_c = Re sum_e conj(gw_e) W_ec
__global__ __launch_bounds__(kLanes) void mvdr_bwd_kernel(const float2* __restrict__ ps, const float2* __restrict__ pn,
                                                          const float* __restrict__ u, const float2* __restrict__ gw,
                                                          float2* __restrict__ gps, float2* __restrict__ gpn,
                                                          float* __restrict__ gu_part, int B, int F, int C) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const long i = (long)blockIdx.x * kLanes + threadIdx.x;
  if (i >= (long)B * F) return;
  const LMat a{lds + threadIdx.x, 3 * C};
  const LMat v{lds + 3 * C * C * 2 * kLanes + threadIdx.x, 2};      // C x 2: column 0 = gw, column 1 = y = A^-H gw
  load_system(a, ps, pn, i, C, true);
  gauss_jordan(a, C);
  Cx d = {kEps, 0.f};
  for (int c = 0; c < C; ++c) { const Cx t = a.get(c, C + c); d.re += t.re; d.im += t.im; }
  const Cx invd = cinv(d), cinvd = cconj(invd);
  const float* ub = u + (i / F) * C;
  for (int e = 0; e < C; ++e) { const float2 g = gw[i * C + e]; v.set(e, 0, {g.x, g.y}); }
  Cx gd = {0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    Cx col = {0.f, 0.f};                                            // sum_e conj(gw_e) N_ec
    for (int e = 0; e < C; ++e) { const Cx t = cmul(cconj(v.get(e, 0)), a.get(e, C + c)); col.re += t.re; col.im += t.im; }
    gu_part[i * C + c] = col.re * invd.re - col.im * invd.im;       // Re(col / d)
    gd.re -= ub[c] * col.re;                                        // -sum_ec gw_e u_c conj(N_ec) = -conj(sum_c u_c col_c)
    gd.im += ub[c] * col.im;
  }
  gd = cmul(gd, cmul(cinvd, cinvd));
  for (int e = 0; e < C; ++e) {
    Cx y = {0.f, 0.f};
    for (int k = 0; k < C; ++k) { const Cx t = cmul(cconj(a.get(k, 2 * C + e)), v.get(k, 0)); y.re += t.re; y.im += t.im; }
    v.set(e, 1, cmul(y, cinvd));
  }
  for (int e = 0; e < C; ++e)
    for (int c = 0; c < C; ++c) {                                   // gS into the (now identity) A block
      const Cx y = v.get(e, 1), t = cmul(gd, cconj(a.get(c, 2 * C + e)));
      const Cx g = {y.re * ub[c] + t.re, y.im * ub[c] + t.im};
      a.set(e, c, g);
      gps[i * C * C + e * C + c] = make_float2(g.re, g.im);
    }
  for (int e = 0; e < C; ++e)
    for (int c = 0; c < C; ++c) {
      Cx acc = {0.f, 0.f};
      for (int k = 0; k < C; ++k) { const Cx t = cmul(a.get(e, k), cconj(a.get(c, C + k))); acc.re += t.re; acc.im += t.im; }
      gpn[i * C * C + e * C + c] = make_float2(-acc.re, -acc.im);
    }
}

// gu[b, c] = sum_f part[b, f, c]: one wave per (b, c), lanes stride over f, a fixed tree - the same bits every launch
__global__ __launch_bounds__(kLanes) void mvdr_gu_kernel(const float* __restrict__ part, float* __restrict__ gu, int F, int C) {
  const int b = blockIdx.x / C, c = blockIdx.x % C;
  float acc = 0.f;
  for (int f = threadIdx.x; f < F; f += kLanes) acc += part[((long)b * F + f) * C + c];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) gu[blockIdx.x] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// filter application
// ---------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kLanes) void apply_kernel(const float2* __restrict__ w, const float2* __restrict__ x,
                                                       float2* __restrict__ y, int B, int T, int F) {
  const int f = blockIdx.x * kLanes + threadIdx.x;
  if (f >= F) return;
  const int b = blockIdx.z;
  float2 wv[C];
#pragma unroll
  for (int c = 0; c < C; ++c) wv[c] = w[((long)b * F + f) * C + c];
  const int t0 = blockIdx.y * kTChunk;
  const int t1 = t0 + kTChunk < T ? t0 + kTChunk : T;
  for (int t = t0; t < t1; ++t) {
    const float2* xp = x + ((long)b * T + t) * C * F + f;
    float re = 0.f, im = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {                                   // conj(w) x
      const float2 xv = xp[(long)c * F];
      re += wv[c].x * xv.x + wv[c].y * xv.y;
      im += wv[c].x * xv.y - wv[c].y * xv.x;
    }
    y[((long)b * T + t) * F + f] = make_float2(re, im);
  }
}

// part [chunk][b][2C][F]: planes (re, im) of sum_{t in chunk} conj(gy[b,t,f]) x[b,t,c,f]
template <int C>
__global__ __launch_bounds__(kLanes) void apply_bwd_partial_kernel(const float2* __restrict__ gy, const float2* __restrict__ x,
                                                                   float* __restrict__ part, int B, int T, int F) {
  const int f = blockIdx.x * kLanes + threadIdx.x;
  if (f >= F) return;
  const int b = blockIdx.z;
  float ar[C], ai[C];
#pragma unroll
  for (int c = 0; c < C; ++c) ar[c] = ai[c] = 0.f;
  const int t0 = blockIdx.y * kTChunk;
  const int t1 = t0 + kTChunk < T ? t0 + kTChunk : T;
  for (int t = t0; t < t1; ++t) {
    const float2 g = gy[((long)b * T + t) * F + f];
    const float2* xp = x + ((long)b * T + t) * C * F + f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float2 xv = xp[(long)c * F];
      ar[c] += g.x * xv.x + g.y * xv.y;
      ai[c] += g.x * xv.y - g.y * xv.x;
    }
  }
  float* o = part + ((long)blockIdx.y * B + b) * 2 * C * F + f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    o[(long)(2 * c) * F] = ar[c];
    o[(long)(2 * c + 1) * F] = ai[c];
  }
}

__global__ __launch_bounds__(256) void apply_bwd_final_kernel(const float* __restrict__ part, float* __restrict__ gw, int B,
                                                              int F, int C2, int nchunk) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;       // (b, k, f), f fastest; k = 2 c + part
  if (i >= (long)B * C2 * F) return;
  const int f = (int)(i % F), k = (int)((i / F) % C2);
  const long b = i / ((long)F * C2);
  float acc = 0.f;
  for (int ch = 0; ch < nchunk; ++ch) acc += part[(long)ch * B * C2 * F + i];
  gw[(b * F + f) * C2 + k] = acc;
}

inline bool bad_c(int C) { return C < kMinC || C > kMaxC; }

#define BF_DISPATCH_C(C, ...)                                                                                        \
  switch (C) {                                                                                                         \
    case 2: { constexpr int C_ = 2; __VA_ARGS__; } break;                                                                     \
    case 3: { constexpr int C_ = 3; __VA_ARGS__; } break;                                                                     \
    case 4: { constexpr int C_ = 4; __VA_ARGS__; } break;                                                                     \
    case 5: { constexpr int C_ = 5; __VA_ARGS__; } break;                                                                     \
    case 6: { constexpr int C_ = 6; __VA_ARGS__; } break;                                                                     \
    case 7: { constexpr int C_ = 7; __VA_ARGS__; } break;                                                                     \
    default: { constexpr int C_ = 8; __VA_ARGS__; } break;                                                                    \
  }

}  // namespace

extern "C" {

int64_t eamd_bf_workspace_bytes(int op, int S, int B, int T, int C, int F) {
  if (S < 1 || B < 1 || T < 1 || F < 1 || bad_c(C)) return EAMD_EINVAL;
  const int64_t nchunk = ceil_div(T, kTChunk);
  switch (op) {
    case EAMD_BF_PSD: return 4 * nchunk * S * B * (C * C + 1) * F;
    case EAMD_BF_PSD_BWD: return 4 * (C * C + 4 * nchunk) * S * B * F + 8;      // coefficients, pad, double partials
    case EAMD_BF_MVDR_BWD: return (int64_t)4 * B * F * C;
    case EAMD_BF_APPLY_BWD: return 4 * nchunk * B * 2 * C * F;
    default: return EAMD_EINVAL;
  }
}

int eamd_bf_psd(const float* x, const float* z, float* psd, float* feat, float* nrm, void* workspace, int S, int B, int T,
                int Tm, int C, int F, void* stream) {
  if (!x || !z || !psd || !feat || !nrm || !workspace) return EAMD_EINVAL;
  if (S < 1 || B < 1 || T < 1 || Tm < 1 || Tm > T || F < 1) return EAMD_EINVAL;
  if (bad_c(C)) return EAMD_EUNSUPPORTED;
  const int pairs = ceil_div(S, 2), nchunk = ceil_div(Tm, kTChunk);
  if ((long)B * pairs > 65535 || nchunk > 65535) return EAMD_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ceil_div(F, kLanes), nchunk, B * pairs);
  const int fin = (int)(((long)S * B * F + 255) / 256);
  BF_DISPATCH_C(C, {
    hipLaunchKernelGGL(psd_partial_kernel<C_>, grid, dim3(kLanes), 0, st, (const float2*)x, z, (float*)workspace, S, B, T, Tm, F);
    hipLaunchKernelGGL(psd_final_kernel<C_>, dim3(fin), dim3(256), 0, st, (const float*)workspace, (float2*)psd, feat, nrm, S, B,
                       F, nchunk);
  });
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_bf_psd_bwd(const float* x, const float* z, const float* psd, const float* nrm, const float* gpsd, const float* gfeat,
                    float* dz, void* workspace, int S, int B, int T, int Tm, int C, int F, void* stream) {
  if (!x || !z || !psd || !nrm || !dz || !workspace || (!gpsd && !gfeat)) return EAMD_EINVAL;
  if (S < 1 || B < 1 || T < 1 || Tm < 1 || Tm > T || F < 1) return EAMD_EINVAL;
  if (bad_c(C)) return EAMD_EUNSUPPORTED;
  const int pairs = ceil_div(S, 2), nchunk = ceil_div(Tm, kTChunk);
  if ((long)B * pairs > 65535 || nchunk > 65535) return EAMD_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ceil_div(F, kLanes), nchunk, B * pairs);
  const int pre = (int)(((long)S * B * F + 255) / 256);
  BF_DISPATCH_C(C, {
    float* coef = (float*)workspace;
    double* qpart = (double*)(coef + (((long)S * B * C * C * F + 1) & ~1L));     /* S B C C F floats: 8-byte aligned when even */
    hipLaunchKernelGGL(psd_bwd_prep_kernel<C_>, dim3(pre), dim3(256), 0, st, (const float2*)gpsd, gfeat, (const float2*)psd, nrm,
                       coef, S, B, F);
    hipLaunchKernelGGL((psd_bwd_kernel<C_, false>), grid, dim3(kLanes), 0, st, (const float2*)x, z, (const float*)coef, nrm,
                       qpart, dz, S, B, T, Tm, F, nchunk);
    hipLaunchKernelGGL((psd_bwd_kernel<C_, true>), grid, dim3(kLanes), 0, st, (const float2*)x, z, (const float*)coef, nrm,
                       qpart, dz, S, B, T, Tm, F, nchunk);
  });
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_bf_mvdr(const float* psd_s, const float* psd_n, const float* u, float* w, int B, int F, int C, void* stream) {
  if (!psd_s || !psd_n || !u || !w) return EAMD_EINVAL;
  if (B < 1 || F < 1) return EAMD_EINVAL;
  if (bad_c(C)) return EAMD_EUNSUPPORTED;
  const size_t lds = (size_t)C * 2 * C * 2 * kLanes * sizeof(float);            // <= 64 KB at C = 8
  const int blocks = (int)(((long)B * F + kLanes - 1) / kLanes);
  hipLaunchKernelGGL(mvdr_kernel, dim3(blocks), dim3(kLanes), lds, (hipStream_t)stream, (const float2*)psd_s,
                     (const float2*)psd_n, u, (float2*)w, B, F, C);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_bf_mvdr_bwd(const float* psd_s, const float* psd_n, const float* u, const float* gw, float* gpsd_s, float* gpsd_n,
                     float* gu, void* workspace, int B, int F, int C, void* stream) {
  if (!psd_s || !psd_n || !u || !gw || !gpsd_s || !gpsd_n || !gu || !workspace) return EAMD_EINVAL;
  if (B < 1 || F < 1) return EAMD_EINVAL;
  if (bad_c(C)) return EAMD_EUNSUPPORTED;
  const size_t lds = ((size_t)C * 3 * C + 2 * C) * 2 * kLanes * sizeof(float);  // 104 KB at C = 8
  static const hipError_t attr_err = hipFuncSetAttribute(reinterpret_cast<const void*>(&mvdr_bwd_kernel),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (attr_err != hipSuccess) return (int)attr_err;
  const int blocks = (int)(((long)B * F + kLanes - 1) / kLanes);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mvdr_bwd_kernel, dim3(blocks), dim3(kLanes), lds, st, (const float2*)psd_s, (const float2*)psd_n, u,
                     (const float2*)gw, (float2*)gpsd_s, (float2*)gpsd_n, (float*)workspace, B, F, C);
  hipLaunchKernelGGL(mvdr_gu_kernel, dim3(B * C), dim3(kLanes), 0, st, (const float*)workspace, gu, F, C);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_bf_apply(const float* w, const float* x, float* y, int B, int T, int C, int F, void* stream) {
  if (!w || !x || !y) return EAMD_EINVAL;
  if (B < 1 || T < 1 || F < 1) return EAMD_EINVAL;
  if (bad_c(C)) return EAMD_EUNSUPPORTED;
  const int nchunk = ceil_div(T, kTChunk);
  if (B > 65535 || nchunk > 65535) return EAMD_EUNSUPPORTED;
  const dim3 grid(ceil_div(F, kLanes), nchunk, B);
  BF_DISPATCH_C(C, hipLaunchKernelGGL(apply_kernel<C_>, grid, dim3(kLanes), 0, (hipStream_t)stream, (const float2*)w,
                                      (const float2*)x, (float2*)y, B, T, F));
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_bf_apply_bwd(const float* gy, const float* x, float* gw, void* workspace, int B, int T, int C, int F, void* stream) {
  if (!gy || !x || !gw || !workspace) return EAMD_EINVAL;
  if (B < 1 || T < 1 || F < 1) return EAMD_EINVAL;
  if (bad_c(C)) return EAMD_EUNSUPPORTED;
  const int nchunk = ceil_div(T, kTChunk);
  if (B > 65535 || nchunk > 65535) return EAMD_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ceil_div(F, kLanes), nchunk, B);
  BF_DISPATCH_C(C, hipLaunchKernelGGL(apply_bwd_partial_kernel<C_>, grid, dim3(kLanes), 0, st, (const float2*)gy,
                                      (const float2*)x, (float*)workspace, B, T, F));
  const int fin = (int)(((long)B * 2 * C * F + 255) / 256);
  hipLaunchKernelGGL(apply_bwd_final_kernel, dim3(fin), dim3(256), 0, st, (const float*)workspace, gw, B, F, 2 * C, nchunk);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
