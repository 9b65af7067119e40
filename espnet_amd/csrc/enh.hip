// Speech enhancement training (the reference's espnet2/enh task): inverse-STFT overlap-add, mask application, the pairwise
// time-frequency and SI-SNR criteria of ESPnetEnhancementModel, and the permutation pick, forward and backward.
//
// Layouts.  Spectra are interleaved (re, im) fp32.  With n the flat inner size of one utterance (T F or T C F):
//   mix [B, n, 2], ref [S, B, n, 2]; an estimate is real [S, B, n] (mask logits, masks) or complex [S, B, n, 2];
//   waveforms est, ref [S, B, L].  pair [B, S, S] fp64: pair[b, s, t] = criterion(reference s, estimate t).
//
// Precision.  Memory is fp32, but for the few sums per utterance (pair, the SI-SNR sums), which stay fp64 up to the loss.
// Every element is evaluated in fp64 from the fp32 operands except the activation itself (expf / tanhf), and every sum
// longer than one frame is fp64: the SI-SNR closed form  Ee - D^2 (2 / te - Er / te^2)  cancels to the noise energy, 1e-6
// of its terms at 60 dB.  bf16 is never used.
//
// Reductions run in two stages and use no atomics: a workgroup sums kChunk elements of one utterance (a thread its
// strided elements in order, a wave by shuffles, the four waves in wave order) and writes its partial; a finishing kernel
// adds the partials in chunk order.  The grid is a function of the shape alone, so two launches give identical bits.
//
// Each operand is read once per pass: all S^2 pairs of an element are formed from one read of the S references, the S
// estimates and the mixture, where the reference's Python loop over permutations reads them S! S times.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;                  // elements of one utterance per workgroup (16 per thread)
constexpr int kMaxSpk = 3;
constexpr double kMaskEps = 10e-12;           // tf_mask_net.py:95, the literal
constexpr double kLabelEps = 10e-8;           // espnet_model.py:64, the literal
constexpr double kSnrEps = 1e-8;              // espnet_model.py:374

enum { ENH_ACT_SIGMOID = 0, ENH_ACT_RELU = 1, ENH_ACT_TANH = 2, ENH_ACT_NONE = 3 };
enum { MODE_MASK = 0, MODE_MAG = 1, MODE_SPEC = 2, MODE_REAL = 3 };
enum { IBM = 0, IRM = 1, IAM = 2, PSM = 3, NPSM = 4, PSM2 = 5 };
enum { SNR_ZEROMEAN = 0, SNR_L2NORM = 1 };

__device__ __forceinline__ float enh_act(float x, int act) {
  if (act == ENH_ACT_SIGMOID) return 1.0f / (1.0f + expf(-x));
  if (act == ENH_ACT_RELU) return fmaxf(x, 0.0f);
  if (act == ENH_ACT_TANH) return tanhf(x);
  return x;
}
// d act / d x from the input x and the activated value m
__device__ __forceinline__ double enh_dact(float x, float m, int act) {
  if (act == ENH_ACT_SIGMOID) return (double)m * (1.0 - (double)m);
  if (act == ENH_ACT_RELU) return x > 0.0f ? 1.0 : 0.0;
  if (act == ENH_ACT_TANH) return 1.0 - (double)m * (double)m;
  return 1.0;
}
__device__ __forceinline__ double cabs2(float2 z) { return sqrt((double)z.x * z.x + (double)z.y * z.y); }
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// permutation k of itertools.permutations(range(S)), S <= 3; an index out of range reads as 0
__device__ __forceinline__ void perm_of(int S, long k, int (&p)[kMaxSpk]) {
  p[0] = 0; p[1] = 1; p[2] = 2;
  if (S == 2 && k == 1) { p[0] = 1; p[1] = 0; }
  if (S == 3 && k > 0 && k < 6) {
    const int first = (int)k / 2, lo = first == 0 ? 1 : 0, hi = first == 2 ? 1 : 2;
    p[0] = first;
    p[1] = (k % 2 == 0) ? lo : hi;
    p[2] = (k % 2 == 0) ? hi : lo;
  }
}

template <int S>
__device__ __forceinline__ void inverse_of(const int (&perm)[kMaxSpk], int (&inv)[kMaxSpk]) {
#pragma unroll
  for (int t = 0; t < kMaxSpk; ++t) {
    inv[t] = t;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (perm[s] == t) inv[t] = s;
  }
}

// the ideal-mask label of reference s (espnet_model.py:47-104).  ar: |r| of all S references, ax = |mix|.
// NPSM clamps to [-1, 1] like PSM: the reference compares the list mask_label, not mask_type, with "NPSM" (:89).
template <int S>
__device__ __forceinline__ double mask_label(int type, int s, const float2 (&r)[S], const double (&ar)[S], float2 X, double ax) {
  if (type == IBM) {
    bool all = true;
#pragma unroll
    for (int q = 0; q < S; ++q) all = all && (ar[s] >= ar[q]);
    return all ? 1.0 : 0.0;
  }
  if (type == IRM) {
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < S; ++q) sum += ar[q];
    return ar[s] / (sum + kLabelEps);
  }
  if (type == IAM) return clampd(ar[s] / (ax + kLabelEps), 0.0, 1.0);
  const double dr = ar[s] + kLabelEps, dx = ax + kLabelEps;
  const double cos_theta = ((double)r[s].x / dr) * ((double)X.x / dx) + ((double)r[s].y / dr) * ((double)X.y / dx);
  if (type == PSM2) return clampd(ar[s] * ar[s] / (ax * ax + kLabelEps) * cos_theta, -1.0, 1.0);
  return clampd(ar[s] / (ax + kLabelEps) * cos_theta, -1.0, 1.0);
}

// sum of v[0..NV) over the workgroup in a fixed order -> out[0..NV)
template <int NV>
__device__ __forceinline__ void block_sum_store(double (&v)[NV], double* __restrict__ out) {
  __shared__ double red[kThreads / 64][NV];
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double x = v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) red[wave][i] = x;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += red[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// ---- inverse STFT: gather-form overlap-add ------------------------------------------------------------------------------
// wav[b, n] = sum_t w[p - t hop] frames[b, t, p - t hop] / sum_t w[p - t hop]^2, p = n + pad, over the frames covering p;
// zeros for siglen <= n < length
__global__ __launch_bounds__(kThreads) void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ w,
                                                             float* __restrict__ wav, int T, int n_fft, int hop, int pad,
                                                             int siglen, int length) {
  const int n = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
  if (n >= length) return;
  float out = 0.0f;
  if (n < siglen) {
    const int p = n + pad;
    const int t_hi = min(T - 1, p / hop), t_lo = p >= n_fft ? (p - n_fft) / hop + 1 : 0;
    double s = 0.0, env = 0.0;
    for (int t = t_lo; t <= t_hi; ++t) {
      const int k = p - t * hop;
      const double wk = w[k];
      s += wk * (double)frames[((long)b * T + t) * n_fft + k];
      env += wk * wk;
    }
    out = (float)(s / env);
  }
  wav[(long)b * length + n] = out;
}

// g[b, p] = dwav[b, p - pad] / env[p] for 0 <= p - pad < siglen, 0 elsewhere; rows of ldg = rpu hop samples and a zero tail
__global__ __launch_bounds__(kThreads) void istft_ola_bwd_kernel(const float* __restrict__ dwav, const float* __restrict__ w,
                                                                 float* __restrict__ g, int B, int T, int n_fft, int hop, int pad,
                                                                 int siglen, int length, long ldg, long total) {
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const long b = idx / ldg;
  const int p = (int)(idx - b * ldg), n = p - pad;
  float out = 0.0f;
  if (b < B && n >= 0 && n < siglen) {
    const int t_hi = min(T - 1, p / hop), t_lo = p >= n_fft ? (p - n_fft) / hop + 1 : 0;
    double env = 0.0;
    for (int t = t_lo; t <= t_hi; ++t) {
      const double wk = w[p - t * hop];
      env += wk * wk;
    }
    out = (float)((double)dwav[b * length + n] / env);
  }
  g[idx] = out;
}

// ---- mask application ---------------------------------------------------------------------------------------------------
// m_s = act(logit_s), P_s = X m_s |X| / (|X| + 10e-12)   (tf_mask_net.py:94-116); X == NULL: the masks only
__global__ __launch_bounds__(kThreads) void mask_apply_kernel(const float* __restrict__ logits, const float2* __restrict__ X,
                                                              float* __restrict__ mask, float2* __restrict__ P, int S, long Bn,
                                                              int act) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < Bn; i += (long)gridDim.x * kThreads) {
    float2 x = make_float2(0.f, 0.f);
    double ratio = 0.0;
    if (X) {
      x = X[i];
      const double ax = cabs2(x);
      ratio = ax / (ax + kMaskEps);
    }
    for (int s = 0; s < S; ++s) {
      const float m = enh_act(logits[s * Bn + i], act);
      if (mask) mask[s * Bn + i] = m;
      if (P) P[s * Bn + i] = make_float2((float)(x.x * (m * ratio)), (float)(x.y * (m * ratio)));
    }
  }
}

// dlogit_s = act'(logit_s) (gmask_s + Re(conj(X) gP_s) |X| / (|X| + 10e-12)); either cotangent may be NULL
__global__ __launch_bounds__(kThreads) void mask_apply_bwd_kernel(const float* __restrict__ logits, const float2* __restrict__ X,
                                                                  const float* __restrict__ gmask, const float2* __restrict__ gP,
                                                                  float* __restrict__ dlogits, int S, long Bn, int act) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < Bn; i += (long)gridDim.x * kThreads) {
    float2 x = make_float2(0.f, 0.f);
    double ratio = 0.0;
    if (gP) {
      x = X[i];
      const double ax = cabs2(x);
      ratio = ax / (ax + kMaskEps);
    }
    for (int s = 0; s < S; ++s) {
      const float l = logits[s * Bn + i];
      const float m = enh_act(l, act);
      double g = gmask ? (double)gmask[s * Bn + i] : 0.0;
      if (gP) {
        const float2 gp = gP[s * Bn + i];
        g += ratio * ((double)x.x * gp.x + (double)x.y * gp.y);
      }
      dlogits[s * Bn + i] = (float)(g * enh_dact(l, m, act));
    }
  }
}

// ---- pairwise time-frequency criteria -----------------------------------------------------------------------------------
// part[b][chunk][s S + t] = sum over the chunk of the squared error between reference s and estimate t
template <int S>
__global__ __launch_bounds__(kThreads) void pair_tf_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                           const float2* __restrict__ mix, double* __restrict__ part, int B, long n,
                                                           int nchunk, int mode, int label, int act) {
  const int b = blockIdx.y, ch = blockIdx.x;
  const long i0 = (long)ch * kChunk, i1 = min(n, i0 + (long)kChunk);
  const float2* est2 = reinterpret_cast<const float2*>(est);
  const float2* ref2 = reinterpret_cast<const float2*>(ref);
  double acc[S * S];
#pragma unroll
  for (int k = 0; k < S * S; ++k) acc[k] = 0.0;
  for (long i = i0 + threadIdx.x; i < i1; i += kThreads) {
    if (mode == MODE_MASK) {
      const float2 X = mix[(long)b * n + i];
      const double ax = cabs2(X);
      float2 r[S];
      double ar[S], m[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        r[s] = ref2[((long)s * B + b) * n + i];
        ar[s] = cabs2(r[s]);
        m[s] = enh_act(est[((long)s * B + b) * n + i], act);
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const double lab = mask_label<S>(label, s, r, ar, X, ax);
#pragma unroll
        for (int t = 0; t < S; ++t) acc[s * S + t] += (lab - m[t]) * (lab - m[t]);
      }
    } else if (mode == MODE_REAL) {
      double r[S], e[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        r[s] = ref[((long)s * B + b) * n + i];
        e[s] = est[((long)s * B + b) * n + i];
      }
#pragma unroll
      for (int s = 0; s < S; ++s)
#pragma unroll
        for (int t = 0; t < S; ++t) acc[s * S + t] += (r[s] - e[t]) * (r[s] - e[t]);
    } else {
      float2 r[S], e[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        r[s] = ref2[((long)s * B + b) * n + i];
        e[s] = est2[((long)s * B + b) * n + i];
      }
      if (mode == MODE_MAG) {
        double ar[S], ae[S];
#pragma unroll
        for (int s = 0; s < S; ++s) { ar[s] = cabs2(r[s]); ae[s] = cabs2(e[s]); }
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
          for (int t = 0; t < S; ++t) acc[s * S + t] += (ar[s] - ae[t]) * (ar[s] - ae[t]);
      } else {
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
          for (int t = 0; t < S; ++t) {
            const double dx = (double)r[s].x - e[t].x, dy = (double)r[s].y - e[t].y;
            acc[s * S + t] += dx * dx + dy * dy;
          }
      }
    }
  }
  block_sum_store<S * S>(acc, part + ((long)b * nchunk + ch) * (S * S));
}

// pair[b][k] = (sum of the chunk partials in chunk order) / n
__global__ __launch_bounds__(kThreads) void pair_tf_finish_kernel(const double* __restrict__ part, double* __restrict__ pair, int B,
                                                                  int SS, int nchunk, double inv_n) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * SS) return;
  const int b = idx / SS, k = idx % SS;
  double s = 0.0;
  for (int ch = 0; ch < nchunk; ++ch) s += part[((long)b * nchunk + ch) * SS + k];
  pair[idx] = s * inv_n;
}

// the gradient of the estimate alone: d loss_b / d est_t with loss_b = sum_s pair[b, s, perm[s]] / S, times cot[b].
// magnitude: |P| is differentiated as 0 at P = 0 (every padded frame), where the reference gets inf * 0 = NaN.
template <int S>
__global__ __launch_bounds__(kThreads) void pair_tf_bwd_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                               const float2* __restrict__ mix, const int64_t* __restrict__ perm_index,
                                                               const float* __restrict__ cot, float* __restrict__ dest, int B, long n,
                                                               int mode, int label, int act) {
  const int b = blockIdx.y;
  const long i0 = (long)blockIdx.x * kChunk, i1 = min(n, i0 + (long)kChunk);
  const float2* est2 = reinterpret_cast<const float2*>(est);
  const float2* ref2 = reinterpret_cast<const float2*>(ref);
  float2* dest2 = reinterpret_cast<float2*>(dest);
  int perm[kMaxSpk], inv[kMaxSpk];
  perm_of(S, perm_index[b], perm);
  inverse_of<S>(perm, inv);                                         // the reference that estimate t is paired with
  const double coef = 2.0 * (double)cot[b] / ((double)S * (double)n);
  for (long i = i0 + threadIdx.x; i < i1; i += kThreads) {
    if (mode == MODE_MASK) {
      const float2 X = mix[(long)b * n + i];
      const double ax = cabs2(X);
      float2 r[S];
      double ar[S];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        r[s] = ref2[((long)s * B + b) * n + i];
        ar[s] = cabs2(r[s]);
      }
#pragma unroll
      for (int t = 0; t < S; ++t) {
        const long at = ((long)t * B + b) * n + i;
        const float l = est[at];
        const float m = enh_act(l, act);
        double lab = 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s)
          if (s == inv[t]) lab = mask_label<S>(label, s, r, ar, X, ax);
        dest[at] = (float)(coef * ((double)m - lab) * enh_dact(l, m, act));
      }
    } else if (mode == MODE_REAL) {
      double r[S];
#pragma unroll
      for (int s = 0; s < S; ++s) r[s] = ref[((long)s * B + b) * n + i];
#pragma unroll
      for (int t = 0; t < S; ++t) {
        const long at = ((long)t * B + b) * n + i;
        double rs = 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s)
          if (s == inv[t]) rs = r[s];
        dest[at] = (float)(coef * ((double)est[at] - rs));
      }
    } else {
      float2 r[S];
#pragma unroll
      for (int s = 0; s < S; ++s) r[s] = ref2[((long)s * B + b) * n + i];
#pragma unroll
      for (int t = 0; t < S; ++t) {
        const long at = ((long)t * B + b) * n + i;
        const float2 e = est2[at];
        float2 rs = make_float2(0.f, 0.f);
#pragma unroll
        for (int s = 0; s < S; ++s)
          if (s == inv[t]) rs = r[s];
        if (mode == MODE_MAG) {
          const double ae = cabs2(e), g = ae > 0.0 ? coef * (ae - cabs2(rs)) / ae : 0.0;
          dest2[at] = make_float2((float)(g * e.x), (float)(g * e.y));
        } else {
          dest2[at] = make_float2((float)(coef * ((double)e.x - rs.x)), (float)(coef * ((double)e.y - rs.y)));
        }
      }
    }
  }
}

// ---- pairwise SI-SNR ----------------------------------------------------------------------------------------------------
// the sums of one utterance, in this order: sum r_s [S], sum r_s^2 [S], sum e_t [S], sum e_t^2 [S], sum r_s e_t [S][S]
__host__ __device__ constexpr int snr_nv(int S) { return 4 * S + S * S; }

template <int S>
__global__ __launch_bounds__(kThreads) void pair_sisnr_kernel(const float* __restrict__ est, const float* __restrict__ ref,
                                                              double* __restrict__ part, int B, long L, int nchunk) {
  const int b = blockIdx.y, ch = blockIdx.x;
  const long i0 = (long)ch * kChunk, i1 = min(L, i0 + (long)kChunk);
  double acc[snr_nv(S)];
#pragma unroll
  for (int k = 0; k < snr_nv(S); ++k) acc[k] = 0.0;
  for (long i = i0 + threadIdx.x; i < i1; i += kThreads) {
    double r[S], e[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      r[s] = ref[((long)s * B + b) * L + i];
      e[s] = est[((long)s * B + b) * L + i];
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
      acc[s] += r[s];
      acc[S + s] += r[s] * r[s];
      acc[2 * S + s] += e[s];
      acc[3 * S + s] += e[s] * e[s];
#pragma unroll
      for (int t = 0; t < S; ++t) acc[4 * S + s * S + t] += r[s] * e[t];
    }
  }
  block_sum_store<snr_nv(S)>(acc, part + ((long)b * nchunk + ch) * snr_nv(S));
}

// the criterion of (reference s, estimate t) and, for the backward, d loss / d e_i = a e_i + b r_i + c, from the sums.
//   zero-mean (espnet_model.py:367-405): D = sum r~ e~, Er = sum r~^2, Ee = sum e~^2 (~: mean over the full L removed),
//     te = Er + eps, P = D^2 Er / te^2, N = Ee - D^2 (2 / te - Er / te^2) + eps, loss = -10 log10(P / N + eps)
//   L2-normalised (:348-364): A = sum r e, loss = -10 log10(A^2 / (sum r^2 sum e^2 - A^2))
struct SnrTerm { double loss, a, b, c; };
__device__ __forceinline__ SnrTerm snr_term(const double* __restrict__ sums, int S, int s, int t, double L, int mode) {
  const double sr = sums[s], srr = sums[S + s], se = sums[2 * S + t], see = sums[3 * S + t], sre = sums[4 * S + s * S + t];
  const double k10 = 10.0 / log(10.0);
  SnrTerm o;
  if (mode == SNR_ZEROMEAN) {
    const double D = sre - sr * se / L, Er = srr - sr * sr / L, Ee = see - se * se / L;
    const double te = Er + kSnrEps, k = 2.0 / te - Er / (te * te);
    const double P = D * D * Er / (te * te), N = Ee - D * D * k + kSnrEps, q = P / N + kSnrEps;
    o.loss = -k10 * log(q);
    const double g = -k10 / q;
    o.a = -g * 2.0 * P / (N * N);
    o.b = g * (2.0 * D * Er / (te * te * N) + 2.0 * D * k * P / (N * N));
    o.c = -(o.a * se + o.b * sr) / L;
  } else {
    const double M = srr * see - sre * sre;
    o.loss = -k10 * log(sre * sre / M);
    o.a = k10 * 2.0 * srr / M;
    o.b = -k10 * (2.0 / sre + 2.0 * sre / M);
    o.c = 0.0;
  }
  return o;
}

// one workgroup of 64 per utterance: sums[b][v] = the chunk partials in chunk order, then pair[b][s][t]
__global__ __launch_bounds__(64) void pair_sisnr_finish_kernel(const double* __restrict__ part, double* __restrict__ sums,
                                                               double* __restrict__ pair, int S, int nchunk, double L, int mode) {
  __shared__ double sh[snr_nv(kMaxSpk)];
  const int b = blockIdx.x, NV = snr_nv(S);
  if ((int)threadIdx.x < NV) {
    double s = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) s += part[((long)b * nchunk + ch) * NV + threadIdx.x];
    sh[threadIdx.x] = s;
    sums[(long)b * NV + threadIdx.x] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < S * S)
    pair[(long)b * S * S + threadIdx.x] = snr_term(sh, S, threadIdx.x / S, threadIdx.x % S, L, mode).loss;
}

template <int S>
__global__ __launch_bounds__(kThreads) void pair_sisnr_bwd_kernel(
    const float* __restrict__ est, const float* __restrict__ ref, const double* __restrict__ sums,
    const int64_t* __restrict__ perm_index, const float* __restrict__ cot, float* __restrict__ dest, int B, long L, int mode) {
  __shared__ double co[kMaxSpk][3];
  const int b = blockIdx.y;
  int perm[kMaxSpk], inv[kMaxSpk];
  perm_of(S, perm_index[b], perm);
  inverse_of<S>(perm, inv);
  if ((int)threadIdx.x < S) {
    const int t = threadIdx.x;
    const SnrTerm o = snr_term(sums + (long)b * snr_nv(S), S, inv[t], t, (double)L, mode);
    const double w = (double)cot[b] / S;
    co[t][0] = w * o.a; co[t][1] = w * o.b; co[t][2] = w * o.c;
  }
  __syncthreads();
  const long i0 = (long)blockIdx.x * kChunk, i1 = min(L, i0 + (long)kChunk);
  for (long i = i0 + threadIdx.x; i < i1; i += kThreads) {
    double r[S];
#pragma unroll
    for (int s = 0; s < S; ++s) r[s] = ref[((long)s * B + b) * L + i];
#pragma unroll
    for (int t = 0; t < S; ++t) {
      const long at = ((long)t * B + b) * L + i;
      double rs = 0.0;
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (s == inv[t]) rs = r[s];
      dest[at] = (float)(co[t][0] * (double)est[at] + co[t][1] * rs + co[t][2]);
    }
  }
}

// ---- permutation pick ---------------------------------------------------------------------------------------------------
// loss[b] = min over the permutations, itertools order, first minimum, of sum_s pair[b, s, perm[s]] / S; forced != NULL:
// that permutation only
__global__ __launch_bounds__(64) void pit_pick_kernel(const double* __restrict__ pair, const int64_t* __restrict__ forced,
                                                      float* __restrict__ loss, int64_t* __restrict__ perm_index, int B, int S) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int nperm = S == 1 ? 1 : (S == 2 ? 2 : 6);
  const double* p = pair + (long)b * S * S;
  double best = 0.0;
  long arg = 0;
  const long k0 = forced ? min(max((long)forced[b], 0L), (long)nperm - 1) : 0, k1 = forced ? k0 + 1 : nperm;
  for (long k = k0; k < k1; ++k) {
    int perm[kMaxSpk];
    perm_of(S, k, perm);
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += p[s * S + perm[s]];
    v /= S;
    if (k == k0 || v < best) { best = v; arg = k; }
  }
  loss[b] = (float)best;
  perm_index[b] = arg;
}

inline int chunks_of(long n) { return (int)((n + kChunk - 1) / kChunk); }
inline bool bad_pair_shape(long n, int nchunk) { return nchunk != chunks_of(n); }

// launches kernel<S> for S = 1, 2, 3 (the callers have refused every other S)
#define ENH_LAUNCH_S(kernel, S, grid, st, ...)                                                         \
  do {                                                                                                 \
    if ((S) == 1) hipLaunchKernelGGL(kernel<1>, grid, dim3(kThreads), 0, st, __VA_ARGS__);             \
    if ((S) == 2) hipLaunchKernelGGL(kernel<2>, grid, dim3(kThreads), 0, st, __VA_ARGS__);             \
    if ((S) == 3) hipLaunchKernelGGL(kernel<3>, grid, dim3(kThreads), 0, st, __VA_ARGS__);             \
  } while (0)

}  // namespace

extern "C" {

int eamd_istft_ola(const float* frames, const float* window, float* wav, int B, int T, int n_fft, int hop, int center, int length,
                   void* stream) {
  if (!frames || !window || !wav) return EAMD_EINVAL;
  if (B < 1 || T < 1 || n_fft < 1 || hop < 1 || length < 1) return EAMD_EINVAL;
  if (n_fft > 16 * hop || B > 65535) return EAMD_EUNSUPPORTED;
  const long full = (long)hop * (T - 1) + n_fft;
  if ((long)B * full > 0x7fffffffL || (long)B * length > 0x7fffffffL) return EAMD_EUNSUPPORTED;
  const int pad = center ? n_fft / 2 : 0;
  const int siglen = (int)std::min<long>(length, full - pad);
  if (siglen < 1) return EAMD_EINVAL;
  hipLaunchKernelGGL(istft_ola_kernel, dim3((length + kThreads - 1) / kThreads, B), dim3(kThreads), 0, (hipStream_t)stream, frames,
                     window, wav, T, n_fft, hop, pad, siglen, length);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_istft_ola_bwd(const float* dwav, const float* window, float* g, int B, int T, int n_fft, int hop, int center, int length,
                       int rows_per_utt, void* stream) {
  if (!dwav || !window || !g) return EAMD_EINVAL;
  if (B < 1 || T < 1 || n_fft < 1 || hop < 1 || length < 1) return EAMD_EINVAL;
  if (n_fft > 16 * hop) return EAMD_EUNSUPPORTED;
  const long full = (long)hop * (T - 1) + n_fft;
  if ((long)rows_per_utt * hop < full) return EAMD_EINVAL;
  const long ldg = (long)rows_per_utt * hop, total = (long)B * ldg + n_fft;
  if (total > 0x7fffffffL || (long)B * length > 0x7fffffffL) return EAMD_EUNSUPPORTED;
  const int pad = center ? n_fft / 2 : 0;
  const int siglen = (int)std::min<long>(length, full - pad);
  if (siglen < 1) return EAMD_EINVAL;
  hipLaunchKernelGGL(istft_ola_bwd_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     (hipStream_t)stream, dwav, window, g, B, T, n_fft, hop, pad, siglen, length, ldg, total);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_enh_mask_apply(const float* logits, const float* X, float* mask, float* P, int S, int64_t Bn, int act, void* stream) {
  if (!logits || (!mask && !P) || (P && !X)) return EAMD_EINVAL;
  if (S < 1 || Bn < 1 || act < ENH_ACT_SIGMOID || act > ENH_ACT_NONE) return EAMD_EINVAL;
  const unsigned grid = (unsigned)std::min<int64_t>((Bn + kThreads - 1) / kThreads, 2048);
  hipLaunchKernelGGL(mask_apply_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, logits, (const float2*)X, mask,
                     (float2*)P, S, (long)Bn, act);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_enh_mask_apply_bwd(const float* logits, const float* X, const float* gmask, const float* gP, float* dlogits, int S,
                            int64_t Bn, int act, void* stream) {
  if (!logits || !dlogits || (!gmask && !gP) || (gP && !X)) return EAMD_EINVAL;
  if (S < 1 || Bn < 1 || act < ENH_ACT_SIGMOID || act > ENH_ACT_NONE) return EAMD_EINVAL;
  const unsigned grid = (unsigned)std::min<int64_t>((Bn + kThreads - 1) / kThreads, 2048);
  hipLaunchKernelGGL(mask_apply_bwd_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, logits, (const float2*)X, gmask,
                     (const float2*)gP, dlogits, S, (long)Bn, act);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

static int check_pair_tf(const float* est, const float* ref, const float* mix, int S, int B, int64_t n, int mode, int label,
                         int act) {
  if (!est || !ref) return EAMD_EINVAL;
  if (mode < MODE_MASK || mode > MODE_REAL || B < 1 || n < 1) return EAMD_EINVAL;
  if (mode == MODE_MASK && (!mix || label < IBM || label > PSM2 || act < ENH_ACT_SIGMOID || act > ENH_ACT_NONE)) return EAMD_EINVAL;
  if (S < 1 || S > kMaxSpk || B > 65535) return EAMD_EUNSUPPORTED;
  return EAMD_OK;
}

int eamd_enh_pair_tf(const float* est, const float* ref, const float* mix, double* pair, void* workspace, int S, int B, int64_t n,
                     int nchunk, int mode, int label, int act, void* stream) {
  if (!pair || !workspace) return EAMD_EINVAL;
  if (const int rc = check_pair_tf(est, ref, mix, S, B, n, mode, label, act)) return rc;
  if (bad_pair_shape(n, nchunk)) return EAMD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nchunk, B);
  double* part = (double*)workspace;
  const float2* mx = (const float2*)mix;
  ENH_LAUNCH_S(pair_tf_kernel, S, grid, st, est, ref, mx, part, B, (long)n, nchunk, mode, label, act);
  hipLaunchKernelGGL(pair_tf_finish_kernel, dim3((B * S * S + kThreads - 1) / kThreads), dim3(kThreads), 0, st, part, pair, B, S * S,
                     nchunk, 1.0 / (double)n);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_enh_pair_tf_bwd(const float* est, const float* ref, const float* mix, const int64_t* perm_index, const float* cot,
                         float* dest, int S, int B, int64_t n, int mode, int label, int act, void* stream) {
  if (!perm_index || !cot || !dest) return EAMD_EINVAL;
  if (const int rc = check_pair_tf(est, ref, mix, S, B, n, mode, label, act)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(chunks_of(n), B);
  const float2* mx = (const float2*)mix;
  ENH_LAUNCH_S(pair_tf_bwd_kernel, S, grid, st, est, ref, mx, perm_index, cot, dest, B, (long)n, mode, label, act);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

static int check_sisnr(const float* est, const float* ref, int S, int B, int64_t L, int mode) {
  if (!est || !ref) return EAMD_EINVAL;
  if ((mode != SNR_ZEROMEAN && mode != SNR_L2NORM) || B < 1 || L < 1) return EAMD_EINVAL;
  if (S < 1 || S > kMaxSpk || B > 65535) return EAMD_EUNSUPPORTED;
  return EAMD_OK;
}

int eamd_enh_pair_sisnr(const float* est, const float* ref, double* pair, double* sums, void* workspace, int S, int B, int64_t L,
                        int nchunk, int mode, void* stream) {
  if (!pair || !sums || !workspace) return EAMD_EINVAL;
  if (const int rc = check_sisnr(est, ref, S, B, L, mode)) return rc;
  if (bad_pair_shape(L, nchunk)) return EAMD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nchunk, B);
  double* part = (double*)workspace;
  ENH_LAUNCH_S(pair_sisnr_kernel, S, grid, st, est, ref, part, B, (long)L, nchunk);
  hipLaunchKernelGGL(pair_sisnr_finish_kernel, dim3(B), dim3(64), 0, st, part, sums, pair, S, nchunk, (double)L, mode);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_enh_pair_sisnr_bwd(const float* est, const float* ref, const double* sums, const int64_t* perm_index, const float* cot,
                            float* dest, int S, int B, int64_t L, int mode, void* stream) {
  if (!sums || !perm_index || !cot || !dest) return EAMD_EINVAL;
  if (const int rc = check_sisnr(est, ref, S, B, L, mode)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(chunks_of(L), B);
  ENH_LAUNCH_S(pair_sisnr_bwd_kernel, S, grid, st, est, ref, sums, perm_index, cot, dest, B, (long)L, mode);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_enh_pit_pick(const double* pair, const int64_t* forced, float* loss, int64_t* perm_index, int B, int S, void* stream) {
  if (!pair || !loss || !perm_index) return EAMD_EINVAL;
  if (B < 1) return EAMD_EINVAL;
  if (S < 1 || S > kMaxSpk) return EAMD_EUNSUPPORTED;
  hipLaunchKernelGGL(pit_pick_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, pair, forced, loss, perm_index, B, S);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
