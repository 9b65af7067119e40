// espnet1 feature transform between the beamformer and the RNN encoder, in both directions, and the input gradient of
// the VGG front-end's first convolution: what lets the ASR loss reach the beamformer's mask estimator
// (E2E(use_frontend=True), Ochiai et al. 2017).
// reference: espnet/nets/pytorch_backend/frontends/feature_transform.py:45-75 (FeatureTransform.forward), :123-132
//            (LogMel: power x melmat, + 1e-20, natural log, padded frames zeroed), :180-190 (GlobalMVN), :213-247
//            (utterance_mvn); rnn/encoders.py:184,203 (VGG2L conv1_1).
// These are NOT the espnet2 layers of features.hip (clamp 1e-10, statistics over the valid frames only): espnet1's
// `masked_fill` calls are not in place, so padded frames carry bias*scale into the utterance mean and leave non-zero.
//
// All fp32, no atomics: every output element is written by one thread from a fixed summation order.
//   ft_logmel_fwd / _bwd   one wave per frame (lanes along mel filters / frequency bins), power row staged in LDS.
//                          The backward RECOMPUTES mel + 1e-20 from the spectrum (it reads the row anyway for the
//                          2*(re, im) factor): exp() of the saved log would carry |log| * 2^-24 of relative error,
//                          3e-6 at the floor log(1e-20) = -46.
//   ft_mvn_fwd / _bwd      column sums over T: one workgroup per (utterance, 64 features), 16 sub-rows of 64 lanes;
//                          then one element-wise sweep.
//   conv3x3_c1_bwd_x       one workgroup marches over a segment of frames: the dy row [F, C] is staged in LDS by
//                          coalesced 16-byte loads, thread (f, i) folds the C channels into the three taps j of kernel
//                          row i, a ring of three such rows gives dx.  Every dy row is loaded once per segment (the
//                          two halo rows of a 32-frame segment are its neighbours' rows, 6% more requests).
#include "common.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr float FT_EPS = 1e-20f;          // feature_transform.py:129
constexpr size_t FT_LDS_MAX = 64 * 1024;

inline int ft_grid_for(long n) {
  long g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}

// power row of one frame into LDS, then the mel sum of filter m over its bin range
__device__ __forceinline__ void ft_power_row(const float2* __restrict__ row, float* __restrict__ p, int F, int lane) {
  for (int f = lane; f < F; f += 64) { const float2 c = row[f]; p[f] = c.x * c.x + c.y * c.y; }
}
__device__ __forceinline__ float ft_mel_sum(const float* __restrict__ p, const float* __restrict__ melmat, int lo, int hi,
                                            int F, int M, int m) {
  lo = max(lo, 0); hi = min(hi, F);
  float acc = 0.f;
  for (int f = lo; f < hi; ++f) acc += p[f] * melmat[(long)f * M + m];
  return acc;
}

__global__ __launch_bounds__(256) void ft_logmel_fwd_kernel(const float* __restrict__ spec, const float* __restrict__ melmat,
                                                            const int* __restrict__ lo, const int* __restrict__ hi,
                                                            const int* __restrict__ lens, float* __restrict__ out, int B,
                                                            int T, int F, int M) {
  extern __shared__ float ft_lds[];   // [4][F]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long fr = (long)blockIdx.x * 4 + wave;
  if (fr >= (long)B * T) return;
  const int b = fr / T, t = fr % T;
  float* o = out + fr * M;
  if (lens && t >= lens[b]) {
    for (int m = lane; m < M; m += 64) o[m] = 0.f;
    return;
  }
  float* p = ft_lds + wave * F;
  ft_power_row(reinterpret_cast<const float2*>(spec + fr * 2 * F), p, F, lane);
  __builtin_amdgcn_wave_barrier();
  for (int m = lane; m < M; m += 64) o[m] = logf(ft_mel_sum(p, melmat, lo[m], hi[m], F, M, m) + FT_EPS);
}

// g_spec[b,t,f] = 2 (re, im) sum_{m in [mlo[f], mhi[f])} melmat[f,m] g[b,t,m] / (mel[b,t,m] + 1e-20); 0 for padded frames
__global__ __launch_bounds__(256) void ft_logmel_bwd_kernel(const float* __restrict__ spec, const float* __restrict__ g,
                                                            const float* __restrict__ melmat, const int* __restrict__ lo,
                                                            const int* __restrict__ hi, const int* __restrict__ mlo,
                                                            const int* __restrict__ mhi, const int* __restrict__ lens,
                                                            float* __restrict__ gspec, int B, int T, int F, int M) {
  extern __shared__ float ft_lds[];   // [4][F + M]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long fr = (long)blockIdx.x * 4 + wave;
  if (fr >= (long)B * T) return;
  const int b = fr / T, t = fr % T;
  float2* o = reinterpret_cast<float2*>(gspec + fr * 2 * F);
  if (lens && t >= lens[b]) {
    for (int f = lane; f < F; f += 64) o[f] = make_float2(0.f, 0.f);
    return;
  }
  const float2* row = reinterpret_cast<const float2*>(spec + fr * 2 * F);
  float* p = ft_lds + wave * (F + M);
  float* r = p + F;
  ft_power_row(row, p, F, lane);
  __builtin_amdgcn_wave_barrier();
  for (int m = lane; m < M; m += 64) r[m] = g[fr * M + m] / (ft_mel_sum(p, melmat, lo[m], hi[m], F, M, m) + FT_EPS);
  __builtin_amdgcn_wave_barrier();
  for (int f = lane; f < F; f += 64) {
    const float2 c = row[f];
    float s = 0.f;
    const int m0 = max(mlo[f], 0), m1 = min(mhi[f], M);
    for (int m = m0; m < m1; ++m) s += melmat[(long)f * M + m] * r[m];
    // a bin without power contributes nothing, whatever its filters' quotients are
    o[f] = (c.x == 0.f && c.y == 0.f) ? make_float2(0.f, 0.f) : make_float2(2.f * c.x * s, 2.f * c.y * s);
  }
}

constexpr int FT_SUB = 16;                // sub-rows of 64 lanes that share a column sum (workgroup of 1024)
// the 16 partial sums of a column in a fixed pairwise order
__device__ __forceinline__ float ft_col_sum(const float (*red)[64], int lane) {
  float s[FT_SUB];
#pragma unroll
  for (int k = 0; k < FT_SUB; ++k) s[k] = red[k][lane];
#pragma unroll
  for (int w = FT_SUB / 2; w >= 1; w >>= 1)
#pragma unroll
    for (int k = 0; k < w; ++k) s[k] = s[2 * k] + s[2 * k + 1];
  return s[0];
}

__device__ __forceinline__ float ft_gmvn(float v, const float* bias, const float* scale, int m) {
  if (bias) { v += bias[m]; v *= scale[m]; }       // x += bias; x *= scale: two roundings, as the reference
  return v;
}

// mean[b,m] = sum over ALL T frames of z / len[b]  (z = (x + bias) * scale, padded frames included);
// var[b,m] (optional) = sum over all T frames of (z - mean)^2 / len[b], clamped at eps
__global__ __launch_bounds__(1024) void ft_mvn_stats_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                           const float* __restrict__ bias, const float* __restrict__ scale,
                                                           float* __restrict__ mean, float* __restrict__ var, float eps,
                                                           int T, int M) {
  __shared__ float red[FT_SUB][64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  const int m = blockIdx.y * 64 + lane;
  const float len = (float)lens[b];
  float s = 0.f;
  if (m < M) for (int t = sub; t < T; t += FT_SUB) s += ft_gmvn(x[((long)b * T + t) * M + m], bias, scale, m);
  red[sub][lane] = s;
  __syncthreads();
  const float mu = ft_col_sum(red, lane) / len;
  __syncthreads();
  if (sub == 0 && m < M) mean[(long)b * M + m] = mu;
  if (!var) return;
  float q = 0.f;
  if (m < M) for (int t = sub; t < T; t += FT_SUB) { const float d = ft_gmvn(x[((long)b * T + t) * M + m], bias, scale, m) - mu; q += d * d; }
  red[sub][lane] = q;
  __syncthreads();
  if (sub == 0 && m < M)
    var[(long)b * M + m] = fmaxf(ft_col_sum(red, lane) / len, eps);
}

// feature_transform.py:230-247: without norm_vars the mean-subtracted copy comes back whatever norm_means says; with
// norm_vars x (mean-subtracted only under norm_means) is divided by sqrt(var)
__global__ void ft_mvn_apply_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ bias,
                                    const float* __restrict__ scale, const float* __restrict__ mean,
                                    const float* __restrict__ var, int norm_means, int B, int T, int M) {
  const long n = (long)B * T * M;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int m = i % M; const int b = i / ((long)T * M);
    float v = ft_gmvn(x[i], bias, scale, m);
    if (mean) {
      if (!var) v -= mean[(long)b * M + m];
      else v = (norm_means ? v - mean[(long)b * M + m] : v) / sqrtf(var[(long)b * M + m]);
    }
    y[i] = v;
  }
}

// colsum[b,m] = sum over all T frames of gy / len[b]
__global__ __launch_bounds__(1024) void ft_mvn_bwd_stats_kernel(const float* __restrict__ gy, const int* __restrict__ lens,
                                                               float* __restrict__ cs, int T, int M) {
  __shared__ float red[FT_SUB][64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  const int m = blockIdx.y * 64 + lane;
  float s = 0.f;
  if (m < M) for (int t = sub; t < T; t += FT_SUB) s += gy[((long)b * T + t) * M + m];
  red[sub][lane] = s;
  __syncthreads();
  if (sub == 0 && m < M)
    cs[(long)b * M + m] = ft_col_sum(red, lane) / (float)lens[b];
}
__global__ void ft_mvn_bwd_apply_kernel(const float* __restrict__ gy, float* __restrict__ gx, const float* __restrict__ scale,
                                        const float* __restrict__ cs, int B, int T, int M) {
  const long n = (long)B * T * M;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int m = i % M; const int b = i / ((long)T * M);
    float v = gy[i];
    if (cs) v -= cs[(long)b * M + m];
    if (scale) v *= scale[m];
    gx[i] = v;
  }
}

// ---- input gradient of the 1 -> C channel 3x3 convolution (stride 1, padding 1) ---------------------------------------
constexpr int CBX_SEG = 32;               // frames per workgroup

__device__ __forceinline__ float4 cbx_load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 cbx_load4(const unsigned short* p) {
  const ushort4 v = *reinterpret_cast<const ushort4*>(p);
  return make_float4(__uint_as_float((unsigned)v.x << 16), __uint_as_float((unsigned)v.y << 16),
                     __uint_as_float((unsigned)v.z << 16), __uint_as_float((unsigned)v.w << 16));
}

// LDS: wl [3][C + 1][4] (kernel row i, channel, tap j; fourth float unused; the extra slot shifts each kernel row by four
// banks: threads of one wave read three rows at once) | row [F][C + 4] | q [3][9][F]
template <typename DY>
__global__ __launch_bounds__(256) void conv3x3_c1_bwd_x_kernel(const DY* __restrict__ dy, const float* __restrict__ w,
                                                               float* __restrict__ dx, int T, int F, int C, int nseg) {
  extern __shared__ float4 cbx_lds4[];
  float* wl = reinterpret_cast<float*>(cbx_lds4);
  const int WS = (C + 1) * 4;
  float* rowb = wl + 3 * WS;
  const int CS = C + 4;
  float* q = rowb + (long)F * CS;
  const int b = blockIdx.x / nseg, t0 = (blockIdx.x % nseg) * CBX_SEG;
  const int t1 = min(t0 + CBX_SEG, T);    // this workgroup writes dx rows [t0, t1)
  for (int k = threadIdx.x; k < 3 * C * 4; k += blockDim.x) {
    const int j = k & 3, c = (k >> 2) % C, i = (k >> 2) / C;
    wl[i * WS + c * 4 + j] = j < 3 ? w[c * 9 + i * 3 + j] : 0.f;
  }
  const int rowlen4 = F * C / 4, c4 = C / 4;
  for (int tp = max(t0 - 1, 0); tp <= min(t1, T - 1); ++tp) {
    const DY* src = dy + ((long)b * T + tp) * F * C;
    for (int k = threadIdx.x; k < rowlen4; k += blockDim.x) {
      const int f = k / c4, c = (k % c4) * 4;
      *reinterpret_cast<float4*>(rowb + (long)f * CS + c) = cbx_load4(src + (long)k * 4);
    }
    __syncthreads();
    float* qr = q + (tp % 3) * 9 * F;
    for (int k = threadIdx.x; k < 3 * F; k += blockDim.x) {
      const int f = k / 3, i = k % 3;
      const float4* d4 = reinterpret_cast<const float4*>(rowb + (long)f * CS);
      const float4* w4 = reinterpret_cast<const float4*>(wl + i * WS);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      for (int c = 0; c < c4; ++c) {
        const float4 d = d4[c];
        const float4 wa = w4[4 * c], wb = w4[4 * c + 1], wc = w4[4 * c + 2], wd = w4[4 * c + 3];
        a0 += d.x * wa.x; a1 += d.x * wa.y; a2 += d.x * wa.z;
        a0 += d.y * wb.x; a1 += d.y * wb.y; a2 += d.y * wb.z;
        a0 += d.z * wc.x; a1 += d.z * wc.y; a2 += d.z * wc.z;
        a0 += d.w * wd.x; a1 += d.w * wd.y; a2 += d.w * wd.z;
      }
      qr[(i * 3 + 0) * F + f] = a0; qr[(i * 3 + 1) * F + f] = a1; qr[(i * 3 + 2) * F + f] = a2;
    }
    __syncthreads();
    // dx[t,f] = sum_{i,j} q_ij[t+1-i, f+1-j]: row t = tp - 1 is complete now; the utterance's last row too when tp is it
    for (int t = max(tp - 1, t0); t <= tp && t < t1; ++t) {
      if (t == tp && tp != T - 1) break;
      for (int f = threadIdx.x; f < F; f += blockDim.x) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int tq = t + 1 - i;
          if (tq < 0 || tq >= T) continue;
          const float* qq = q + (tq % 3) * 9 * F + i * 3 * F;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const int fq = f + 1 - j;
            if (fq >= 0 && fq < F) s += qq[j * F + fq];
          }
        }
        dx[((long)b * T + t) * F + f] = s;
      }
    }
  }
}

inline size_t cbx_lds_bytes(int F, int C) { return ((size_t)3 * (C + 1) * 4 + (size_t)F * (C + 4) + (size_t)27 * F) * sizeof(float); }

}  // namespace

extern "C" {

int eamd_ft_logmel_fwd(const float* spec, const float* melmat, const int32_t* lo, const int32_t* hi, const int32_t* lens,
                       float* out, int B, int T, int F, int M, void* stream) {
  if (!spec || !melmat || !lo || !hi || !lens || !out || B <= 0 || T <= 0 || F <= 0 || M <= 0) return EAMD_EINVAL;
  if ((uintptr_t)spec & 7) return EAMD_EINVAL;
  const size_t sm = (size_t)4 * F * sizeof(float);
  if (sm > FT_LDS_MAX) return EAMD_EUNSUPPORTED;
  hipLaunchKernelGGL(ft_logmel_fwd_kernel, dim3((unsigned)(((long)B * T + 3) / 4)), dim3(256), sm, (hipStream_t)stream, spec,
                     melmat, lo, hi, lens, out, B, T, F, M);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_ft_logmel_bwd(const float* spec, const float* g, const float* melmat, const int32_t* lo, const int32_t* hi,
                       const int32_t* mlo, const int32_t* mhi, const int32_t* lens, float* gspec, int B, int T, int F, int M,
                       void* stream) {
  if (!spec || !g || !melmat || !lo || !hi || !mlo || !mhi || !lens || !gspec || B <= 0 || T <= 0 || F <= 0 || M <= 0)
    return EAMD_EINVAL;
  if (((uintptr_t)spec | (uintptr_t)gspec) & 7) return EAMD_EINVAL;
  const size_t sm = (size_t)4 * ((size_t)F + M) * sizeof(float);
  if (sm > FT_LDS_MAX) return EAMD_EUNSUPPORTED;
  hipLaunchKernelGGL(ft_logmel_bwd_kernel, dim3((unsigned)(((long)B * T + 3) / 4)), dim3(256), sm, (hipStream_t)stream, spec,
                     g, melmat, lo, hi, mlo, mhi, lens, gspec, B, T, F, M);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_ft_mvn_fwd(const float* x, float* y, const int32_t* lens, const float* bias, const float* scale, float* workspace,
                    int apply_utt, int norm_means, int norm_vars, float eps, int B, int T, int M, void* stream) {
  if (!x || !y || B <= 0 || T <= 0 || M <= 0 || (bias == nullptr) != (scale == nullptr)) return EAMD_EINVAL;
  if (apply_utt && (!lens || !workspace)) return EAMD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* mean = apply_utt ? workspace : nullptr;
  float* var = apply_utt && norm_vars ? workspace + (long)B * M : nullptr;
  if (apply_utt) {
    hipLaunchKernelGGL(ft_mvn_stats_kernel, dim3(B, (M + 63) / 64), dim3(64 * FT_SUB), 0, s, x, lens, bias, scale, mean, var, eps, T, M);
    EAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ft_mvn_apply_kernel, dim3(ft_grid_for((long)B * T * M)), dim3(256), 0, s, x, y, bias, scale,
                     (const float*)mean, (const float*)var, norm_means, B, T, M);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_ft_mvn_bwd(const float* gy, float* gx, const int32_t* lens, const float* scale, float* workspace, int apply_utt,
                    int B, int T, int M, void* stream) {
  if (!gy || !gx || B <= 0 || T <= 0 || M <= 0) return EAMD_EINVAL;
  if (apply_utt && (!lens || !workspace)) return EAMD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (apply_utt) {
    hipLaunchKernelGGL(ft_mvn_bwd_stats_kernel, dim3(B, (M + 63) / 64), dim3(64 * FT_SUB), 0, s, gy, lens, workspace, T, M);
    EAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ft_mvn_bwd_apply_kernel, dim3(ft_grid_for((long)B * T * M)), dim3(256), 0, s, gy, gx, scale,
                     (const float*)(apply_utt ? workspace : nullptr), B, T, M);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_conv3x3_c1_bwd_x(const void* dy, const float* w, float* dx, int B, int T, int F, int C, int dy_bf16, void* stream) {
  if (!dy || !w || !dx || B <= 0 || T <= 0 || F <= 0 || C <= 0) return EAMD_EINVAL;
  if (C % 4 != 0 || cbx_lds_bytes(F, C) > FT_LDS_MAX) return EAMD_EUNSUPPORTED;   // 16-byte channel groups; one dy row in LDS
  if ((uintptr_t)dy & (dy_bf16 ? 7 : 15)) return EAMD_EINVAL;
  const int nseg = (T + CBX_SEG - 1) / CBX_SEG;
  if ((long)B * nseg > 0x7fffffffL) return EAMD_EUNSUPPORTED;
  const dim3 grid((unsigned)((long)B * nseg));
  if (dy_bf16)
    hipLaunchKernelGGL(conv3x3_c1_bwd_x_kernel<unsigned short>, grid, dim3(256), cbx_lds_bytes(F, C), (hipStream_t)stream,
                       (const unsigned short*)dy, w, dx, T, F, C, nseg);
  else
    hipLaunchKernelGGL(conv3x3_c1_bwd_x_kernel<float>, grid, dim3(256), cbx_lds_bytes(F, C), (hipStream_t)stream,
                       (const float*)dy, w, dx, T, F, C, nseg);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
