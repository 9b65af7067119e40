// WPE dereverberation (weighted prediction error, Nakatani et al. 2010; the algorithm the reference's DNN_WPE,
// espnet/nets/pytorch_backend/frontends/dnn_wpe.py, delegates to the pytorch_wpe package), forward and backward, on
// interleaved (re, im) fp32 spectra y [B, T, C, F, 2] exactly as Stft.forward lays them out.
//
// Per utterance b of n = lens[b] frames and bin f, with K taps, delay D, N = C K unknowns per output channel and the
// stacked history  h_t[k C + c] = y[t - D - k, c]  (zero before the first frame), t0 = D + K - 1:
//   R = sum_{t0 <= t < n} w_t h_t h_t^H,   P = sum_{t0 <= t < n} w_t h_t y_t^H,   G = R^-1 P,   x_t = y_t - G^H h_t.
// The sums stop at the utterance's own length (the padded frames of a batch carry weight 1 / eps).
//
// Precision: y, power, G and x are fp32 in memory; every product, every sum and the whole solve are fp64 (the espnet2
// twin of DNN_WPE computes WPE in double for the same reason: R is a sum of |y|^2 / power over time with a condition
// number of 1e3..1e5).  bf16 is never used here.
//
// The correlation pass, the in-LDS solve and the filter pass live in wpe_kernels.h, which wpd.hip shares.
//
//   corr     one workgroup per (b, 32-bin tile, group of 8 tasks, time chunk).  h_t is never written to memory: the
//            workgroup stages a window of TS + K - 1 frames of the tile (and the TS right-hand frames and weights) in LDS,
//            f fastest - 256 contiguous bytes per (frame, channel) row - and every half-wave (32 lanes = the 32 bins)
//            accumulates one 4 x 4 tile of [R | P] in registers: lane l reads float2 l of a row, conflict-free.  Only the
//            tiles on or above R's diagonal are formed.  Chunk partials go to a workspace [chunk][b][f][N][N + C]; the
//            solve adds them in chunk order (no atomics, the same bits on every launch).
//   solve    one workgroup per (b, f): the lower triangle of R in LDS (rows padded by one element), right-looking LDL^H
//            without pivoting, the forward substitution of the C right-hand sides fused into the elimination, then the
//            back substitution.  A pivot that is zero, negative or not finite takes reciprocal 0 (a singular bin gives a
//            finite, meaningless answer, never NaN - the convention of mvdr_kernel).  The factor is KEPT for the backward
//            (fac [B,F,N,N] complex double: L d below the diagonal, 1 / d on it), not recomputed: the correlation pass is
//            the expensive one.
//   filter   x_t = y_t - G^H h_t; thread = (bin, output channel), 8 frames in registers, the window in LDS as above,
//            G [B,N,C,F] read along f.  Exact zeros for t >= n.
//   backward gG = -sum_{t < n} h_t gx_t^H (the corr pass, weight -1, no R), Z = R^-1 gG (the solve from the kept factor),
//            gw_t = Re(h_t^H Z x_t) (the filter pass with Z for G, then a dot with x_t summed over channels in a fixed
//            order), gpower_t = -gw_t / power_t^2 where power_t > eps, else 0.
//   power    power[b,t,f] = mean_c |y|^2 sigmoid(z[0,b,c,t,f]) and its backward: one streaming kernel each.
//
// Complex cotangents follow PyTorch: g is the tensor with dL = Re sum conj(g) dv, stored (re, im) like the value.
#include "wpe_kernels.h"

namespace {

// IEEE division and libm's expf, as in beamformer.hip: the tests hold these kernels to the fp32 reference's own error
__device__ __forceinline__ float wpe_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float wpe_dsigmoid(float x) {
  const float e = expf(-fabsf(x)), s = 1.0f / (1.0f + e);
  return e * s * s;
}

// FACTOR: part [chunk][b][f][N][N + C] as the corr pass wrote it; factors R, writes fac (unless NULL) and G = R^-1 P.
// !FACTOR: part [chunk][b][f][N][C]; reads fac and writes G = R^-1 (sum of the chunks).  G [B][N][C][F] fp32.
template <bool FACTOR>
__global__ __launch_bounds__(kSolveThreads) void wpe_solve_kernel(const double2* __restrict__ part, double2* __restrict__ fac,
                                                                  float2* __restrict__ G, int B, int F, int N, int C, int nchunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lda = N + 1;                                          // padded: a column walk moves 4 banks per row
  double2* A = reinterpret_cast<double2*>(smem);                  // [N][lda], lower triangle: L d (unscaled columns)
  double2* Z = A + (long)N * lda;                                 // [N][C]
  double* dinv = reinterpret_cast<double*>(Z + (long)N * C);      // [N]
  const long bf = blockIdx.x;
  const int b = (int)(bf / F), f = (int)(bf % F);
  const int ld = FACTOR ? N + C : C, pc0 = FACTOR ? N : 0;
  const long cstride = (long)B * F * N * ld;                      // between chunks
  const double2* p0 = part + bf * N * ld;
  const int tid = threadIdx.x;
  if (FACTOR) {
    for (int idx = tid; idx < N * N; idx += kSolveThreads) {
      const int i = idx / N, j = idx % N;
      if (j < i) continue;
      double2 s = make_double2(0.0, 0.0);
      for (int ch = 0; ch < nchunk; ++ch) {                        // chunk order: the same bits on every launch
        const double2 v = p0[ch * cstride + (long)i * ld + j];
        s.x += v.x; s.y += v.y;
      }
      A[j * lda + i] = make_double2(s.x, i == j ? 0.0 : -s.y);      // R[j][i] = conj(R[i][j])
    }
  } else {
    load_factor(fac + bf * N * N, A, dinv, N, lda);
  }
  for (int idx = tid; idx < N * C; idx += kSolveThreads) {
    const int i = idx / C, c = idx % C;
    double2 s = make_double2(0.0, 0.0);
    for (int ch = 0; ch < nchunk; ++ch) {
      const double2 v = p0[ch * cstride + (long)i * ld + pc0 + c];
      s.x += v.x; s.y += v.y;
    }
    Z[idx] = s;
  }
  ldl_solve_lds<FACTOR>(A, Z, dinv, N, C, lda);
  for (int idx = tid; idx < N * C; idx += kSolveThreads) {
    const double2 z = Z[idx];
    G[((long)b * N * C + idx) * F + f] = make_float2((float)z.x, (float)z.y);
  }
  if (FACTOR && fac) store_factor(fac + bf * N * N, A, dinv, N, lda);
}

inline size_t solve_lds_bytes(int N, int C) { return ((size_t)N * (N + 1) + (size_t)N * C) * 16 + (size_t)N * 8; }

// ---------------------------------------------------------------------------------------------------------------------
// power from the mask, and its backward
// ---------------------------------------------------------------------------------------------------------------------
// power[b,t,f] = mean_c |y[b,t,c,f]|^2 m,  m = sigmoid(z[0,b,c,t,f]) for t < Tm, 0 for Tm <= t < T;  z == NULL: m = 1
__global__ __launch_bounds__(256) void wpe_power_kernel(const float2* __restrict__ y, const float* __restrict__ z,
                                                        float* __restrict__ power, int B, int T, int Tm, int C, int F) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (b, t, f), f fastest
  if (i >= (long)B * T * F) return;
  const int f = (int)(i % F), t = (int)((i / F) % T);
  const long b = i / ((long)F * T);
  float acc = 0.f;
  if (!z || t < Tm)
    for (int c = 0; c < C; ++c) {
      const float2 v = y[((b * T + t) * C + c) * F + f];
      const float p = v.x * v.x + v.y * v.y;
      acc += z ? p * wpe_sigmoid(z[((b * C + c) * Tm + t) * F + f]) : p;
    }
  power[i] = acc / (float)C;
}

__global__ __launch_bounds__(256) void wpe_power_bwd_kernel(const float2* __restrict__ y, const float* __restrict__ z,
                                                            const float* __restrict__ gpower, float* __restrict__ dz, int B,
                                                            int T, int Tm, int C, int F) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (b, c, t, f) over the Tm mask frames, f fastest
  if (i >= (long)B * C * Tm * F) return;
  const int f = (int)(i % F), t = (int)((i / F) % Tm), c = (int)((i / ((long)F * Tm)) % C);
  const long b = i / ((long)F * Tm * C);
  const float2 v = y[((b * T + t) * C + c) * F + f];
  dz[i] = gpower[(b * T + t) * F + f] * ((v.x * v.x + v.y * v.y) / (float)C) * wpe_dsigmoid(z[i]);
}

inline int bad_shape(int B, int T, int C, int F, int K, int delay) {
  if (B < 1 || T < 1 || C < 1 || F < 1 || K < 1 || delay < 0) return EAMD_EINVAL;
  if ((long)C * K > kMaxN) return EAMD_EUNSUPPORTED;
  return EAMD_OK;
}

template <bool FACTOR>
int launch_solve(const void* part, void* fac, float* G, int B, int F, int N, int C, int nchunk, hipStream_t st) {
  static const hipError_t attr_err = hipFuncSetAttribute(reinterpret_cast<const void*>(&wpe_solve_kernel<FACTOR>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (attr_err != hipSuccess) return (int)attr_err;
  hipLaunchKernelGGL(wpe_solve_kernel<FACTOR>, dim3((unsigned)((long)B * F)), dim3(kSolveThreads), solve_lds_bytes(N, C), st,
                     (const double2*)part, (double2*)fac, (float2*)G, B, F, N, C, nchunk);
  return EAMD_OK;
}

}  // namespace

extern "C" {

int eamd_wpe_power(const float* y, const float* z, float* power, int B, int T, int Tm, int C, int F, void* stream) {
  if (!y || !power) return EAMD_EINVAL;
  if (B < 1 || T < 1 || C < 1 || F < 1 || (z && (Tm < 1 || Tm > T))) return EAMD_EINVAL;
  const long total = (long)B * T * F;
  if ((total + 255) / 256 > 0x7fffffffL) return EAMD_EUNSUPPORTED;
  hipLaunchKernelGGL(wpe_power_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)y, z, power, B, T, Tm, C, F);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_wpe_power_bwd(const float* y, const float* z, const float* gpower, float* dz, int B, int T, int Tm, int C, int F,
                       void* stream) {
  if (!y || !z || !gpower || !dz) return EAMD_EINVAL;
  if (B < 1 || T < 1 || C < 1 || F < 1 || Tm < 1 || Tm > T) return EAMD_EINVAL;
  const long total = (long)B * C * Tm * F;
  if ((total + 255) / 256 > 0x7fffffffL) return EAMD_EUNSUPPORTED;
  hipLaunchKernelGGL(wpe_power_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)y, z, gpower, dz, B, T, Tm, C, F);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_wpe_taps(const float* y, const float* power, const int32_t* lens, float* G, double* fac, void* workspace, int B, int T,
                  int C, int F, int taps, int delay, float eps, int inverse_power, int nchunk, void* stream) {
  if (!y || !power || !G || !workspace) return EAMD_EINVAL;
  if (nchunk < 1 || nchunk > T) return EAMD_EINVAL;
  if (const int rc = bad_shape(B, T, C, F, taps, delay)) return rc;
  if ((long)B * F > 0x7fffffffL) return EAMD_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = launch_corr<false>(y, y, power, lens, workspace, B, T, C, F, taps, delay, eps, inverse_power ? 0 : 1, nchunk,
                                        st))
    return rc;
  if (const int rc = launch_solve<true>(workspace, fac, G, B, F, C * taps, C, nchunk, st)) return rc;
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_wpe_filter(const float* y, const float* G, const int32_t* lens, float* x, int B, int T, int C, int F, int taps, int delay,
                    void* stream) {
  if (!y || !G || !x) return EAMD_EINVAL;
  if (const int rc = bad_shape(B, T, C, F, taps, delay)) return rc;
  if (B > 65535 || ceil_div(T, 2) > 65535) return EAMD_EUNSUPPORTED;
  launch_filter<kWpeFilter>(y, G, lens, x, nullptr, nullptr, B, T, C, F, taps, delay, 0.f, 1, (hipStream_t)stream);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_wpe_bwd(const float* y, const float* x, const float* gx, const float* power, const int32_t* lens, const double* fac,
                 float* gpower, void* workspace, int B, int T, int C, int F, int taps, int delay, float eps, int inverse_power,
                 int nchunk, void* stream) {
  if (!y || !x || !gx || !power || !fac || !gpower || !workspace) return EAMD_EINVAL;
  if (nchunk < 1 || nchunk > T) return EAMD_EINVAL;
  if (const int rc = bad_shape(B, T, C, F, taps, delay)) return rc;
  if ((long)B * F > 0x7fffffffL || B > 65535 || ceil_div(T, 2) > 65535) return EAMD_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int N = C * taps;
  float* Z = (float*)((char*)workspace + (size_t)nchunk * B * F * N * C * 16);       // [B][N][C][F] complex fp32
  if (const int rc = launch_corr<false>(y, gx, nullptr, lens, workspace, B, T, C, F, taps, delay, eps, 2, nchunk, st)) return rc;
  if (const int rc = launch_solve<false>(workspace, (void*)fac, Z, B, F, N, C, nchunk, st)) return rc;
  launch_filter<kWpeBwd>(y, Z, lens, (float*)x, power, gpower, B, T, C, F, taps, delay, eps, inverse_power, st);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
