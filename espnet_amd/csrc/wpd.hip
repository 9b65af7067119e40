// WPD convolutional beamformer (weighted power minimisation distortionless response, Nakatani and Kinoshita, IEEE SPL 26,
// 2019; the reference's espnet2/enh/layers/conv_beamformer.py) and, with no taps and unit weights, the covariance of the
// MPDR beamformer, forward and backward, on interleaved (re, im) fp32 spectra y [B, T, C, F, 2].
//
// Per utterance b of n = lens[b] frames and bin f, with K = btaps >= 0, D = bdelay >= 1, N = (K + 1) C and the stacked
// vector  v_t[c] = y[t, c],  v_t[(k + 1) C + c] = y[t - D - k, c]  (zero before frame 0), t0 = D + K - 1:
//   Rf = sum_{t0 <= t < n} w_t v_t v_t^H          w_t = 1 / max(power_t, eps), or power_t as given, or 1
//   X = Rf^-1 E  (E = the first C columns of I_N),  M = X Phi,  tau = tr(M[:C]) + 1e-15,  h = M u / tau
//   e_t = h^H v_t  for t < n,  0 for t >= n
// The sums stop at the utterance's own length, as in wpe.hip.
//
// Precision: y, power, Phi, u, h and e are fp32 in memory; every product, every sum and the solve are fp64, and Rf, which
// the solve takes, stays fp64 in memory too: rounding it to fp32 would cost cond(Rf) * 6e-8 in h.  bf16 is never used.
//
// The correlation pass, the LDL^H solve and the filter pass are those of wpe.hip (wpe_kernels.h), on the stacked vector
// with the current frame in front:
//   cov      wpe_corr_kernel<STACK>: 4 x 4 tiles on and above the diagonal, chunk partials [chunk][b][f][N][N]; a second
//            kernel adds them in chunk order (no atomics, the same bits on every launch) and mirrors the upper triangle,
//            so Rf is exactly Hermitian with a real diagonal.
//   vector   one workgroup per (b, f): Rf's triangle and E in LDS, ldl_solve_lds (a zero, negative or non-finite pivot
//            takes reciprocal 0, so an all-zero bin gives h = 0 / 1e-15 = 0 exactly), then M, tau and h.  The factor
//            and X are kept for the backward (complex double).
//   apply    wpe_filter_kernel<kWpdApply> with h moved to f-fastest order first.
//   backward gh = sum_{t < n} conj(ge_t) v_t (time chunks, added in chunk order);
//            gv = gh / conj(tau), gtau = -(sum_i gh_i conj(h_i)) / conj(tau), gM = gv u^T + gtau E, gu = Re(M^H gv) summed
//            over the bins in bin order, gPhi = X^H gM, gX = gM Phi^H, Z = Rf^-1 gX from the kept factor, gRf = -Z X^H;
//            gw_t = Re(v_t^H gRf v_t) = -Re((v_t^H Z)(X^H v_t)) for t0 <= t < n (wpe_filter_kernel<kWpdQuad>, gRf moved to
//            f-fastest order first and kept fp64: the form cancels by a factor of cond(Rf)), gpower_t = -gw_t / power_t^2 where power_t > eps, else 0 (weights as given: gw_t).
//            gRf is handed over as a full matrix so that the three steps stay separate differentiable functions.
//
// Complex cotangents follow PyTorch: g is the tensor with dL = Re sum conj(g) dv, stored (re, im) like the value.
#include "wpe_kernels.h"

namespace {

constexpr double kTraceEps = 1e-15;

// sum of the chunk partials -> Rf [B][F][N][N] complex double, the lower triangle mirrored from the upper one
__global__ __launch_bounds__(256) void wpd_cov_sum_kernel(const double2* __restrict__ part, double2* __restrict__ Rf, long BF,
                                                          int N, int nchunk) {
  const long bf = blockIdx.x;
  const double2* p0 = part + bf * N * N;
  double2* o = Rf + bf * N * N;
  for (int idx = threadIdx.x; idx < N * N; idx += 256) {
    const int i = idx / N, j = idx % N;
    if (j < i) continue;
    double2 s = make_double2(0.0, 0.0);
    for (int ch = 0; ch < nchunk; ++ch) {                          // chunk order
      const double2 v = p0[ch * BF * N * N + (long)i * N + j];
      s.x += v.x; s.y += v.y;
    }
    if (i == j) { o[idx] = make_double2(s.x, 0.0); continue; }
    o[idx] = s;
    o[(long)j * N + i] = make_double2(s.x, -s.y);
  }
}

// in [B][F][M] -> out [B][M][F] (complex fp32 or fp64), through a 32 x 32 LDS tile
template <typename T2>
__global__ __launch_bounds__(256) void wpd_f_fastest_kernel(const T2* __restrict__ in, T2* __restrict__ out, int F, int M) {
  __shared__ T2 tile[32][33];
  const int b = blockIdx.z, f0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
  const int tx = threadIdx.x % 32, ty = threadIdx.x / 32;
  for (int r = ty; r < 32; r += 8) {
    const int f = f0 + r, m = m0 + tx;
    if (f < F && m < M) tile[r][tx] = in[((long)b * F + f) * M + m];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int m = m0 + r, f = f0 + tx;
    if (f < F && m < M) out[((long)b * M + m) * F + f] = tile[tx][r];
  }
}

struct VecLds {
  double2 *A, *Z, *X, *M, *phi, *gh, *hv, *gv, *sc;
  double *dinv, *u;
};
__device__ __forceinline__ VecLds vec_lds(char* smem, int N, int C) {
  VecLds s;
  s.A = reinterpret_cast<double2*>(smem);                          // [N][N + 1]
  s.Z = s.A + (long)N * (N + 1);                                   // [N][C]
  s.X = s.Z + (long)N * C;                                         // [N][C]
  s.M = s.X + (long)N * C;                                         // [N][C]
  s.phi = s.M + (long)N * C;                                       // [C][C]
  s.gh = s.phi + (long)C * C;                                      // [N]
  s.hv = s.gh + N;                                                 // [N]
  s.gv = s.hv + N;                                                 // [N]
  s.sc = s.gv + N;                                                 // tau, gtau
  s.dinv = reinterpret_cast<double*>(s.sc + 2);                    // [N]
  s.u = s.dinv + N;                                                // [C]
  return s;
}
constexpr size_t kVecLdsMax = 160 * 1024;                          // the CU's LDS: N = 64 fits with C <= 19 channels
inline size_t vec_lds_bytes(int N, int C) {
  return ((size_t)N * (N + 1) + 3 * (size_t)N * C + (size_t)C * C + 3 * (size_t)N + 2) * 16 + ((size_t)N + C) * 8;
}

__device__ __forceinline__ double2 zdiv(double2 a, double2 b) {       // a / b
  const double d = b.x * b.x + b.y * b.y;
  return make_double2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}

// M = X Phi, tau = tr(M[:C]) + 1e-15 and hv = M u / tau from X, phi and u in LDS; every thread may read them afterwards
__device__ __forceinline__ void vector_from_x(const VecLds& s, int N, int C) {
  const int tid = threadIdx.x;
  for (int idx = tid; idx < N * C; idx += kSolveThreads) {
    const int i = idx / C, d = idx % C;
    double2 m = make_double2(0.0, 0.0);
    for (int c = 0; c < C; ++c) {
      const double2 p = zmul(s.X[i * C + c], s.phi[c * C + d]);
      m.x += p.x; m.y += p.y;
    }
    s.M[idx] = m;
  }
  __syncthreads();
  if (tid == 0) {
    double2 t = make_double2(0.0, 0.0);
    for (int c = 0; c < C; ++c) { t.x += s.M[c * C + c].x; t.y += s.M[c * C + c].y; }
    s.sc[0] = make_double2(t.x + kTraceEps, t.y);
  }
  __syncthreads();
  const double2 tau = s.sc[0];
  for (int i = tid; i < N; i += kSolveThreads) {
    double2 v = make_double2(0.0, 0.0);
    for (int c = 0; c < C; ++c) { v.x += s.M[i * C + c].x * s.u[c]; v.y += s.M[i * C + c].y * s.u[c]; }
    s.hv[i] = zdiv(v, tau);
  }
  __syncthreads();
}

// Rf [B][F][N][N] complex double (its upper triangle is read), phi [B][F][C][C] complex fp32, u [B][C]
// -> h [B][F][N] complex fp32; fac [B][F][N][N] and xk [B][F][N][C] complex double unless NULL
__global__ __launch_bounds__(kSolveThreads) void wpd_vector_kernel(const double2* __restrict__ Rf, const float2* __restrict__ phi,
                                                                   const float* __restrict__ u, float2* __restrict__ h,
                                                                   double2* __restrict__ fac, double2* __restrict__ xk, int F,
                                                                   int N, int C) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const VecLds s = vec_lds(smem, N, C);
  const int lda = N + 1, tid = threadIdx.x;
  const long bf = blockIdx.x;
  const int b = (int)(bf / F);
  const double2* r0 = Rf + bf * N * N;
  for (int idx = tid; idx < N * N; idx += kSolveThreads) {
    const int i = idx / N, j = idx % N;
    if (j < i) continue;
    const double2 v = r0[idx];
    s.A[j * lda + i] = make_double2(v.x, i == j ? 0.0 : -v.y);      // Rf[j][i] = conj(Rf[i][j])
  }
  for (int idx = tid; idx < N * C; idx += kSolveThreads) s.Z[idx] = make_double2(idx / C == idx % C ? 1.0 : 0.0, 0.0);
  for (int idx = tid; idx < C * C; idx += kSolveThreads) {
    const float2 p = phi[bf * C * C + idx];
    s.phi[idx] = make_double2((double)p.x, (double)p.y);
  }
  if (tid < C) s.u[tid] = (double)u[(long)b * C + tid];
  ldl_solve_lds<true>(s.A, s.Z, s.dinv, N, C, lda);
  for (int idx = tid; idx < N * C; idx += kSolveThreads) s.X[idx] = s.Z[idx];
  __syncthreads();
  vector_from_x(s, N, C);
  for (int i = tid; i < N; i += kSolveThreads) h[bf * N + i] = make_float2((float)s.hv[i].x, (float)s.hv[i].y);
  if (fac) store_factor(fac + bf * N * N, s.A, s.dinv, N, lda);
  if (xk)
    for (int idx = tid; idx < N * C; idx += kSolveThreads) xk[bf * N * C + idx] = s.X[idx];
}

// gh [B][F][N] complex fp32 -> gphi [B][F][C][C] complex fp32, gup [B][F][C] fp64 (the bin's share of gu) and
// gRf [B][F][N][N] complex double; fac, xk as wpd_vector_kernel wrote them
__global__ __launch_bounds__(kSolveThreads) void wpd_vector_bwd_kernel(const double2* __restrict__ fac, const double2* __restrict__ xk,
                                                                       const float2* __restrict__ phi, const float* __restrict__ u,
                                                                       const float2* __restrict__ gh, float2* __restrict__ gphi,
                                                                       double* __restrict__ gup, double2* __restrict__ gRf, int F,
                                                                       int N, int C) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const VecLds s = vec_lds(smem, N, C);
  const int lda = N + 1, tid = threadIdx.x;
  const long bf = blockIdx.x;
  const int b = (int)(bf / F);
  load_factor(fac + bf * N * N, s.A, s.dinv, N, lda);
  for (int idx = tid; idx < N * C; idx += kSolveThreads) s.X[idx] = xk[bf * N * C + idx];
  for (int idx = tid; idx < C * C; idx += kSolveThreads) {
    const float2 p = phi[bf * C * C + idx];
    s.phi[idx] = make_double2((double)p.x, (double)p.y);
  }
  for (int i = tid; i < N; i += kSolveThreads) {
    const float2 g = gh[bf * N + i];
    s.gh[i] = make_double2((double)g.x, (double)g.y);
  }
  if (tid < C) s.u[tid] = (double)u[(long)b * C + tid];
  __syncthreads();
  vector_from_x(s, N, C);
  const double2 ctau = make_double2(s.sc[0].x, -s.sc[0].y);
  for (int i = tid; i < N; i += kSolveThreads) s.gv[i] = zdiv(s.gh[i], ctau);
  if (tid == 0) {
    double2 t = make_double2(0.0, 0.0);
    for (int i = 0; i < N; ++i) { const double2 p = zmulc(s.gh[i], s.hv[i]); t.x += p.x; t.y += p.y; }
    const double2 q = zdiv(t, ctau);
    s.sc[1] = make_double2(-q.x, -q.y);
  }
  __syncthreads();
  if (tid < C) {                                                    // gu's share: Re sum_i conj(M[i][c]) gv_i
    double g = 0.0;
    for (int i = 0; i < N; ++i) g += s.M[i * C + tid].x * s.gv[i].x + s.M[i * C + tid].y * s.gv[i].y;
    gup[bf * C + tid] = g;
  }
  __syncthreads();
  const double2 gtau = s.sc[1];
  for (int idx = tid; idx < N * C; idx += kSolveThreads) {          // gM over M
    const int i = idx / C, c = idx % C;
    double2 m = make_double2(s.gv[i].x * s.u[c], s.gv[i].y * s.u[c]);
    if (i == c) { m.x += gtau.x; m.y += gtau.y; }
    s.M[idx] = m;
  }
  __syncthreads();
  for (int idx = tid; idx < C * C; idx += kSolveThreads) {          // gPhi = X^H gM
    const int c = idx / C, d = idx % C;
    double2 g = make_double2(0.0, 0.0);
    for (int i = 0; i < N; ++i) {
      const double2 x = s.X[i * C + c], m = s.M[i * C + d];
      g.x += x.x * m.x + x.y * m.y; g.y += x.x * m.y - x.y * m.x;
    }
    gphi[bf * C * C + idx] = make_float2((float)g.x, (float)g.y);
  }
  for (int idx = tid; idx < N * C; idx += kSolveThreads) {          // gX = gM Phi^H
    const int i = idx / C, c = idx % C;
    double2 g = make_double2(0.0, 0.0);
    for (int d = 0; d < C; ++d) {
      const double2 p = zmulc(s.M[i * C + d], s.phi[c * C + d]);
      g.x += p.x; g.y += p.y;
    }
    s.Z[idx] = g;
  }
  ldl_solve_lds<false>(s.A, s.Z, s.dinv, N, C, lda);
  for (int idx = tid; idx < N * N; idx += kSolveThreads) {          // gRf = -Z X^H
    const int i = idx / N, j = idx % N;
    double2 g = make_double2(0.0, 0.0);
    for (int c = 0; c < C; ++c) {
      const double2 p = zmulc(s.Z[i * C + c], s.X[j * C + c]);
      g.x -= p.x; g.y -= p.y;
    }
    gRf[bf * N * N + idx] = g;
  }
}

// gu [B][C] = sum_f gup[b][f][c], in bin order
__global__ void wpd_gu_kernel(const double* __restrict__ gup, float* __restrict__ gu, int F, int C) {
  const int b = blockIdx.x, c = threadIdx.x;
  if (c >= C) return;
  double g = 0.0;
  for (int f = 0; f < F; ++f) g += gup[((long)b * F + f) * C + c];
  gu[(long)b * C + c] = (float)g;
}

// part [chunk][b][f][N] = sum over the chunk's frames t < n of conj(ge_t) v_t[i]; thread = (bin, 8 consecutive i)
constexpr int kGhSlots = 8;
__global__ __launch_bounds__(kFT * kGhSlots) void wpd_gh_kernel(const float2* __restrict__ ge, const float2* __restrict__ y,
                                                                const int* __restrict__ lens, double2* __restrict__ part, int B,
                                                                int T, int C, int F, int K, int delay, int nchunk) {
  const int N = C * (K + 1);
  const int f = blockIdx.x * kFT + threadIdx.x % kFT, i = blockIdx.y * kGhSlots + threadIdx.x / kFT;
  const int b = blockIdx.z / nchunk, ch = blockIdx.z % nchunk;
  if (f >= F || i >= N) return;
  int n = lens ? lens[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const int L = ceil_div(T, nchunk);
  const int c = i % C, shift = i < C ? 0 : delay + i / C - 1;
  const int tb = ch * L > shift ? ch * L : shift;                   // v_t[i] = 0 for t < shift
  const int te = n < (ch + 1) * L ? n : (ch + 1) * L;
  double ar = 0.0, ai = 0.0;
  for (int t = tb; t < te; ++t) {
    const float2 g = ge[((long)b * T + t) * F + f], v = y[(((long)b * T + t - shift) * C + c) * F + f];
    ar += (double)g.x * (double)v.x + (double)g.y * (double)v.y;
    ai += (double)g.x * (double)v.y - (double)g.y * (double)v.x;
  }
  part[((((long)ch * B + b) * F + f) * N) + i] = make_double2(ar, ai);
}

__global__ __launch_bounds__(256) void wpd_gh_sum_kernel(const double2* __restrict__ part, float2* __restrict__ gh, long total,
                                                         int nchunk) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  double2 s = make_double2(0.0, 0.0);
  for (int ch = 0; ch < nchunk; ++ch) { const double2 v = part[ch * total + i]; s.x += v.x; s.y += v.y; }
  gh[i] = make_float2((float)s.x, (float)s.y);
}

inline int bad_shape(int B, int T, int C, int F, int K, int delay) {
  if (B < 1 || T < 1 || C < 1 || F < 1 || K < 0 || delay < 1) return EAMD_EINVAL;
  if ((long)C * (K + 1) > kMaxN) return EAMD_EUNSUPPORTED;
  return EAMD_OK;
}

template <typename T2>
void to_f_fastest(const void* in, void* out, int B, int F, int M, hipStream_t st) {
  hipLaunchKernelGGL(wpd_f_fastest_kernel<T2>, dim3(ceil_div(F, 32), ceil_div(M, 32), B), dim3(256), 0, st, (const T2*)in,
                     (T2*)out, F, M);
}

}  // namespace

extern "C" {

int eamd_wpd_cov(const float* y, const float* power, const int32_t* lens, double* Rf, void* workspace, int B, int T, int C,
                 int F, int btaps, int bdelay, float eps, int inverse_power, int nchunk, void* stream) {
  if (!y || !Rf || !workspace) return EAMD_EINVAL;
  if (nchunk < 1 || nchunk > T) return EAMD_EINVAL;
  if (const int rc = bad_shape(B, T, C, F, btaps, bdelay)) return rc;
  if ((long)B * F > 0x7fffffffL) return EAMD_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int N = C * (btaps + 1);
  if (const int rc = launch_corr<true>(y, y, power, lens, workspace, B, T, C, F, btaps, bdelay, eps, inverse_power ? 0 : 1,
                                       nchunk, st))
    return rc;
  hipLaunchKernelGGL(wpd_cov_sum_kernel, dim3((unsigned)((long)B * F)), dim3(256), 0, st, (const double2*)workspace,
                     (double2*)Rf, (long)B * F, N, nchunk);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_wpd_cov_bwd(const float* y, const double* gRf, const float* power, const int32_t* lens, float* gpower, void* workspace,
                     int B, int T, int C, int F, int btaps, int bdelay, float eps, int inverse_power, void* stream) {
  if (!y || !gRf || !power || !gpower || !workspace) return EAMD_EINVAL;
  if (const int rc = bad_shape(B, T, C, F, btaps, bdelay)) return rc;
  if (B > 65535 || ceil_div(T, 2) > 65535) return EAMD_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int N = C * (btaps + 1);
  to_f_fastest<double2>(gRf, workspace, B, F, N * N, st);
  launch_filter<kWpdQuad>(y, workspace, lens, nullptr, power, gpower, B, T, C, F, btaps, bdelay, eps,
                          inverse_power, st);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_wpd_vector(const double* Rf, const float* phi, const float* u, float* h, double* fac, double* xkeep, int B, int F, int C,
                    int btaps, void* stream) {
  if (!Rf || !phi || !u || !h) return EAMD_EINVAL;
  if (const int rc = bad_shape(B, 1, C, F, btaps, 1)) return rc;
  if ((long)B * F > 0x7fffffffL) return EAMD_EUNSUPPORTED;
  if (vec_lds_bytes(C * (btaps + 1), C) > kVecLdsMax) return EAMD_EUNSUPPORTED;
  static const hipError_t attr_err = hipFuncSetAttribute(reinterpret_cast<const void*>(&wpd_vector_kernel),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVecLdsMax);
  if (attr_err != hipSuccess) return (int)attr_err;
  const int N = C * (btaps + 1);
  hipLaunchKernelGGL(wpd_vector_kernel, dim3((unsigned)((long)B * F)), dim3(kSolveThreads), vec_lds_bytes(N, C),
                     (hipStream_t)stream, (const double2*)Rf, (const float2*)phi, u, (float2*)h, (double2*)fac, (double2*)xkeep, F,
                     N, C);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_wpd_vector_bwd(const double* fac, const double* xkeep, const float* phi, const float* u, const float* gh, float* gphi,
                        float* gu, double* gRf, void* workspace, int B, int F, int C, int btaps, void* stream) {
  if (!fac || !xkeep || !phi || !u || !gh || !gphi || !gu || !gRf || !workspace) return EAMD_EINVAL;
  if (const int rc = bad_shape(B, 1, C, F, btaps, 1)) return rc;
  if ((long)B * F > 0x7fffffffL) return EAMD_EUNSUPPORTED;
  if (vec_lds_bytes(C * (btaps + 1), C) > kVecLdsMax) return EAMD_EUNSUPPORTED;
  static const hipError_t attr_err = hipFuncSetAttribute(reinterpret_cast<const void*>(&wpd_vector_bwd_kernel),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVecLdsMax);
  if (attr_err != hipSuccess) return (int)attr_err;
  hipStream_t st = (hipStream_t)stream;
  const int N = C * (btaps + 1);
  hipLaunchKernelGGL(wpd_vector_bwd_kernel, dim3((unsigned)((long)B * F)), dim3(kSolveThreads), vec_lds_bytes(N, C), st,
                     (const double2*)fac, (const double2*)xkeep, (const float2*)phi, u, (const float2*)gh, (float2*)gphi,
                     (double*)workspace, (double2*)gRf, F, N, C);
  hipLaunchKernelGGL(wpd_gu_kernel, dim3(B), dim3(64), 0, st, (const double*)workspace, gu, F, C);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_wpd_apply(const float* h, const float* y, const int32_t* lens, float* e, void* workspace, int B, int T, int C, int F,
                   int btaps, int bdelay, void* stream) {
  if (!h || !y || !e || !workspace) return EAMD_EINVAL;
  if (const int rc = bad_shape(B, T, C, F, btaps, bdelay)) return rc;
  if (B > 65535 || ceil_div(T, 2) > 65535) return EAMD_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  to_f_fastest<float2>(h, workspace, B, F, C * (btaps + 1), st);
  launch_filter<kWpdApply>(y, workspace, lens, e, nullptr, nullptr, B, T, C, F, btaps, bdelay, 0.f, 1, st);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_wpd_apply_bwd(const float* ge, const float* y, const int32_t* lens, float* gh, void* workspace, int B, int T, int C,
                       int F, int btaps, int bdelay, int nchunk, void* stream) {
  if (!ge || !y || !gh || !workspace) return EAMD_EINVAL;
  if (nchunk < 1 || nchunk > T) return EAMD_EINVAL;
  if (const int rc = bad_shape(B, T, C, F, btaps, bdelay)) return rc;
  if ((long)B * nchunk > 65535) return EAMD_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int N = C * (btaps + 1);
  const long total = (long)B * F * N;
  hipLaunchKernelGGL(wpd_gh_kernel, dim3(ceil_div(F, kFT), ceil_div(N, kGhSlots), B * nchunk), dim3(kFT * kGhSlots), 0, st,
                     (const float2*)ge, (const float2*)y, lens, (double2*)workspace, B, T, C, F, btaps, bdelay, nchunk);
  hipLaunchKernelGGL(wpd_gh_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double2*)workspace,
                     (float2*)gh, total, nchunk);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
