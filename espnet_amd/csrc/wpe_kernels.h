// Kernels that the WPE dereverberation (wpe.hip) and the WPD / MPDR convolutional beamformers (wpd.hip) share: the
// correlation pass over stacked frames, the in-LDS LDL^H solve and the filter pass.  Both files work on interleaved
// (re, im) fp32 spectra y [B, T, C, F, 2] and on a vector of stacked frames per (b, t, f):
//   WPE (STACK = false)   h_t[k C + c] = y[t - D - k, c],  k = 0..K-1                      N = C K
//   WPD (STACK = true)    the current frame first: v_t[c] = y[t, c],  v_t[(k + 1) C + c] = y[t - D - k, c]    N = C (K + 1)
// (zero before frame 0).  Neither vector is ever written to memory: a workgroup stages a window of frames of a 32-bin
// tile in LDS, f fastest - 256 contiguous bytes per (frame, channel) row - and lane l reads float2 l of a row,
// conflict-free.  Every product and sum is fp64.  See wpe.hip for the description of each pass.
#pragma once
#include "common.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int kFT = EAMD_WPE_FTILE;          // frequency bins per workgroup
constexpr int kCorrThreads = 256;           // 3 workgroups per CU (registers and LDS): one stages while two compute
constexpr int kSlots = kCorrThreads / kFT;   // tasks (4 x 4 tiles of [R | P]) per corr workgroup
constexpr int kTile = 4;
constexpr int kMaxN = EAMD_WPE_MAX_UNKNOWNS;
constexpr int kSolveThreads = 256;
constexpr int kMaxCG = 8;                    // output channels that a filter workgroup handles side by side

__host__ __device__ constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }

__host__ __device__ inline int corr_sub_frames(int C) { const int ts = 64 / C; return ts < 1 ? 1 : (ts > 8 ? 8 : ts); }

// rows of the delayed-frame window that serves TT consecutive frames (none without taps: WPD with K = 0 is MPDR)
__host__ __device__ inline int window_rows(int TT, int C, int K) { return K > 0 ? (TT + K - 1) * C : 0; }

// LDS row (at sub-step frame 0) of element i of the stacked vector; the current frames follow the `hrows` window rows
template <bool STACK>
__device__ __forceinline__ int stacked_row(int i, int C, int K, int hrows) {
  if (STACK) {
    if (i < C) return hrows + i;
    i -= C;
  }
  return (K - 1 - i / C) * C + i % C;
}

// ---------------------------------------------------------------------------------------------------------------------
// correlations
// ---------------------------------------------------------------------------------------------------------------------
// mode 0: w_t = 1 / max(power, eps), t0 <= t < n;  mode 1: w_t = power (power == NULL: 1);  mode 2 (backward, WPE only):
// w_t = -1, 0 <= t < n, no R.
// !STACK: out [chunk][b][f][N][ld]: ld = N + C with R (columns 0..N-1, on and above the diagonal tiles) then P, or ld = C.
// STACK:  out [chunk][b][f][N][N]: sum w_t v_t v_t^H on and above the diagonal tiles; rhs is y.
template <bool STACK>
__global__ __launch_bounds__(kCorrThreads, 3) void wpe_corr_kernel(const float2* __restrict__ y, const float2* __restrict__ rhs,
                                                                const float* __restrict__ power, const int* __restrict__ lens,
                                                                double2* __restrict__ out, int B, int T, int C, int F, int K,
                                                                int delay, float eps, int mode, int nchunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int N = STACK ? C * (K + 1) : C * K, NT = ceil_div(N, kTile), PT = STACK ? 0 : ceil_div(C, kTile);
  const int TS = corr_sub_frames(C);
  const bool with_r = mode != 2;
  const int hrows = window_rows(TS, C, K), rrows = TS * C;
  float2* hist = reinterpret_cast<float2*>(smem);                 // [hrows][kFT]
  float2* cur = hist + (long)hrows * kFT;                         // [rrows][kFT]
  double* wgt = reinterpret_cast<double*>(cur + (long)(rrows + 1) * kFT);   // [TS][kFT], behind one row of zeros
  const int f0 = blockIdx.x * kFT;
  const int b = blockIdx.z / nchunk, ch = blockIdx.z % nchunk;
  const int lane = threadIdx.x % kFT, slot = threadIdx.x / kFT;
  const int f = f0 + lane;
  int n = lens ? lens[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const int L = ceil_div(T, nchunk);
  const int first = with_r ? delay + K - 1 : 0;
  const int tb = first > ch * L ? first : ch * L;
  const int te = n < (ch + 1) * L ? n : (ch + 1) * L;

  // this half-wave's tile (ti, tj): tj < NT a tile of R (tj >= ti), tj >= NT tile tj - NT of P
  const int ntask = with_r ? NT * (NT + 1) / 2 + NT * PT : NT * PT;
  const int task = blockIdx.y * kSlots + slot;
  int ti = -1, tj = -1;
  if (task < ntask) {
    if (with_r) {
      int r = 0, rem = task;
      while (rem >= NT - r + PT) { rem -= NT - r + PT; ++r; }
      ti = r; tj = r + rem;
    } else if (!STACK) {
      const int pt = STACK ? 1 : PT;
      ti = task / pt; tj = NT + task % pt;
    }
  }
  const bool active = ti >= 0 && f < F;
  // LDS offsets (in float2) of the tile's operands at sub-step frame 0 and their step per frame; an operand past the
  // matrix edge reads the zero row with step 0, so the inner loop has no branch
  const int zrow = (hrows + rrows) * kFT;
  int aoff[kTile], boff[kTile], astep[kTile], bstep[kTile];
  const bool bhist = tj < NT;
#pragma unroll
  for (int r = 0; r < kTile; ++r) {
    const int i = ti * kTile + r;
    const bool av = ti >= 0 && i < N;
    aoff[r] = (av ? stacked_row<STACK>(i, C, K, hrows) * kFT : zrow) + lane;
    astep[r] = av ? C * kFT : 0;
    const int q = (bhist ? tj : tj - NT) * kTile + r;
    const bool bv = ti >= 0 && q < (bhist ? N : C);
    const int brow = bhist ? stacked_row<STACK>(bv ? q : 0, C, K, hrows) : hrows + q;
    boff[r] = (bv ? brow * kFT : zrow) + lane;
    bstep[r] = bv ? C * kFT : 0;
  }
  double accr[kTile][kTile], acci[kTile][kTile];
#pragma unroll
  for (int r = 0; r < kTile; ++r)
#pragma unroll
    for (int s = 0; s < kTile; ++s) accr[r][s] = acci[r][s] = 0.0;
  if (threadIdx.x < kFT) hist[zrow + threadIdx.x] = make_float2(0.f, 0.f);

  constexpr int U = 8;                                              // loads in flight per thread while staging
  const int total = hrows + rrows;                                  // < 256 rows: hrows < 128, rrows <= 64
  const unsigned magic = (65536u + C - 1) / C;                      // (rr * magic) >> 16 == rr / C for rr < 1024, C <= 64
  for (int ts = tb; ts < te; ts += TS) {
    for (int r0 = slot; r0 < total; r0 += kSlots * U) {             // cur follows hist: one row index for both
      float2 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = r0 + u * kSlots;
        const bool h = row < hrows;
        const int rr = h ? row : row - hrows;
        const int q = (int)(((unsigned)rr * magic) >> 16);
        const int frame = (h ? ts - delay - (K - 1) : ts) + q, c = rr - q * C;
        v[u] = make_float2(0.f, 0.f);
        if (row < total && frame >= 0 && frame < T && f < F) v[u] = (h ? y : rhs)[(((long)b * T + frame) * C + c) * F + f];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int row = r0 + u * kSlots;
        if (row < total) hist[row * kFT + lane] = v[u];
      }
    }
    if (threadIdx.x < TS * kFT) {                                   // TS <= 8: one weight per thread
      const int t = ts + threadIdx.x / kFT;
      double w = 0.0;
      if (t < te && f < F) {
        if (mode == 2) w = -1.0;
        else if (!power) w = 1.0;
        else {
          const double p = (double)power[((long)b * T + t) * F + f];
          w = mode == 0 ? 1.0 / (p > (double)eps ? p : (double)eps) : p;
        }
      }
      wgt[threadIdx.x] = w;
    }
    __syncthreads();
    if (active) {
      const int nt = te - ts < TS ? te - ts : TS;
      for (int tt = 0; tt < nt; ++tt) {
        const double w = wgt[tt * kFT + lane];
        double ar[kTile], ai[kTile], br[kTile], bi[kTile];
#pragma unroll
        for (int r = 0; r < kTile; ++r) {
          const float2 a = hist[aoff[r] + tt * astep[r]], bb = hist[boff[r] + tt * bstep[r]];
          ar[r] = w * (double)a.x; ai[r] = w * (double)a.y;
          br[r] = (double)bb.x; bi[r] = (double)bb.y;
        }
#pragma unroll
        for (int r = 0; r < kTile; ++r)
#pragma unroll
          for (int s = 0; s < kTile; ++s) {                      // a conj(b), four FMAs
            accr[r][s] = fma(ai[r], bi[s], fma(ar[r], br[s], accr[r][s]));
            acci[r][s] = fma(-ar[r], bi[s], fma(ai[r], br[s], acci[r][s]));
          }
      }
    }
    __syncthreads();
  }
  if (!active) return;
  const int ld = STACK ? N : (with_r ? N + C : C);
  double2* o = out + (((long)ch * B + b) * F + f) * N * ld;
#pragma unroll
  for (int r = 0; r < kTile; ++r) {
    const int i = ti * kTile + r;
    if (i >= N) continue;
#pragma unroll
    for (int s = 0; s < kTile; ++s) {
      const int q = (bhist ? tj : tj - NT) * kTile + s;
      if (q >= (bhist ? N : C)) continue;
      const int col = bhist ? q : (with_r ? N + q : q);
      o[(long)i * ld + col] = make_double2(accr[r][s], acci[r][s]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// solve
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double2 zmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 zmulc(double2 a, double2 b) {      // a conj(b)
  return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}

// The solve of R X = Z in LDS, by the whole workgroup of kSolveThreads threads.  A [N][lda] holds the lower triangle
// (FACTOR: of R, overwritten by L d; !FACTOR: L d as a factorisation left it, and dinv [N] = 1 / d), Z [N][C] the right-
// hand sides, overwritten by the solution.  Right-looking LDL^H without pivoting, the forward substitution fused into
// the elimination, then the back substitution.  A pivot that is zero, negative or not finite takes reciprocal 0.
// The caller's writes to A, Z and dinv need no barrier before the call; the result is visible to every thread after it.
template <bool FACTOR>
__device__ __forceinline__ void ldl_solve_lds(double2* A, double2* Z, double* dinv, int N, int C, int lda) {
  const int tid = threadIdx.x;
  __syncthreads();
  // right-looking LDL^H; the same sweep eliminates the right-hand sides (L z = P)
  for (int k = 0; k < N; ++k) {
    double di;
    if (FACTOR) {
      const double d = A[k * lda + k].x;
      di = (d > 0.0 && d < __builtin_inf()) ? 1.0 / d : 0.0;
      if (tid == 0) dinv[k] = di;
    } else {
      di = dinv[k];
    }
    const int m = N - 1 - k;
    if (FACTOR)
      for (int idx = tid; idx < m * m; idx += kSolveThreads) {
        const int i = k + 1 + idx / m, j = k + 1 + idx % m;
        if (j > i) continue;
        const double2 u = zmulc(A[i * lda + k], A[j * lda + k]);
        double2 a = A[i * lda + j];
        a.x -= u.x * di; a.y -= u.y * di;
        A[i * lda + j] = a;
      }
    for (int idx = tid; idx < m * C; idx += kSolveThreads) {
      const int i = k + 1 + idx / C, c = idx % C;
      const double2 u = zmul(A[i * lda + k], Z[k * C + c]);
      double2 z = Z[i * C + c];
      z.x -= u.x * di; z.y -= u.y * di;
      Z[i * C + c] = z;
    }
    __syncthreads();
  }
  for (int idx = tid; idx < N * C; idx += kSolveThreads) {
    const double di = dinv[idx / C];
    Z[idx].x *= di; Z[idx].y *= di;
  }
  __syncthreads();
  for (int k = N - 1; k > 0; --k) {                                  // L^H g = z
    for (int idx = tid; idx < k * C; idx += kSolveThreads) {
      const int i = idx / C, c = idx % C;
      const double2 a = A[k * lda + i];
      const double di = dinv[i];
      const double2 u = zmul(make_double2(a.x * di, -a.y * di), Z[k * C + c]);
      double2 z = Z[i * C + c];
      z.x -= u.x; z.y -= u.y;
      Z[i * C + c] = z;
    }
    __syncthreads();
  }
}

// fac [N][N] complex double of one (b, f): L d below the diagonal, 1 / d on it, 0 above - what eamd_wpe_bwd and
// eamd_wpd_vector_bwd take back
__device__ __forceinline__ void store_factor(double2* __restrict__ fac, const double2* A, const double* dinv, int N, int lda) {
  for (int idx = threadIdx.x; idx < N * N; idx += kSolveThreads) {
    const int i = idx / N, j = idx % N;
    double2 v = make_double2(0.0, 0.0);
    if (j < i) v = A[i * lda + j];
    else if (j == i) v.x = dinv[i];
    fac[idx] = v;
  }
}

__device__ __forceinline__ void load_factor(const double2* __restrict__ fac, double2* A, double* dinv, int N, int lda) {
  for (int idx = threadIdx.x; idx < N * N; idx += kSolveThreads) {
    const int i = idx / N, j = idx % N;
    const double2 v = fac[idx];
    if (j < i) A[i * lda + j] = v;
    else if (j == i) dinv[i] = v.x;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// filter
// ---------------------------------------------------------------------------------------------------------------------
// u_t[c'] = sum_i conj(G[i][c']) s_t[i] over the stacked vector s_t (h_t or v_t above), G [B][N][Co][F], f fastest.
//   kWpeFilter  Co = C:  x_t = y_t - u_t (0 for t >= n) into xio [B,T,C,F]
//   kWpeBwd     Co = C, G holds Z:  gw_t = Re sum_c' conj(u_t[c']) x_t[c'], x read from xio; gp = -gw / power^2 where
//               power > eps (inverse_power == 0: gw), 0 outside t0 <= t < n
//   kWpdApply   Co = 1, G holds the filter vector:  e_t = u_t (0 for t >= n) into xio [B,T,F]
//   kWpdQuad    Co = N, G holds a matrix in fp64 (the quadratic form cancels by a factor of cond(Rf): fp32 would not do):  gw_t = Re sum_j conj(u_t[j]) v_t[j] = Re(v_t^H G v_t), v_t read from the window;
//               gp from gw as kWpeBwd
enum { kWpeFilter = 0, kWpeBwd = 1, kWpdApply = 2, kWpdQuad = 3 };
template <int MODE> struct filter_matrix { using type = float2; };
template <> struct filter_matrix<kWpdQuad> { using type = double2; };

template <int TT, int MODE>
__global__ __launch_bounds__(kFT * kMaxCG) void wpe_filter_kernel(const float2* __restrict__ y,
                                                                  const typename filter_matrix<MODE>::type* __restrict__ G,
                                                                  const int* __restrict__ lens, float2* __restrict__ xio,
                                                                  const float* __restrict__ pw, float* __restrict__ gp, int B,
                                                                  int T, int C, int F, int K, int delay, float eps,
                                                                  int inverse_power) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool STACK = MODE == kWpdApply || MODE == kWpdQuad;
  constexpr bool BWD = MODE == kWpeBwd || MODE == kWpdQuad;
  const int N = STACK ? C * (K + 1) : C * K, CG = blockDim.x / kFT;
  const int Co = MODE == kWpdApply ? 1 : (MODE == kWpdQuad ? N : C);
  const int hrows = window_rows(TT, C, K);
  const int wrows = hrows + (STACK ? TT * C : 0);                 // STACK: the TT current frames follow the window
  float2* win = reinterpret_cast<float2*>(smem);                  // [wrows][kFT]
  double* red = reinterpret_cast<double*>(win + (long)wrows * kFT);   // BWD: [CG][TT][kFT]
  const int f0 = blockIdx.x * kFT, tc = blockIdx.y * TT, b = blockIdx.z;
  const int lane = threadIdx.x % kFT, cg = threadIdx.x / kFT;
  const int f = f0 + lane;
  int n = lens ? lens[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  if (tc >= n) {                                                  // a chunk of padded frames: exact zeros (uniform branch)
    const int per = BWD || MODE == kWpdApply ? 1 : C;
    for (int idx = threadIdx.x; idx < TT * per * kFT; idx += blockDim.x) {
      const int l = idx % kFT, r = idx / kFT;
      const int t = tc + r / per;
      if (t >= T || f0 + l >= F) continue;
      if (BWD) gp[((long)b * T + t) * F + f0 + l] = 0.f;
      else xio[(((long)b * T + t) * per + r % per) * F + f0 + l] = make_float2(0.f, 0.f);
    }
    return;
  }
  constexpr int U = 8;                                              // loads in flight per thread while staging
  const unsigned magic = (65536u + C - 1) / C;                      // (row * magic) >> 16 == row / C for row < 1024, C <= 64
  for (int r0 = cg; r0 < wrows; r0 += CG * U) {
    float2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = r0 + u * CG;
      const bool h = row < hrows;
      const int rr = h ? row : row - hrows;
      const int q = (int)(((unsigned)rr * magic) >> 16);
      const int frame = (h ? tc - delay - (K - 1) : tc) + q, c = rr - q * C;
      v[u] = make_float2(0.f, 0.f);
      if (row < wrows && frame >= 0 && frame < T && f < F) v[u] = y[(((long)b * T + frame) * C + c) * F + f];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = r0 + u * CG;
      if (row < wrows) win[row * kFT + lane] = v[u];
    }
  }
  __syncthreads();
  double s[TT];
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) s[tt] = 0.0;
  for (int co = cg; co < Co; co += CG) {
    double ur[TT], ui[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) ur[tt] = ui[tt] = 0.0;
    if (f < F) {
      for (int i = 0; i < N; ++i) {
        const auto g = G[(((long)b * N + i) * Co + co) * F + f];
        const double gr = (double)g.x, gi = (double)g.y;
        const float2* wp = win + (long)stacked_row<STACK>(i, C, K, hrows) * kFT + lane;
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {                          // conj(g) h
          const float2 v = wp[(long)tt * C * kFT];
          ur[tt] += gr * (double)v.x + gi * (double)v.y;
          ui[tt] += gr * (double)v.y - gi * (double)v.x;
        }
      }
      const float2* vp = win + (long)stacked_row<STACK>(MODE == kWpdQuad ? co : 0, C, K, hrows) * kFT + lane;
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const int t = tc + tt;
        if (t >= T) continue;
        const long o = (((long)b * T + t) * Co + co) * F + f;
        if (MODE == kWpdQuad) {
          if (t < n) { const float2 xv = vp[(long)tt * C * kFT]; s[tt] += ur[tt] * (double)xv.x + ui[tt] * (double)xv.y; }
        } else if (MODE == kWpeBwd) {
          if (t < n) { const float2 xv = xio[o]; s[tt] += ur[tt] * (double)xv.x + ui[tt] * (double)xv.y; }
        } else if (MODE == kWpdApply) {
          xio[o] = t < n ? make_float2((float)ur[tt], (float)ui[tt]) : make_float2(0.f, 0.f);
        } else {
          float2 r = make_float2(0.f, 0.f);
          if (t < n) { const float2 yv = y[o]; r = make_float2((float)((double)yv.x - ur[tt]), (float)((double)yv.y - ui[tt])); }
          xio[o] = r;
        }
      }
    }
  }
  if (BWD) {
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) red[((long)cg * TT + tt) * kFT + lane] = s[tt];
    __syncthreads();
    for (int idx = threadIdx.x; idx < TT * kFT; idx += blockDim.x) {
      const int tt = idx / kFT, l = idx % kFT, t = tc + tt;
      if (t >= T || f0 + l >= F) continue;
      double gw = 0.0;
      for (int g = 0; g < CG; ++g) gw += red[((long)g * TT + tt) * kFT + l];     // channel-group order
      float r = 0.f;
      if (t >= delay + K - 1 && t < n) {
        if (inverse_power) {
          const double p = (double)pw[((long)b * T + t) * F + f0 + l];
          if (p > (double)eps) r = (float)(-gw / (p * p));
        } else {
          r = (float)gw;
        }
      }
      gp[((long)b * T + t) * F + f0 + l] = r;
    }
  }
}

inline int filter_frames(int C) { return C <= 16 ? 8 : 2; }
inline size_t filter_lds_bytes(int TT, int C, int K, int CG, bool stack, bool bwd) {
  return (size_t)(window_rows(TT, C, K) + (stack ? TT * C : 0)) * kFT * 8 + (bwd ? (size_t)CG * TT * kFT * 8 : 0);
}

template <bool STACK>
int launch_corr(const float* y, const float* rhs, const float* power, const int* lens, void* out, int B, int T, int C, int F,
                int K, int delay, float eps, int mode, int nchunk, hipStream_t st) {
  const int N = STACK ? C * (K + 1) : C * K, NT = ceil_div(N, kTile), PT = STACK ? 0 : ceil_div(C, kTile);
  const int TS = corr_sub_frames(C);
  const int ntask = mode != 2 ? NT * (NT + 1) / 2 + NT * PT : NT * PT;
  if ((long)B * nchunk > 65535) return EAMD_EUNSUPPORTED;
  const size_t lds = ((size_t)window_rows(TS, C, K) + (size_t)TS * C + 1) * kFT * 8 + (size_t)TS * kFT * 8;
  const dim3 grid(ceil_div(F, kFT), ceil_div(ntask, kSlots), B * nchunk);
  hipLaunchKernelGGL(wpe_corr_kernel<STACK>, grid, dim3(kCorrThreads), lds, st, (const float2*)y, (const float2*)rhs, power,
                     lens, (double2*)out, B, T, C, F, K, delay, eps, mode, nchunk);
  return EAMD_OK;
}

template <int MODE>
void launch_filter(const float* y, const void* G, const int* lens, float* xio, const float* pw, float* gp, int B, int T, int C,
                   int F, int K, int delay, float eps, int inverse_power, hipStream_t st) {
  constexpr bool STACK = MODE == kWpdApply || MODE == kWpdQuad;
  constexpr bool BWD = MODE == kWpeBwd || MODE == kWpdQuad;
  using GT = typename filter_matrix<MODE>::type;
  const int CG = C < kMaxCG ? C : kMaxCG;
  int TT = filter_frames(C);
  if (filter_lds_bytes(TT, C, K, CG, STACK, BWD) > 64 * 1024) TT = 2;   // only the stacked window of 9..16 channels
  const dim3 grid(ceil_div(F, kFT), ceil_div(T, TT), B), block(kFT * CG);
  const size_t lds = filter_lds_bytes(TT, C, K, CG, STACK, BWD);
  if (TT == 8)
    hipLaunchKernelGGL((wpe_filter_kernel<8, MODE>), grid, block, lds, st, (const float2*)y, (const GT*)G, lens, (float2*)xio,
                       pw, gp, B, T, C, F, K, delay, eps, inverse_power);
  else
    hipLaunchKernelGGL((wpe_filter_kernel<2, MODE>), grid, block, lds, st, (const float2*)y, (const GT*)G, lens, (float2*)xio,
                       pw, gp, B, T, C, F, K, delay, eps, inverse_power);
}

}  // namespace
