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

// IEEE division and libm's expf, as in beamformer.hip: the tests hold these kernels to the fp32 reference's own error
__device__ __forceinline__ float wpe_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float wpe_dsigmoid(float x) {
  const float e = expf(-fabsf(x)), s = 1.0f / (1.0f + e);
  return e * s * s;
}

__host__ __device__ inline int corr_sub_frames(int C) { const int ts = 64 / C; return ts < 1 ? 1 : (ts > 8 ? 8 : ts); }

// ---------------------------------------------------------------------------------------------------------------------
// correlations
// ---------------------------------------------------------------------------------------------------------------------
// mode 0: w_t = 1 / max(power, eps), t0 <= t < n;  mode 1: w_t = power;  mode 2 (backward): w_t = -1, 0 <= t < n, no R.
// out [chunk][b][f][N][ld]: ld = N + C with R (columns 0..N-1, on and above the diagonal tiles) then P, or ld = C.
__global__ __launch_bounds__(kCorrThreads, 3) void wpe_corr_kernel(const float2* __restrict__ y, const float2* __restrict__ rhs,
                                                                const float* __restrict__ power, const int* __restrict__ lens,
                                                                double2* __restrict__ out, int B, int T, int C, int F, int K,
                                                                int delay, float eps, int mode, int nchunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int N = C * K, NT = ceil_div(N, kTile), PT = ceil_div(C, kTile), TS = corr_sub_frames(C);
  const bool with_r = mode != 2;
  const int hrows = (TS + K - 1) * C, rrows = TS * C;
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
    } else {
      ti = task / PT; tj = NT + task % PT;
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
    aoff[r] = (av ? ((K - 1 - i / C) * C + i % C) * kFT : zrow) + lane;
    astep[r] = av ? C * kFT : 0;
    const int q = (bhist ? tj : tj - NT) * kTile + r;
    const bool bv = ti >= 0 && q < (bhist ? N : C);
    const int brow = bhist ? (K - 1 - q / C) * C + q % C : hrows + q;
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
  const int ld = with_r ? N + C : C;
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
  for (int idx = tid; idx < N * N; idx += kSolveThreads) {
    const int i = idx / N, j = idx % N;
    if (FACTOR) {
      if (j < i) continue;
      double2 s = make_double2(0.0, 0.0);
      for (int ch = 0; ch < nchunk; ++ch) {                        // chunk order: the same bits on every launch
        const double2 v = p0[ch * cstride + (long)i * ld + j];
        s.x += v.x; s.y += v.y;
      }
      A[j * lda + i] = make_double2(s.x, i == j ? 0.0 : -s.y);      // R[j][i] = conj(R[i][j])
    } else {
      const double2 v = fac[(bf * N + i) * N + j];
      if (j < i) A[i * lda + j] = v;
      else if (j == i) dinv[i] = v.x;
    }
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
  for (int idx = tid; idx < N * C; idx += kSolveThreads) {
    const double2 z = Z[idx];
    G[((long)b * N * C + idx) * F + f] = make_float2((float)z.x, (float)z.y);
  }
  if (FACTOR && fac)
    for (int idx = tid; idx < N * N; idx += kSolveThreads) {
      const int i = idx / N, j = idx % N;
      double2 v = make_double2(0.0, 0.0);
      if (j < i) v = A[i * lda + j];
      else if (j == i) v.x = dinv[i];
      fac[bf * N * N + idx] = v;
    }
}

inline size_t solve_lds_bytes(int N, int C) { return ((size_t)N * (N + 1) + (size_t)N * C) * 16 + (size_t)N * 8; }

// ---------------------------------------------------------------------------------------------------------------------
// filter and its backward
// ---------------------------------------------------------------------------------------------------------------------
// u_t[c'] = sum_i conj(G[i][c']) h_t[i].  !BWD: x_t = y_t - u_t (0 for t >= n).  BWD (G holds Z): gw_t = Re sum_c'
// conj(u_t[c']) x_t[c'], gpower as in the header; xio is x (read), pw the power the forward took, gp the output.
template <int TT, bool BWD>
__global__ __launch_bounds__(kFT * kMaxCG) void wpe_filter_kernel(const float2* __restrict__ y, const float2* __restrict__ G,
                                                                  const int* __restrict__ lens, float2* __restrict__ xio,
                                                                  const float* __restrict__ pw, float* __restrict__ gp, int B,
                                                                  int T, int C, int F, int K, int delay, float eps,
                                                                  int inverse_power) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int N = C * K, CG = blockDim.x / kFT;
  const int wrows = (TT + K - 1) * C;
  float2* win = reinterpret_cast<float2*>(smem);                  // [wrows][kFT]
  double* red = reinterpret_cast<double*>(win + (long)wrows * kFT);   // BWD: [CG][TT][kFT]
  const int f0 = blockIdx.x * kFT, tc = blockIdx.y * TT, b = blockIdx.z;
  const int lane = threadIdx.x % kFT, cg = threadIdx.x / kFT;
  const int f = f0 + lane;
  int n = lens ? lens[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  if (tc >= n) {                                                  // a chunk of padded frames: exact zeros (uniform branch)
    for (int idx = threadIdx.x; idx < TT * (BWD ? 1 : C) * kFT; idx += blockDim.x) {
      const int l = idx % kFT, r = idx / kFT;
      const int t = tc + (BWD ? r : r / C);
      if (t >= T || f0 + l >= F) continue;
      if (BWD) gp[((long)b * T + t) * F + f0 + l] = 0.f;
      else xio[(((long)b * T + t) * C + r % C) * F + f0 + l] = make_float2(0.f, 0.f);
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
      const int q = (int)(((unsigned)row * magic) >> 16);
      const int frame = tc - delay - (K - 1) + q, c = row - q * C;
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
  for (int co = cg; co < C; co += CG) {
    double ur[TT], ui[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) ur[tt] = ui[tt] = 0.0;
    if (f < F) {
      for (int i = 0; i < N; ++i) {
        const float2 g = G[(((long)b * N + i) * C + co) * F + f];
        const double gr = (double)g.x, gi = (double)g.y;
        const float2* wp = win + (long)((K - 1 - i / C) * C + i % C) * kFT + lane;
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {                          // conj(g) h
          const float2 v = wp[(long)tt * C * kFT];
          ur[tt] += gr * (double)v.x + gi * (double)v.y;
          ui[tt] += gr * (double)v.y - gi * (double)v.x;
        }
      }
#pragma unroll
      for (int tt = 0; tt < TT; ++tt) {
        const int t = tc + tt;
        if (t >= T) continue;
        const long o = (((long)b * T + t) * C + co) * F + f;
        if (BWD) {
          if (t < n) { const float2 xv = xio[o]; s[tt] += ur[tt] * (double)xv.x + ui[tt] * (double)xv.y; }
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
inline size_t filter_lds_bytes(int TT, int C, int K, int CG, bool bwd) {
  return (size_t)(TT + K - 1) * C * kFT * 8 + (bwd ? (size_t)CG * TT * kFT * 8 : 0);
}

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

int launch_corr(const float* y, const float* rhs, const float* power, const int* lens, void* out, int B, int T, int C, int F,
                int K, int delay, float eps, int mode, int nchunk, hipStream_t st) {
  const int N = C * K, NT = ceil_div(N, kTile), PT = ceil_div(C, kTile), TS = corr_sub_frames(C);
  const int ntask = mode != 2 ? NT * (NT + 1) / 2 + NT * PT : NT * PT;
  if ((long)B * nchunk > 65535) return EAMD_EUNSUPPORTED;
  const size_t lds = ((size_t)(TS + K - 1) * C + (size_t)TS * C + 1) * kFT * 8 + (size_t)TS * kFT * 8;
  const dim3 grid(ceil_div(F, kFT), ceil_div(ntask, kSlots), B * nchunk);
  hipLaunchKernelGGL(wpe_corr_kernel, grid, dim3(kCorrThreads), lds, st, (const float2*)y, (const float2*)rhs, power, lens,
                     (double2*)out, B, T, C, F, K, delay, eps, mode, nchunk);
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

template <bool BWD>
void launch_filter(const float* y, const float* G, const int* lens, float* xio, const float* pw, float* gp, int B, int T, int C,
                   int F, int K, int delay, float eps, int inverse_power, hipStream_t st) {
  const int TT = filter_frames(C), CG = C < kMaxCG ? C : kMaxCG;
  const dim3 grid(ceil_div(F, kFT), ceil_div(T, TT), B), block(kFT * CG);
  const size_t lds = filter_lds_bytes(TT, C, K, CG, BWD);
  if (TT == 8)
    hipLaunchKernelGGL((wpe_filter_kernel<8, BWD>), grid, block, lds, st, (const float2*)y, (const float2*)G, lens, (float2*)xio,
                       pw, gp, B, T, C, F, K, delay, eps, inverse_power);
  else
    hipLaunchKernelGGL((wpe_filter_kernel<2, BWD>), grid, block, lds, st, (const float2*)y, (const float2*)G, lens, (float2*)xio,
                       pw, gp, B, T, C, F, K, delay, eps, inverse_power);
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
  if (const int rc = launch_corr(y, y, power, lens, workspace, B, T, C, F, taps, delay, eps, inverse_power ? 0 : 1, nchunk, st))
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
  launch_filter<false>(y, G, lens, x, nullptr, nullptr, B, T, C, F, taps, delay, 0.f, 1, (hipStream_t)stream);
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
  if (const int rc = launch_corr(y, gx, nullptr, lens, workspace, B, T, C, F, taps, delay, eps, 2, nchunk, st)) return rc;
  if (const int rc = launch_solve<false>(workspace, (void*)fac, Z, B, F, N, C, nchunk, st)) return rc;
  launch_filter<true>(y, Z, lens, (float*)x, power, gpower, B, T, C, F, taps, delay, eps, inverse_power, st);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
