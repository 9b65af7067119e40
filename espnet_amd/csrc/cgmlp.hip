// Convolutional spatial gating unit (CSGU) of the E-Branchformer's cgMLP branch, forward and backward, on the
// channels-last pre-activation a [B, T, 2*Ch] of channel_proj1 (value columns 0..Ch-1 | gate columns Ch..2Ch-1):
//     h = GELU(a) (exact erf form),  r = h[.., :Ch],  g = h[.., Ch:]
//     n = LayerNorm_Ch(g; gamma, beta),  c = depthwise_conv1d_K(n; w, bias) over time (zero padding, per utterance),  y = r * c
// (Kim et al., "E-Branchformer", SLT 2022; Sakuma et al., "MLP-based architecture with variable length input", 2021).
// h, n and c never reach memory: the only things kept for backward are a and the [B*T, 2] row statistics of g.
//
// Why it is tiled this way.  The LayerNorm couples all Ch channels of a frame, the convolution couples K frames of one
// channel: a single tile that closes over both would be a whole utterance.  The coupling across channels is only two
// numbers per frame, so it is taken out first (forward: mean / rstd, one wave per row, GELU on load, (g - mean)^2 summed
// after the mean is known) or last (backward: two row sums).  What remains is local in channels, and a workgroup owns
// (utterance b, 64 frames, 64 channels): lane = channel, so every global row access is one contiguous 256-byte line, and
// 8 waves x 8 frames.  The 64 + K - 1 gate rows of the tile (halo included, rows outside [0, T) as zeros: the padding
// is applied to n, and the clamp never crosses into a neighbouring utterance) are loaded once with all of a thread's
// loads in flight, GELU'd and normalised on their way into LDS (24 KB at K = 31), so each element pays its erf once per
// tile - (64 + K - 1) / 64 times overall - rather than K times.  The K taps of a lane's channel sit in registers
// (staged through LDS so that the global read is contiguous) and each wave slides them over its 8 + K - 1 LDS rows with
// fully unrolled FMAs: 8 accumulators, one LDS read per 8 FMAs.  The value half a_r is touched only in the epilogue.
// Two instantiations bound the unroll: K <= 15 and K <= 31.
//
// Backward recomputes instead of reading: the tile kernel rebuilds xhat (the normalised gate) and dc = dy * GELU(a_r)
// for its rows + halo in two LDS tiles (48 KB), then in ONE sweep over the rows forms c (for dr = dy * c), the transposed
// convolution dn of dc (the dc tile is stored time-reversed, so dn walks it forwards with the same tap registers), and the
// K tap-gradient accumulators dc[t] * n[t + k - pad].  da_r = dy c GELU'(a_r) is final there;
// the gate half needs the LayerNorm backward's two sums over ALL channels of a row, so the tile kernel stores
// dxhat = dn * gamma into da's gate columns and leaves its 64-channel share of sum(dxhat), sum(dxhat * xhat) per
// (row, slab); a row kernel (one wave per row) adds the <= 32 slab partials in a fixed order and finishes
// da_g = rstd (dxhat - s1/Ch - xhat s2/Ch) GELU'(a_g) in place.  dw, dbias, dgamma and dbeta are sums over (b, t): a
// workgroup walks several tiles with its accumulators in registers, the 8 waves are added in wave order through LDS, the
// workgroup's [64, K + 3] partial goes to the workspace and a last kernel adds the partials in order into the
// gradients.  No atomics and no waiting between workgroups anywhere: every result is bit-identical from launch to launch.
#include "common.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int NWV = 8;             // waves per workgroup of the tile kernels
constexpr int TB = NWV * 8;        // frames per tile
constexpr int CSGU_KMAX = 31;
constexpr int CSGU_CMAX = 2048;

__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }
// d/dx [x Phi(x)] = Phi(x) + x phi(x)
__device__ __forceinline__ float dgelu(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * expf(-0.5f * x * x);
}

// stats[row] = (mean, rstd) of GELU(a[row, Ch:]).  One wave per row, the row's <= 2048 gate values in registers.
__global__ __launch_bounds__(256) void csgu_stats_kernel(const float* __restrict__ a, float* __restrict__ stats, long rows,
                                                         int C, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nq = C / 4;
  const float4* g4 = reinterpret_cast<const float4*>(a + row * 2 * C + C);
  float4 v[CSGU_CMAX / 256];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < CSGU_CMAX / 256; ++i) {
    const int q = lane + i * 64;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < nq) {
      const float4 t = g4[q];
      v[i] = make_float4(gelu(t.x), gelu(t.y), gelu(t.z), gelu(t.w));
      s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  }
  const float mean = wave_sum(s) / (float)C;
  float m2 = 0.f;
#pragma unroll
  for (int i = 0; i < CSGU_CMAX / 256; ++i) {
    if (lane + i * 64 < nq) {
      const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
      m2 += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  const float var = wave_sum(m2) / (float)C;
  if (lane == 0) {
    stats[row * 2] = mean;
    stats[row * 2 + 1] = 1.f / sqrtf(var + eps);
  }
}

// The K taps of this lane's channel out of the staged [nch, K] block (zeros beyond K).
template <int KM>
__device__ __forceinline__ void load_taps(const float* wl, int ln, int K, float (&wr)[KM]) {
#pragma unroll
  for (int k = 0; k < KM; ++k) wr[k] = (k < K) ? wl[ln * K + k] : 0.f;
}

// y[b, t, c] = GELU(a_r) * (bias[c] + sum_k w[c, k] n[b, t + k - pad, c]);   grid (B * tiles, slabs), KM >= K taps unrolled
template <int KM>
__global__ __launch_bounds__(NWV * 64) void csgu_fwd_kernel(const float* __restrict__ a, const float* __restrict__ stats,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ y, int T, int C, int K) {
  constexpr int ROWS = TB + KM - 1;                  // LDS rows (upper bound of TB + K - 1)
  constexpr int NR = (ROWS + NWV - 1) / NWV;         // rows a wave loads
  __shared__ float xs[ROWS * 64];
  __shared__ float wl[64 * KM];
  // the wave index as a scalar: row numbers, bounds tests and the statistics loads then live in SGPRs
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c0 = blockIdx.y * 64, nch = min(64, C - c0);
  const bool live = lane < nch;
  const int c = c0 + min(lane, nch - 1);             // dead lanes shadow a valid channel and store nothing
  const int ntile = (T + TB - 1) / TB;
  const int b = blockIdx.x / ntile, tb0 = (blockIdx.x % ntile) * TB;
  const int pad = (K - 1) / 2, rows = TB + K - 1;
  const float* ab = a + (long)b * T * 2 * C + c;
  const float* sb = stats + (long)b * T * 2;
  const float gm = gamma[c], bt = beta[c];
  float av[NR], mu[NR], rs[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int ts = min(max(tb0 - pad + wave + i * NWV, 0), T - 1);
    av[i] = ab[(long)ts * 2 * C + C];
    mu[i] = sb[2 * ts];
    rs[i] = sb[2 * ts + 1];
  }
  for (int i = threadIdx.x; i < nch * K; i += NWV * 64) wl[i] = w[(long)c0 * K + i];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int r = wave + i * NWV, ts = tb0 - pad + r;
    if (r < rows) xs[r * 64 + lane] = (ts >= 0 && ts < T) ? fmaf((gelu(av[i]) - mu[i]) * rs[i], gm, bt) : 0.f;
  }
  __syncthreads();
  const int t0 = tb0 + wave * 8;
  if (t0 >= T) return;
  float wr[KM];
  load_taps<KM>(wl, min(lane, nch - 1), K, wr);
  float ar[8], acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ar[i] = ab[(long)min(t0 + i, T - 1) * 2 * C];
  const float bv = bias[c];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = bv;
#pragma unroll
  for (int j = 0; j < 8 + KM - 1; ++j) {
    const float v = (j < 8 + K - 1) ? xs[(wave * 8 + min(j, 8 + K - 2)) * 64 + lane] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = j - i;
      if (k >= 0 && k < KM) acc[i] += wr[k] * v;
    }
  }
  float* yb = y + (long)b * T * C + c;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (live && t0 + i < T) yb[(long)(t0 + i) * C] = gelu(ar[i]) * acc[i];
}

// The tile kernel of backward (see the head of the file).  grid (parts, slabs); workgroup `p` walks tiles
// [p * tiles_per_block, (p + 1) * tiles_per_block) of the B * ceil(T / 64) tiles.  Writes da[.., :Ch] (final),
// da[.., Ch:] = dn * gamma (finished by csgu_bwd_row_kernel), rowpart[row, slab] = (sum dxhat, sum dxhat xhat) over the
// slab's channels, and part[p, c, 0..K+2] = this workgroup's share of (dw[c, :], dbias[c], dgamma[c], dbeta[c]).
template <int KM>
__global__ __launch_bounds__(NWV * 64) void csgu_bwd_tile_kernel(
    const float* __restrict__ dy, const float* __restrict__ a, const float* __restrict__ stats, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ da,
    float* __restrict__ rowpart, float* __restrict__ part, int B, int T, int C, int K, int tiles_per_block) {
  constexpr int ROWS = TB + KM - 1;
  constexpr int NR = (ROWS + NWV - 1) / NWV;
  __shared__ float xs[ROWS * 64];        // xhat of the tile's rows + halo (later: the workgroup's [64, K + 3] sums)
  __shared__ float ds[ROWS * 64];        // dc = dy * GELU(a_r) of the same rows
  __shared__ float wl[64 * KM];
  static_assert(64 * (KM + 3) <= ROWS * 64, "the reduction buffer lives in the xhat tile");
  // the wave index as a scalar: row numbers, bounds tests and the statistics loads then live in SGPRs
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c0 = blockIdx.y * 64, nch = min(64, C - c0), nslab = gridDim.y;
  const bool live = lane < nch;
  const int c = c0 + min(lane, nch - 1);
  const int ntile = (T + TB - 1) / TB;
  const long total = (long)B * ntile;
  const int pad = (K - 1) / 2, rows = TB + K - 1, KP = K + 3;
  const float gm = gamma[c], bt = beta[c], bv = bias[c];
  for (int i = threadIdx.x; i < nch * K; i += NWV * 64) wl[i] = w[(long)c0 * K + i];
  __syncthreads();
  float wr[KM], accw[KM];
  load_taps<KM>(wl, min(lane, nch - 1), K, wr);
#pragma unroll
  for (int k = 0; k < KM; ++k) accw[k] = 0.f;
  float accb = 0.f, accg = 0.f, accbt = 0.f;
  for (int r = 0; r < tiles_per_block; ++r) {
    const long q = (long)blockIdx.x * tiles_per_block + r;
    if (q >= total) break;
    const int b = (int)(q / ntile), tb0 = (int)(q % ntile) * TB;
    const float* ab = a + (long)b * T * 2 * C + c;
    const float* gb = dy + (long)b * T * C + c;
    const float* sb = stats + (long)b * T * 2;
    float ag[NR], av[NR], dv[NR], mu[NR], rs[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int ts = min(max(tb0 - pad + wave + i * NWV, 0), T - 1);
      av[i] = ab[(long)ts * 2 * C];
      ag[i] = ab[(long)ts * 2 * C + C];
      dv[i] = gb[(long)ts * C];
      mu[i] = sb[2 * ts];
      rs[i] = sb[2 * ts + 1];
    }
    __syncthreads();                     // the previous tile is fully consumed
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int rr = wave + i * NWV, ts = tb0 - pad + rr;
      if (rr < rows) {
        const bool in = ts >= 0 && ts < T;
        xs[rr * 64 + lane] = in ? (gelu(ag[i]) - mu[i]) * rs[i] : 0.f;
        ds[(rows - 1 - rr) * 64 + lane] = in ? dv[i] * gelu(av[i]) : 0.f;       // time-reversed (see below)
      }
    }
    __syncthreads();
    const int t0 = tb0 + wave * 8;
    // dn[t] = sum_k w[k] dc[t - k + pad] walks dc backwards in time.  With the dc tile stored time-reversed, frame
    // 7 - i of this wave reads reversed rows rb + i + k: the forward pattern, served by the same tap registers in the
    // same order (a mirrored copy of the taps would cost K more registers; K is not a compile-time constant).
    const int rb = (NWV - 1 - wave) * 8;
    float g[8], cc[8], dnr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      g[i] = ds[(rows - 1 - (wave * 8 + i + pad)) * 64 + lane];
      cc[i] = bv;
      dnr[i] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8 + KM - 1; ++j) {
      const int jj = min(j, 8 + K - 2), tj = t0 - pad + j;
      const bool use = j < 8 + K - 1;
      const float nv = (use && tj >= 0 && tj < T) ? fmaf(xs[(wave * 8 + jj) * 64 + lane], gm, bt) : 0.f;   // n is zero-padded
      const float dc = use ? ds[(rb + jj) * 64 + lane] : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = j - i;
        if (k >= 0 && k < KM) {
          cc[i] += wr[k] * nv;
          dnr[i] += wr[k] * dc;
          accw[k] += g[i] * nv;
        }
      }
    }
    float dn[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) dn[i] = dnr[7 - i];
    float ar[8], dyv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int ts = min(t0 + i, T - 1);
      ar[i] = ab[(long)ts * 2 * C];
      dyv[i] = gb[(long)ts * C];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool tl = t0 + i < T;                        // wave-uniform
      const float xh = xs[(wave * 8 + i + pad) * 64 + lane];
      const float dnv = tl ? dn[i] : 0.f;
      accg += dnv * xh;
      accbt += dnv;
      accb += g[i];
      const float dx = dnv * gm;
      const float s1 = wave_sum(live ? dx : 0.f), s2 = wave_sum(live ? dx * xh : 0.f);
      if (tl) {
        const long row = (long)b * T + t0 + i;
        if (live) {
          da[row * 2 * C + c] = dyv[i] * cc[i] * dgelu(ar[i]);
          da[row * 2 * C + C + c] = dx;
        }
        if (lane == 0) {
          rowpart[(row * nslab + blockIdx.y) * 2] = s1;
          rowpart[(row * nslab + blockIdx.y) * 2 + 1] = s2;
        }
      }
    }
  }
  // the 8 waves' sums, added in wave order
  float* red = xs;
  for (int wv = 0; wv < NWV; ++wv) {
    __syncthreads();
    if (wave == wv && live) {
      float* rl = red + lane * KP;
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (k < K) rl[k] = (wv ? rl[k] : 0.f) + accw[k];
      rl[K] = (wv ? rl[K] : 0.f) + accb;
      rl[K + 1] = (wv ? rl[K + 1] : 0.f) + accg;
      rl[K + 2] = (wv ? rl[K + 2] : 0.f) + accbt;
    }
  }
  __syncthreads();
  float* pp = part + ((long)blockIdx.x * C + c0) * KP;
  for (int i = threadIdx.x; i < nch * KP; i += NWV * 64) pp[i] = red[i];
}

// da[row, Ch + c] <- rstd (dxhat - s1 / Ch - xhat s2 / Ch) GELU'(a_g), dxhat read from the same place; one wave per row
__global__ __launch_bounds__(256) void csgu_bwd_row_kernel(const float* __restrict__ a, const float* __restrict__ stats,
                                                           const float* __restrict__ rowpart, float* __restrict__ da, long rows,
                                                           int C, int nslab) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* rp = rowpart + row * nslab * 2;
  const float s1 = wave_sum(lane < nslab ? rp[2 * lane] : 0.f) / (float)C;
  const float s2 = wave_sum(lane < nslab ? rp[2 * lane + 1] : 0.f) / (float)C;
  const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
  const float4* g4 = reinterpret_cast<const float4*>(a + row * 2 * C + C);
  float4* d4 = reinterpret_cast<float4*>(da + row * 2 * C + C);
  for (int q = lane; q < C / 4; q += 64) {
    const float4 ag = g4[q], dx = d4[q];
    float4 o;
    o.x = rstd * (dx.x - s1 - (gelu(ag.x) - mean) * rstd * s2) * dgelu(ag.x);
    o.y = rstd * (dx.y - s1 - (gelu(ag.y) - mean) * rstd * s2) * dgelu(ag.y);
    o.z = rstd * (dx.z - s1 - (gelu(ag.z) - mean) * rstd * s2) * dgelu(ag.z);
    o.w = rstd * (dx.w - s1 - (gelu(ag.w) - mean) * rstd * s2) * dgelu(ag.w);
    d4[q] = o;
  }
}

// dw[c, k], dbias[c], dgamma[c], dbeta[c] += sum over the parts, in part order (one thread per element of [C, K + 3])
__global__ __launch_bounds__(256) void csgu_bwd_reduce_kernel(const float* __restrict__ part, int nparts, int C, int K,
                                                              float* __restrict__ dw, float* __restrict__ dbias,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int KP = K + 3;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)C * KP) return;
  float s = 0.f;
  for (int p = 0; p < nparts; ++p) s += part[(long)p * C * KP + idx];
  const int ch = (int)(idx / KP), j = (int)(idx % KP);
  if (j < K) dw[(long)ch * K + j] += s;
  else if (j == K) dbias[ch] += s;
  else if (j == K + 1) dgamma[ch] += s;
  else dbeta[ch] += s;
}

bool csgu_shape_ok(int C, int K) { return K >= 3 && K <= CSGU_KMAX && (K & 1) && C >= 8 && C <= CSGU_CMAX && C % 8 == 0; }

// workgroups of the backward tile kernel: about two per CU across the slabs, each walking `tpb` tiles
void csgu_bwd_geom(int B, int T, int C, long* nparts, int* tpb) {
  const long total = (long)B * ((T + TB - 1) / TB);
  const int nslab = (C + 63) / 64;
  long gx = (512 + nslab - 1) / nslab;
  if (gx > total) gx = total;
  *tpb = (int)((total + gx - 1) / gx);
  *nparts = (total + *tpb - 1) / *tpb;
}

}  // namespace

extern "C" {

int eamd_csgu_fwd(const float* a, const float* gamma, const float* beta, const float* w, const float* bias, float eps, float* y,
                  float* stats, int B, int T, int C, int K, void* stream) {
  if (!a || !gamma || !beta || !w || !bias || !y || !stats || B <= 0 || T <= 0 || C <= 0 || K <= 0) return EAMD_EINVAL;
  if (!csgu_shape_ok(C, K)) return EAMD_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)B * T;
  hipLaunchKernelGGL(csgu_stats_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a, stats, rows, C, eps);
  const dim3 grid((unsigned)(B * ((T + TB - 1) / TB)), (C + 63) / 64);
  if (K <= 15) hipLaunchKernelGGL(csgu_fwd_kernel<15>, grid, dim3(NWV * 64), 0, s, a, stats, gamma, beta, w, bias, y, T, C, K);
  else hipLaunchKernelGGL(csgu_fwd_kernel<31>, grid, dim3(NWV * 64), 0, s, a, stats, gamma, beta, w, bias, y, T, C, K);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_csgu_bwd_workspace(int B, int T, int C, int K) {
  if (B <= 0 || T <= 0) return EAMD_EINVAL;
  if (!csgu_shape_ok(C, K)) return EAMD_EUNSUPPORTED;
  long nparts;
  int tpb;
  csgu_bwd_geom(B, T, C, &nparts, &tpb);
  const long n = nparts * C * (K + 3) + (long)B * T * ((C + 63) / 64) * 2;
  return n <= 0x7fffffffL ? (int)n : EAMD_EUNSUPPORTED;
}

int eamd_csgu_bwd(const float* dy, const float* a, const float* stats, const float* gamma, const float* beta, const float* w,
                  const float* bias, float* da, float* dw, float* dbias, float* dgamma, float* dbeta, float* workspace, int B,
                  int T, int C, int K, void* stream) {
  if (!dy || !a || !stats || !gamma || !beta || !w || !bias || !da || !dw || !dbias || !dgamma || !dbeta || !workspace || B <= 0 ||
      T <= 0 || C <= 0 || K <= 0)
    return EAMD_EINVAL;
  if (eamd_csgu_bwd_workspace(B, T, C, K) < 0) return EAMD_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  long nparts;
  int tpb;
  csgu_bwd_geom(B, T, C, &nparts, &tpb);
  const int nslab = (C + 63) / 64;
  const long rows = (long)B * T;
  float* part = workspace;
  float* rowpart = workspace + nparts * C * (K + 3);
  const dim3 grid((unsigned)nparts, nslab);
  if (K <= 15)
    hipLaunchKernelGGL(csgu_bwd_tile_kernel<15>, grid, dim3(NWV * 64), 0, s, dy, a, stats, gamma, beta, w, bias, da, rowpart, part,
                       B, T, C, K, tpb);
  else
    hipLaunchKernelGGL(csgu_bwd_tile_kernel<31>, grid, dim3(NWV * 64), 0, s, dy, a, stats, gamma, beta, w, bias, da, rowpart, part,
                       B, T, C, K, tpb);
  hipLaunchKernelGGL(csgu_bwd_row_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a, stats, rowpart, da, rows, C, nslab);
  hipLaunchKernelGGL(csgu_bwd_reduce_kernel, dim3((unsigned)(((long)C * (K + 3) + 255) / 256)), dim3(256), 0, s, part, (int)nparts, C,
                     K, dw, dbias, dgamma, dbeta);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
