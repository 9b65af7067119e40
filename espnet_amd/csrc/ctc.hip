// CTC loss forward + gradient for gfx950.
// Replaces warp-ctc (tools/installers/install_warp-ctc.sh; call sites ctc.py:40-43,62-63) and
// torch.nn.CTCLoss(reduction="sum")/B (ctc.py:37-39,53-61; espnet2/asr/ctc.py:32-52): takes raw
// activations, returns sum_b(-log p(y_b|x_b)) per utterance and d(loss)/d(activations).
//
// Four launches, no host synchronisation:
//   prep       : compact padded labels (ignore_id removed) -> extended label table
//   lse_gather : one 256-thread block per (t,b) row: log-sum-exp over V (the only pass that reads the
//                whole 159 MB logits), then gathers the <=2L+1 label log-probs into a compact lattice
//   alpha_beta : one block per (b, direction): wavefront scan over T in log space, states across
//                lanes, previous column exchanged through LDS (double buffered, 1 barrier per frame)
//   grad       : one block per (t,b): softmax row minus per-label occupancies accumulated in LDS
// eamd_ctc_pit_loss (permutation-invariant CTC of S speakers, below) runs the same kernels with kPit: the gather reads each
// (speaker, utterance, frame) row once for all S label sets, the alpha scan covers the B S^2 lattices, and beta and the gradient
// only the B S lattices that the per-utterance permutation choice (ctc_pit_select_kernel) keeps.
#include <stdlib.h>
#include <type_traits>
#include "common.h"
#include "../../include/espnet_amd.h"

namespace {

__device__ __forceinline__ float lse2(float a, float b) {
  float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m));
}
// the scan's critical path: hardware exp2 / log2 forms (v_exp_f32 / v_log_f32; arguments are <= 0 resp. in [1, 3]),
// the libm-accurate chains tripled the per-frame latency of the serial T-frame recursion
__device__ __forceinline__ float lse3(float a, float b, float c) {
  float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

// one wave per utterance: 64 labels per step, kept ones compacted by ballot / popcount (a thread per utterance walked the
// Lmax labels through 100 dependent loads: 25 us at config 2)
__global__ __launch_bounds__(64) void ctc_prep_kernel(const long long* __restrict__ ys, int Lmax, int ignore_id,
                                                      int* __restrict__ lab, int* __restrict__ lablen, int B) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int n = 0;
  for (int i0 = 0; i0 < Lmax; i0 += 64) {
    const int i = i0 + lane;
    const long long y = i < Lmax ? ys[(long)b * Lmax + i] : (long long)ignore_id;
    const bool keep = i < Lmax && y != ignore_id;
    const unsigned long long m = __ballot(keep);
    if (keep) lab[(long)b * Lmax + n + __popcll(m & ((1ULL << lane) - 1ULL))] = (int)y;
    n += __popcll(m);
  }
  if (lane == 0) lablen[b] = n;
}

// kNormalized (forced alignment of rows that already are log-probabilities): no reduction, the gather reads the rows as they are.
// kGuardLabels (forced alignment): a label outside [0, V) is never read - its state gets log-probability -inf, so the utterance
// has no path (the loss keeps its unchecked gather)
// kPit (PIT loss): blockIdx.z = hypothesis speaker i, rows at x + i si; the row's log-softmax is gathered for each of the nsp label
// rows b nsp + j into lattice (i B + b) nsp + j; lse_out holds (i B + b) T + t
template <bool kNormalized, bool kGuardLabels, bool kPit = false>
__global__ __launch_bounds__(256) void ctc_lse_gather_kernel(const float* __restrict__ x, long st, long sb,
                                                             const int* __restrict__ ilen,
                                                             const int* __restrict__ lab,
                                                             const int* __restrict__ lablen, int Lmax,
                                                             float* __restrict__ lse_out, float* __restrict__ lp,
                                                             int T, int V, int Smax, int blank, long si = 0, int nsp = 1) {
  __shared__ float red[16];
  const int t = blockIdx.x, b = blockIdx.y;
  if (t >= ilen[b]) return;
  const int ib = kPit ? blockIdx.z * gridDim.y + b : b;        // row set (speaker, utterance)
  const float* xr = x + t * st + b * sb + (kPit ? blockIdx.z * si : 0);
  if constexpr (kNormalized) {
    const int S = 2 * lablen[b] + 1;
    float* lpr = lp + ((long)b * T + t) * Smax;
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
      const int l = (s & 1) ? lab[(long)b * Lmax + (s >> 1)] : blank;
      lpr[s] = (kGuardLabels && (l < 0 || l >= V)) ? -INFINITY : xr[l];
    }
    return;
  }
  // one pass over the row: running maximum and rescaled sum per thread (16-byte loads where the row allows)
  float mx = -INFINITY, se = 0.f;
  if (((reinterpret_cast<uintptr_t>(xr) & 15) == 0) && (V % 4 == 0)) {
    const float4* x4 = reinterpret_cast<const float4*>(xr);
    for (int q = threadIdx.x; q < V / 4; q += blockDim.x) {
      const float4 v = x4[q];
      const float m4 = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
      if (m4 > mx) { se *= expf(mx - m4); mx = m4; }
      se += (expf(v.x - mx) + expf(v.y - mx)) + (expf(v.z - mx) + expf(v.w - mx));
    }
  } else {
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
      const float xv = xr[v];
      if (xv > mx) { se *= expf(mx - xv); mx = xv; }
      se += expf(xv - mx);
    }
  }
  const float mt = mx;
  mx = block_max(mx, red);
  se = block_sum(mt == -INFINITY ? 0.f : se * expf(mt - mx), red);
  const float lse = mx + logf(se);
  if (threadIdx.x == 0) lse_out[(long)ib * T + t] = lse;
  for (int j = 0; j < (kPit ? nsp : 1); ++j) {
    const int r = kPit ? b * nsp + j : b;                      // label row
    const long lat = kPit ? (long)ib * nsp + j : b;            // lattice
    const int S = 2 * lablen[r] + 1;
    float* lpr = lp + (lat * T + t) * Smax;
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
      int l = (s & 1) ? lab[(long)r * Lmax + (s >> 1)] : blank;
      if constexpr (kGuardLabels) {
        if (l < 0 || l >= V) { lpr[s] = -INFINITY; continue; }
      }
      lpr[s] = xr[l] - lse;
    }
  }
}

// kCtcLoss: blockIdx.y == 0: alpha (forward), == 1: beta (backward, includes the emission at t); lattice, label row and output b
// kPitAlpha: alpha of lattice k = blockIdx.x = (i B + b) nsp + j (hypothesis i, reference j), -log p into nll[(b nsp + i) nsp + j]
// kPitBeta : beta of the lattice the permutation keeps for q = blockIdx.x = i B + b (j = perm[b nsp + i]), written to beta row q
enum { kCtcLoss = 0, kPitAlpha = 1, kPitBeta = 2 };
template <int kMode = kCtcLoss>
__global__ __launch_bounds__(1024) void ctc_alpha_beta_kernel(const float* __restrict__ lp,
                                                              const int* __restrict__ ilen,
                                                              const int* __restrict__ lab,
                                                              const int* __restrict__ lablen, int Lmax,
                                                              float* __restrict__ alpha, float* __restrict__ beta,
                                                              float* __restrict__ nll, int T, int Smax, int blank,
                                                              int nb = 1, int nsp = 1, const long long* __restrict__ perm = nullptr) {
  extern __shared__ float sh[];  // [2][Smax + 4]
  constexpr int PF = 8;
  int b = blockIdx.x, r = b;                 // utterance, label row
  long lat = b, orow = b, nslot = b;         // lattice (lp), output row, nll slot
  if constexpr (kMode == kPitAlpha) {
    const int k = blockIdx.x, j = k % nsp, i = k / (nsp * nb);
    b = (k / nsp) % nb; r = b * nsp + j; lat = k; orow = k; nslot = ((long)b * nsp + i) * nsp + j;
  } else if constexpr (kMode == kPitBeta) {
    const int q = blockIdx.x, i = q / nb;
    b = q % nb;
    const int j = (int)perm[(long)b * nsp + i];
    r = b * nsp + j; lat = (long)q * nsp + j; orow = q;
  }
  const int dir = kMode == kCtcLoss ? (int)blockIdx.y : (kMode == kPitAlpha ? 0 : 1);
  const int s = threadIdx.x;
  const int Tb = ilen[b];
  const int L = lablen[r];
  const int S = 2 * L + 1;
  const int W = Smax + 4;
  float* buf0 = sh;
  float* buf1 = sh + W;
  // pads: indices [0,1] and [S+2, S+3] hold -inf so s-1, s-2, s+1, s+2 never need bounds checks
  for (int i = threadIdx.x; i < 2 * W; i += blockDim.x) sh[i] = -INFINITY;
  __syncthreads();
  if (Tb <= 0) {
    if (dir == 0 && s == 0) nll[nslot] = (L == 0) ? 0.f : INFINITY;
    return;
  }
  const bool active = s < S;
  const int my = active ? ((s & 1) ? lab[(long)r * Lmax + (s >> 1)] : blank) : blank;
  bool skip = false;  // may take the s-2 (alpha) / s+2 (beta) transition
  if (active && (s & 1)) {
    if (dir == 0) skip = (s >= 2) && (lab[(long)r * Lmax + ((s - 2) >> 1)] != my);
    else          skip = (s + 2 < S) && (lab[(long)r * Lmax + ((s + 2) >> 1)] != my);
  }
  const float* lpb = lp + lat * T * Smax;
  float* out = (dir == 0 ? alpha : beta) + orow * T * Smax;

  if (dir == 0) {
    float cur = -INFINITY;
    if (active && s < 2) cur = lpb[s];
    if (active) { buf0[s + 2] = cur; out[s] = cur; }
    __syncthreads();
    float* prev = buf0; float* next = buf1;
    // emissions are fetched PF frames ahead (a frame's own compute + barrier is ~0.1 us, an L2 / HBM round trip
    // several times that: with one frame of look-ahead every step of the scan waited for its load)
    float er[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) er[i] = (active && 1 + i < Tb) ? lpb[(long)(1 + i) * Smax + s] : 0.f;
    for (int t0 = 1; t0 < Tb; t0 += PF) {
      float en[PF];
#pragma unroll
      for (int i = 0; i < PF; ++i) en[i] = (active && t0 + PF + i < Tb) ? lpb[(long)(t0 + PF + i) * Smax + s] : 0.f;
#pragma unroll
      for (int i = 0; i < PF; ++i) {
        const int t = t0 + i;
        if (t < Tb) {                                 // block-uniform
          if (active) {
            float a = lse3(prev[s + 2], prev[s + 1], skip ? prev[s] : -INFINITY) + er[i];
            next[s + 2] = a;
            out[(long)t * Smax + s] = a;
          }
          __syncthreads();
          float* tmp = prev; prev = next; next = tmp;
        }
      }
#pragma unroll
      for (int i = 0; i < PF; ++i) er[i] = en[i];
    }
    if (s == 0) {
      float a1 = prev[S - 1 + 2];
      float a2 = S >= 2 ? prev[S - 2 + 2] : -INFINITY;
      nll[nslot] = -lse2(a1, a2);
    }
  } else {
    float cur = -INFINITY;
    if (active && s >= S - 2) cur = lpb[(long)(Tb - 1) * Smax + s];
    if (active) { buf0[s + 2] = cur; out[(long)(Tb - 1) * Smax + s] = cur; }
    __syncthreads();
    float* prev = buf0; float* next = buf1;
    float er[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) er[i] = (active && Tb - 2 - i >= 0) ? lpb[(long)(Tb - 2 - i) * Smax + s] : 0.f;
    for (int t0 = Tb - 2; t0 >= 0; t0 -= PF) {
      float en[PF];
#pragma unroll
      for (int i = 0; i < PF; ++i) en[i] = (active && t0 - PF - i >= 0) ? lpb[(long)(t0 - PF - i) * Smax + s] : 0.f;
#pragma unroll
      for (int i = 0; i < PF; ++i) {
        const int t = t0 - i;
        if (t >= 0) {                                 // block-uniform
          if (active) {
            float a = lse3(prev[s + 2], prev[s + 3], skip ? prev[s + 4] : -INFINITY) + er[i];
            next[s + 2] = a;
            out[(long)t * Smax + s] = a;
          }
          __syncthreads();
          float* tmp = prev; prev = next; next = tmp;
        }
      }
#pragma unroll
      for (int i = 0; i < PF; ++i) er[i] = en[i];
    }
  }
}

// kPit: blockIdx.z = hypothesis speaker i (rows at x + i si, gradient at grad + i gsi); the lattice is the one the permutation
// keeps, (i B + b) nsp + perm[b nsp + i], its beta row i B + b
template <bool kPit = false>
__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ x, long st, long sb,
                                                       const int* __restrict__ ilen, const int* __restrict__ lab,
                                                       const int* __restrict__ lablen, int Lmax,
                                                       const float* __restrict__ lse, const float* __restrict__ lp,
                                                       const float* __restrict__ alpha,
                                                       const float* __restrict__ beta, const float* __restrict__ nll,
                                                       float* __restrict__ grad, long gst, long gsb, int T, int V,
                                                       int Smax, int blank, float scale, long si = 0, long gsi = 0,
                                                       int nsp = 1, const long long* __restrict__ perm = nullptr,
                                                       const float* __restrict__ gscale = nullptr) {
  extern __shared__ float occ[];  // [V]
  const int t = blockIdx.x, b = blockIdx.y;
  const int i = kPit ? (int)blockIdx.z : 0;
  float* gr = grad + t * gst + b * gsb + (kPit ? i * gsi : 0);
  if (t >= ilen[b]) {
    for (int v = threadIdx.x; v < V; v += blockDim.x) gr[v] = 0.f;
    return;
  }
  for (int v = threadIdx.x; v < V; v += blockDim.x) occ[v] = 0.f;
  __syncthreads();
  const long q = kPit ? (long)i * gridDim.y + b : b;                   // row set (speaker, utterance), beta row
  const int j = kPit ? (int)perm[(long)b * nsp + i] : 0;
  const int r = kPit ? b * nsp + j : b;                                // label row
  const long lat = kPit ? q * nsp + j : b;                             // lattice (lp, alpha)
  const int S = 2 * lablen[r] + 1;
  const long base = (lat * T + t) * Smax;
  const long bbase = (q * T + t) * Smax;
  const float nl = nll[kPit ? ((long)b * nsp + i) * nsp + j : b];
  for (int s = threadIdx.x; s < S; s += blockDim.x) {
    int l = (s & 1) ? lab[(long)r * Lmax + (s >> 1)] : blank;
    float g = expf(alpha[base + s] + beta[bbase + s] - lp[base + s] + nl);
    atomicAdd(&occ[l], g);
  }
  __syncthreads();
  const float* xr = x + t * st + b * sb + (kPit ? i * si : 0);
  const float ls = lse[q * T + t];
  if (gscale) {      // the upstream scalar, read on the device: the value a scale_dev pass over the gradient would leave
    const float gs = gscale[0];
    for (int v = threadIdx.x; v < V; v += blockDim.x) gr[v] = ((expf(xr[v] - ls) - occ[v]) * scale) * gs;
    return;
  }
  for (int v = threadIdx.x; v < V; v += blockDim.x) gr[v] = (expf(xr[v] - ls) - occ[v]) * scale;
}

// the pieces of eamd_ctc_loss's workspace (eamd_ctc_workspace_bytes)
struct CtcWs { int* lab; int* lablen; float* lse; float* lp; float* alpha; float* beta; int Lm; };
inline CtcWs ctc_ws_carve(void* workspace, int B, int T, int Lmax) {
  CtcWs r;
  const int Smax = 2 * Lmax + 1;
  char* w = (char*)workspace;
  r.Lm = Lmax > 0 ? Lmax : 1;
  r.lab = (int*)w; w += (size_t)B * r.Lm * 4;
  r.lablen = (int*)w; w += (size_t)B * 4;
  w = (char*)(((uintptr_t)w + 15) & ~(uintptr_t)15);
  r.lse = (float*)w; w += (size_t)B * T * 4;
  r.lp = (float*)w; w += (size_t)B * T * Smax * 4;
  r.alpha = (float*)w; w += (size_t)B * T * Smax * 4;
  r.beta = (float*)w;
  return r;
}

}  // namespace

extern "C" {

/* workspace bytes needed by eamd_ctc_loss */
int64_t eamd_ctc_workspace_bytes(int B, int T, int Lmax) {
  int64_t Smax = 2 * (int64_t)Lmax + 1;
  int64_t n = (int64_t)B * Lmax * 4 + (int64_t)B * 4      /* lab, lablen */
              + (int64_t)B * T * 4                          /* lse */
              + 3 * (int64_t)B * T * Smax * 4;              /* lp, alpha, beta */
  return n + 256;
}

/*
 * acts  : [T,B,V] or [B,T,V] fp32 via element strides (stride_t, stride_b); V contiguous
 * ys_pad: [B,Lmax] int64 padded with ignore_id; ilens: [B] int32 valid frames
 * nll   : [B] fp32 out (-log p per utterance, +inf if no valid alignment)
 * grad  : optional, same strides convention (gstride_t, gstride_b); = scale * d(sum_b nll_b)/d acts
 */
int eamd_ctc_loss(const float* acts, int64_t stride_t, int64_t stride_b, const int64_t* ys_pad,
                  const int32_t* ilens, float* nll, float* grad, int64_t gstride_t, int64_t gstride_b,
                  void* workspace, int B, int T, int V, int Lmax, int blank, int ignore_id, float grad_scale,
                  void* stream) {
  if (!acts || !ys_pad || !ilens || !nll || !workspace || B <= 0 || T <= 0 || V <= 0 || Lmax < 0) return EAMD_EINVAL;
  const int Smax = 2 * Lmax + 1;
  int threads = ((Smax + 63) / 64) * 64;
  if (threads > 1024) return EAMD_EUNSUPPORTED;
  if (grad && (size_t)V * 4 > 64 * 1024) return EAMD_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const CtcWs ws = ctc_ws_carve(workspace, B, T, Lmax);
  int* lab = ws.lab; int* lablen = ws.lablen;
  float* lse = ws.lse; float* lp = ws.lp; float* alpha = ws.alpha; float* beta = ws.beta;
  const int Lm = ws.Lm;

  hipLaunchKernelGGL(ctc_prep_kernel, dim3(B), dim3(64), 0, s, (const long long*)ys_pad, Lmax, ignore_id, lab, lablen, B);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((ctc_lse_gather_kernel<false, false>), dim3(T, B), dim3(256), 0, s, acts, (long)stride_t, (long)stride_b, ilens,
                     lab, lablen, Lm, lse, lp, T, V, Smax, blank, 0L, 1);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_alpha_beta_kernel<kCtcLoss>, dim3(B, 2), dim3(threads), 2 * (Smax + 4) * sizeof(float), s, lp, ilens,
                     lab, lablen, Lm, alpha, beta, nll, T, Smax, blank, 1, 1, nullptr);
  EAMD_LAUNCH_CHECK();
  if (grad) {
    hipLaunchKernelGGL(ctc_grad_kernel<false>, dim3(T, B), dim3(256), (size_t)V * sizeof(float), s, acts, (long)stride_t,
                       (long)stride_b, ilens, lab, lablen, Lm, lse, lp, alpha, beta, nll, grad, (long)gstride_t,
                       (long)gstride_b, T, V, Smax, blank, grad_scale, 0L, 0L, 1, nullptr);
    EAMD_LAUNCH_CHECK();
  }
  return EAMD_OK;
}


/* gradient pass alone, from the workspace a previous eamd_ctc_loss call (grad = NULL) on the same acts / ilens filled:
 * lets the caller run it in backward and fold the upstream scalar, read from device memory, into the one pass */
int eamd_ctc_grad(const float* acts, int64_t stride_t, int64_t stride_b, const int32_t* ilens, const float* nll, float* grad,
                  int64_t gstride_t, int64_t gstride_b, const void* workspace, int B, int T, int V, int Lmax, int blank,
                  float grad_scale, const float* gscale_dev, void* stream) {
  if (!acts || !ilens || !nll || !grad || !workspace || B <= 0 || T <= 0 || V <= 0 || Lmax < 0) return EAMD_EINVAL;
  const int Smax = 2 * Lmax + 1;
  if (((Smax + 63) / 64) * 64 > 1024) return EAMD_EUNSUPPORTED;
  if ((size_t)V * 4 > 64 * 1024) return EAMD_EUNSUPPORTED;
  const CtcWs ws = ctc_ws_carve((void*)workspace, B, T, Lmax);
  hipLaunchKernelGGL(ctc_grad_kernel<false>, dim3(T, B), dim3(256), (size_t)V * sizeof(float), (hipStream_t)stream, acts,
                     (long)stride_t, (long)stride_b, ilens, ws.lab, ws.lablen, ws.Lm, ws.lse, ws.lp, ws.alpha, ws.beta, nll, grad,
                     (long)gstride_t, (long)gstride_b, T, V, Smax, blank, grad_scale, 0L, 0L, 1, (const long long*)nullptr,
                     gscale_dev);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Permutation-invariant CTC of S = 2 or 3 speakers (PIT).  reference: e2e_asr_mix_transformer.py:116-135 (S^2 CTC calls, each
// with its own log-softmax of the same speaker's logits), e2e_asr_mix.py:48-108 (PIT: the best permutation per utterance, on
// the host).  Here five launches on the caller's stream, no host synchronisation:
//   prep       : ctc_prep_kernel over the B S label rows (ys_pad [B, S, Lmax] is B S rows of Lmax)
//   lse_gather : ctc_lse_gather_kernel<kPit>, one block per (t, b, i): the log-softmax of the row once, the 2L+1 emissions of each
//                of the S label sets
//   alpha      : ctc_alpha_beta_kernel<kPitAlpha>, one block per lattice (i, b, j): B S^2 scans in one launch
//   select     : ctc_pit_select_kernel, one thread per utterance: the S! permutation scores, perm and pit
//   beta, grad : ctc_alpha_beta_kernel<kPitBeta> and ctc_grad_kernel<kPit> for the B S lattices kept
// ---------------------------------------------------------------------------------------------
namespace {
// the reference's PIT.permutationDFS order (swap-based depth first search, not lexicographic)
__constant__ int kPitPerm2[2][2] = {{0, 1}, {1, 0}};
__constant__ int kPitPerm3[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 1, 0}, {2, 0, 1}};

// PIT.min_pit_sample in its fp32 arithmetic: score(p) = (sum_i in order (nll[i, p[i]] / B)) / S, the first minimum wins (torch.min)
template <int NS>
__global__ __launch_bounds__(64) void ctc_pit_select_kernel(const float* __restrict__ nll, long long* __restrict__ perm,
                                                            float* __restrict__ pit, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  constexpr int NP = NS == 2 ? 2 : 6;
  const float* n = nll + (long)b * NS * NS;
  const float fb = (float)B;
  float best = 0.f;
  int arg = -1;
  for (int k = 0; k < NP; ++k) {
    float sc = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int j = NS == 2 ? kPitPerm2[k][i] : kPitPerm3[k][i];
      const float v = n[i * NS + j] / fb;
      sc = i == 0 ? v : sc + v;
    }
    sc = sc / (float)NS;
    if (arg < 0 || sc < best || (sc != sc && best == best)) { best = sc; arg = k; }     // NaN propagates, as torch.min
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) perm[(long)b * NS + i] = NS == 2 ? kPitPerm2[arg][i] : kPitPerm3[arg][i];
  pit[b] = best;
}
}  // namespace

extern "C" {

/* workspace bytes needed by eamd_ctc_pit_loss */
int64_t eamd_ctc_pit_workspace_bytes(int S, int B, int T, int Lmax) {
  const int64_t Lm = Lmax > 0 ? Lmax : 1;
  const int64_t Smax = 2 * (int64_t)Lmax + 1;
  const int64_t R = (int64_t)B * S;                                  /* label rows, (speaker, utterance) row sets */
  return R * Lm * 4 + R * 4 + 16                                     /* lab, lablen (+ alignment) */
         + R * T * 4                                                 /* lse */
         + 2 * R * S * T * Smax * 4                                  /* lp, alpha of the B S^2 lattices */
         + R * T * Smax * 4                                          /* beta of the B S kept */
         + 256;
}

/*
 * acts    : [S, B, T, V] fp32 raw activations (speaker-major, V contiguous); ys_pad [B, S, Lmax] int64 padded with ignore_id;
 * ilens   : [B] int32 (the frames of every speaker of utterance b)
 * nll_pair: [B, S, S] out, -log p of hypothesis i against reference j (+inf where infeasible)
 * perm    : [B, S] int64 out, the reference assigned to hypothesis i;  pit: [B] out, the chosen permutation's score
 * grad    : optional [S, B, T, V] = grad_scale * d(sum_b sum_i nll_pair[b, i, perm[b, i]]) / d acts (zero past ilens)
 */
int eamd_ctc_pit_loss(const float* acts, const int64_t* ys_pad, const int32_t* ilens, float* nll_pair, int64_t* perm, float* pit,
                      float* grad, void* workspace, int S, int B, int T, int V, int Lmax, int blank, int ignore_id, float grad_scale,
                      void* stream) {
  if (!acts || !ys_pad || !ilens || !nll_pair || !perm || !pit || !workspace || B <= 0 || T <= 0 || V <= 0 || Lmax < 0)
    return EAMD_EINVAL;
  if (S != 2 && S != 3) return EAMD_EUNSUPPORTED;
  const int Smax = 2 * Lmax + 1;
  const int threads = ((Smax + 63) / 64) * 64;
  if (threads > 1024) return EAMD_EUNSUPPORTED;
  if (grad && (size_t)V * 4 > 64 * 1024) return EAMD_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int Lm = Lmax > 0 ? Lmax : 1;
  const size_t R = (size_t)B * S;
  char* w = (char*)workspace;
  int* lab = (int*)w; w += R * Lm * 4;
  int* lablen = (int*)w; w += R * 4;
  w = (char*)(((uintptr_t)w + 15) & ~(uintptr_t)15);
  float* lse = (float*)w; w += R * T * 4;
  float* lp = (float*)w; w += R * S * T * Smax * 4;
  float* alpha = (float*)w; w += R * S * T * Smax * 4;
  float* beta = (float*)w;
  const long sb = (long)T * V, si = (long)B * T * V;

  hipLaunchKernelGGL(ctc_prep_kernel, dim3(R), dim3(64), 0, s, (const long long*)ys_pad, Lmax, ignore_id, lab, lablen, (int)R);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((ctc_lse_gather_kernel<false, false, true>), dim3(T, B, S), dim3(256), 0, s, acts, (long)V, sb, ilens, lab,
                     lablen, Lm, lse, lp, T, V, Smax, blank, si, S);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_alpha_beta_kernel<kPitAlpha>, dim3(R * S), dim3(threads), 2 * (Smax + 4) * sizeof(float), s, lp, ilens,
                     lab, lablen, Lm, alpha, beta, nll_pair, T, Smax, blank, B, S, nullptr);
  EAMD_LAUNCH_CHECK();
  if (S == 2)
    hipLaunchKernelGGL(ctc_pit_select_kernel<2>, dim3((B + 63) / 64), dim3(64), 0, s, nll_pair, (long long*)perm, pit, B);
  else
    hipLaunchKernelGGL(ctc_pit_select_kernel<3>, dim3((B + 63) / 64), dim3(64), 0, s, nll_pair, (long long*)perm, pit, B);
  EAMD_LAUNCH_CHECK();
  if (grad) {
    hipLaunchKernelGGL(ctc_alpha_beta_kernel<kPitBeta>, dim3(R), dim3(threads), 2 * (Smax + 4) * sizeof(float), s, lp, ilens,
                       lab, lablen, Lm, alpha, beta, nll_pair, T, Smax, blank, B, S, (const long long*)perm);
    EAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_grad_kernel<true>, dim3(T, B, S), dim3(256), (size_t)V * sizeof(float), s, acts, (long)V, sb, ilens,
                       lab, lablen, Lm, lse, lp, alpha, beta, nll_pair, grad, (long)V, sb, T, V, Smax, blank, grad_scale, si, si,
                       S, (const long long*)perm);
    EAMD_LAUNCH_CHECK();
  }
  return EAMD_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// CTC forced alignment (Viterbi over the extended-label lattice).  reference: ctc.py:153-216 (CTC.forced_align, one utterance,
// numpy loop over frames x states); here a batch, on the caller's stream, four launches:
//   prep          : ctc_prep_kernel (labels compacted)
//   lse_gather    : ctc_lse_gather_kernel<normalized, true> (log-softmax over V and the 2L+1 state emissions; normalized rows:
//                   gather only; a label outside [0, V) gets -inf instead of a read)
//   viterbi       : one workgroup per utterance: the max-plus scan of ctc_alpha_beta_kernel's alpha recursion (a thread owns 4
//                   consecutive states, the previous column's last two states of each thread exchanged through LDS, one barrier
//                   per frame, emissions prefetched PF frames ahead), backpointers as one byte per (t, s) into the workspace
//   backtrack     : one wave per utterance: the walk back from the end state, writing states, tokens and segment bounds.
// Recursion and tie-break as the reference: delta[t,s] = max(stay, s-1, s-2 where allowed) + lp[t,s] in fp32 (first maximum:
// stay before s-1 before s-2), end state S-1 before S-2.  Departures: state 0 has no s-1 (numpy reads index -1 there, the last
// state), an infeasible pair (T_b < L_b + adjacent repeats) gives score -inf and -1 outputs, L_b = 0 gives the all-blank path.
// ---------------------------------------------------------------------------------------------
namespace {
constexpr int kAlignMaxThreads = 1024;            // 4 states per thread: S <= 4096

__global__ __launch_bounds__(kAlignMaxThreads) void ctc_viterbi_kernel(const float* __restrict__ lp, const int* __restrict__ ilen,
                                                                        const int* __restrict__ lab, const int* __restrict__ lablen,
                                                                        int Lmax, int Lout, unsigned char* __restrict__ bp,
                                                                        float* __restrict__ score, int* __restrict__ endst,
                                                                        int* __restrict__ states, long long* __restrict__ tokens,
                                                                        int* __restrict__ seg_start, int* __restrict__ seg_end, int T,
                                                                        int Spad, int blank) {
  __shared__ float2 xch[2][kAlignMaxThreads + 1];   // [buffer][1 + thread]: states 4 tid + 2, 4 tid + 3; slot 0 = (-inf, -inf)
  __shared__ float endv[2];
  constexpr int PF = 8;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int Tb = min(ilen[b], T);
  const int L = lablen[b];
  const int S = 2 * L + 1;
  const int s0 = 4 * tid;
  int* st_b = states + (long)b * T;
  long long* tk_b = tokens + (long)b * T;
  int* ss_b = seg_start + (long)b * Lout;
  int* se_b = seg_end + (long)b * Lout;
  const int* lab_b = lab + (long)b * Lmax;
  // frames behind the utterance and label slots behind its labels: -1
  for (int t = max(Tb, 0) + tid; t < T; t += nt) { st_b[t] = -1; tk_b[t] = -1; }
  for (int i = L + tid; i < Lout; i += nt) { ss_b[i] = -1; se_b[i] = -1; }
  if (Tb <= 0) {
    if (tid == 0) score[b] = L == 0 ? 0.f : -INFINITY;
    for (int i = tid; i < min(L, Lout); i += nt) { ss_b[i] = -1; se_b[i] = -1; }
    return;
  }
  const bool active = s0 < S;
  // the transitions each of the 4 states may take: s-2 only for a label state whose label differs from the one before it
  unsigned skip = 0;
  if (active) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int s = s0 + k;
      if ((s & 1) && s >= 3 && s < S) {
        const int y = lab_b[s >> 1];
        if (y != blank && y != lab_b[(s - 2) >> 1]) skip |= 1u << k;
      }
    }
  }
  const float* lpb = lp + (long)b * T * Spad;
  unsigned* bpw = reinterpret_cast<unsigned*>(bp + (long)b * T * Spad);
  const long rw = Spad / 4;                        // 4-state words per frame
  float d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = (s0 + k < 2 && s0 + k < S) ? lpb[s0 + k] : -INFINITY;
  if (tid == 0) { xch[0][0] = make_float2(-INFINITY, -INFINITY); xch[1][0] = make_float2(-INFINITY, -INFINITY); }
  xch[0][tid + 1] = make_float2(d[2], d[3]);
  __syncthreads();
  int p = 0;
  const float4* lp4 = reinterpret_cast<const float4*>(lpb) + tid;
  float4 er[PF];
#pragma unroll
  for (int i = 0; i < PF; ++i) er[i] = (active && 1 + i < Tb) ? lp4[(1 + i) * rw] : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t0 = 1; t0 < Tb; t0 += PF) {
    float4 en[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) en[i] = (active && t0 + PF + i < Tb) ? lp4[(t0 + PF + i) * rw] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int t = t0 + i;
      if (t < Tb) {                                  // block-uniform
        const float2 nb = xch[p][tid];              // previous column, states s0 - 2 and s0 - 1
        const float prv[6] = {nb.x, nb.y, d[0], d[1], d[2], d[3]};
        const float e[4] = {er[i].x, er[i].y, er[i].z, er[i].w};
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float best = prv[k + 2];
          unsigned off = 0;
          if (prv[k + 1] > best) { best = prv[k + 1]; off = 1; }
          if (((skip >> k) & 1u) && prv[k] > best) { best = prv[k]; off = 2; }
          d[k] = (s0 + k < S) ? best + e[k] : -INFINITY;
          word |= off << (8 * k);
        }
        if (active) bpw[t * rw + tid] = word;
        xch[p ^ 1][tid + 1] = make_float2(d[2], d[3]);
        __syncthreads();
        p ^= 1;
      }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) er[i] = en[i];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (s0 + k == S - 1) endv[0] = d[k];
    if (s0 + k == S - 2) endv[1] = d[k];
  }
  __syncthreads();
  if (tid == 0) {
    const float e1 = endv[0], e2 = S >= 2 ? endv[1] : -INFINITY;
    const float best = e2 > e1 ? e2 : e1;
    score[b] = best;
    endst[b] = best == -INFINITY ? -1 : (e2 > e1 ? S - 2 : S - 1);     // -1: no CTC path of Tb frames spells these labels
  }
}

// the walk back through the backpointers: one wave per utterance, lane 0 follows the chain (one dependent byte load per frame)
// and writes states, tokens and the segment bounds as it goes; an utterance without a path gets -1 everywhere
__global__ __launch_bounds__(64) void ctc_backtrack_kernel(const unsigned char* __restrict__ bp, const int* __restrict__ ilen,
                                                           const int* __restrict__ lab, const int* __restrict__ lablen, int Lmax,
                                                           int Lout, const int* __restrict__ endst, int* __restrict__ states,
                                                           long long* __restrict__ tokens, int* __restrict__ seg_start,
                                                           int* __restrict__ seg_end, int T, int Spad, int blank) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = min(ilen[b], T);
  if (Tb <= 0) return;                               // (the scan wrote every output of an empty utterance)
  const int L = lablen[b];
  int* st_b = states + (long)b * T;
  long long* tk_b = tokens + (long)b * T;
  int* ss_b = seg_start + (long)b * Lout;
  int* se_b = seg_end + (long)b * Lout;
  const int send = endst[b];
  if (send < 0) {
    for (int t = lane; t < Tb; t += 64) { st_b[t] = -1; tk_b[t] = -1; }
    for (int i = lane; i < min(L, Lout); i += 64) { ss_b[i] = -1; se_b[i] = -1; }
    return;
  }
  if (lane != 0) return;
  const int* lab_b = lab + (long)b * Lmax;
  const unsigned char* bpb = bp + (long)b * T * Spad;
  int s = send, nxt = -1;                            // nxt: the state at t + 1
  for (int t = Tb - 1; t >= 0; --t) {
    st_b[t] = s;
    tk_b[t] = (s & 1) ? lab_b[s >> 1] : blank;
    if ((s & 1) && nxt != s) se_b[s >> 1] = t;
    if (nxt >= 0 && (nxt & 1) && nxt != s) ss_b[nxt >> 1] = t + 1;
    nxt = s;
    if (t > 0) s -= bpb[(long)t * Spad + s];
  }
  if (nxt & 1) ss_b[nxt >> 1] = 0;
}
}  // namespace

extern "C" {

/* workspace bytes needed by eamd_ctc_forced_align */
int64_t eamd_ctc_align_workspace_bytes(int B, int T, int Lmax) {
  const int64_t Lm = Lmax > 0 ? Lmax : 1;
  const int64_t Spad = (2 * (int64_t)Lmax + 1 + 3) / 4 * 4;
  return (int64_t)B * Lm * 4 + (int64_t)B * 4 + 16      /* lab, lablen (+ alignment) */
         + (int64_t)B * T * 4 + 16                      /* lse (+ alignment) */
         + (int64_t)B * T * Spad * 4                    /* lp */
         + (int64_t)B * T * Spad                        /* backpointers */
         + (int64_t)B * 4                               /* end states */
         + 256;
}

int eamd_ctc_forced_align(const float* acts, int64_t stride_t, int64_t stride_b, const int64_t* ys_pad, const int32_t* ilens,
                          float* score, int32_t* states, int64_t* tokens, int32_t* seg_start, int32_t* seg_end, void* workspace,
                          int B, int T, int V, int Lmax, int blank, int ignore_id, int normalized, void* stream) {
  if (!acts || !ys_pad || !ilens || !score || !states || !tokens || !seg_start || !seg_end || !workspace || B <= 0 || T <= 0 ||
      V <= 0 || Lmax < 0 || blank < 0 || blank >= V)
    return EAMD_EINVAL;
  const int Smax = 2 * Lmax + 1;
  if (Smax > 4 * kAlignMaxThreads) return EAMD_EUNSUPPORTED;
  const int Spad = (Smax + 3) / 4 * 4;
  const int threads = ((Spad / 4 + 63) / 64) * 64;
  hipStream_t s = (hipStream_t)stream;
  const int Lm = Lmax > 0 ? Lmax : 1;
  char* w = (char*)workspace;
  int* lab = (int*)w; w += (size_t)B * Lm * 4;
  int* lablen = (int*)w; w += (size_t)B * 4;
  w = (char*)(((uintptr_t)w + 15) & ~(uintptr_t)15);
  float* lse = (float*)w; w += (size_t)B * T * 4;
  w = (char*)(((uintptr_t)w + 15) & ~(uintptr_t)15);
  float* lp = (float*)w; w += (size_t)B * T * Spad * 4;     // rows of Spad (% 4 == 0) floats: a thread's 4 states are one 16-byte load
  unsigned char* bp = (unsigned char*)w; w += (size_t)B * T * Spad;
  int* endst = (int*)w;                              // (B T Spad is a multiple of 4)

  hipLaunchKernelGGL(ctc_prep_kernel, dim3(B), dim3(64), 0, s, (const long long*)ys_pad, Lmax, ignore_id, lab, lablen, B);
  EAMD_LAUNCH_CHECK();
  if (normalized)
    hipLaunchKernelGGL((ctc_lse_gather_kernel<true, true>), dim3(T, B), dim3(256), 0, s, acts, (long)stride_t, (long)stride_b, ilens,
                       lab, lablen, Lm, nullptr, lp, T, V, Spad, blank, 0L, 1);
  else
    hipLaunchKernelGGL((ctc_lse_gather_kernel<false, true>), dim3(T, B), dim3(256), 0, s, acts, (long)stride_t, (long)stride_b, ilens,
                       lab, lablen, Lm, lse, lp, T, V, Spad, blank, 0L, 1);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_viterbi_kernel, dim3(B), dim3(threads), 0, s, lp, ilens, lab, lablen, Lm, Lmax, bp, score, endst, states,
                     (long long*)tokens, seg_start, seg_end, T, Spad, blank);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_backtrack_kernel, dim3(B), dim3(64), 0, s, bp, ilens, lab, lablen, Lm, Lmax, endst, states,
                     (long long*)tokens, seg_start, seg_end, T, Spad, blank);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// CTC prefix scoring for joint CTC/attention beam search (Watanabe et al. 2017, Algorithm 2).
// reference: espnet/nets/ctc_prefix_score.py:224-310 (CTCPrefixScore.__call__), :157-162 (the per-frame
// loop of CTCPrefixScoreTH).  One thread = one (hypothesis, candidate token): sequential scan over the
// T frames in log space; candidates of one hypothesis share the broadcast r_prev reads.
//   logp   [T, V]                  frame log-posteriors (CTC.log_softmax)
//   r_prev [nhyp, T, 2]            (r^n, r^b) of each hypothesis prefix
//   cand   [nhyp, ncand] int32     tokens to score;  last[nhyp], olen[nhyp] = last token / prefix length-1
//   psi    [nhyp, ncand]           log prefix probabilities;  r_new [nhyp, ncand, T, 2]
// ---------------------------------------------------------------------------------------------
namespace {
constexpr float kLogZero = -10000000000.0f;
// numpy.logaddexp for the prefix recursion: 249 frames x 4 of these in ONE wave's dependent chain - with the library expf / log1pf
// (~100 instructions each) a search step spent 345 us here.  Hardware exp2 / log2 (1 ulp each) instead; log1p(e) below 2^-12 by its
// series (1 + e would round the term away).  Absolute error of one call <= 1.2e-7 on values of magnitude 1 .. 100.
__device__ __forceinline__ float lae(float a, float b) {
  const float m = fmaxf(a, b);
  const float e = a == b ? 1.f : __expf(-fabsf(a - b));     // equal operands incl. (-inf, -inf): log 2 on top of m, not NaN
  const float l = e < 2.44140625e-4f ? e * (1.f - 0.5f * e) : __logf(1.f + e);
  return m + l;
}
// The frame-by-frame recursion of one (prefix, token) pair, written ONCE for every kernel that walks it: rp = (r^n, r^b) of the
// prefix, rn = those of prefix + c; ol = prefix length - 1, already clamped to 0 .. T; same = c repeats the prefix's last token.
// Returns log psi before the <eos> / blank fix-up (a caller that only wants the state drops it, and its log-add chain with it).
// NB = groups of PF frames in flight.  With one group phi is formed as the rows arrive, so a group holds it instead of the two
// rows it is made of (8 registers less); with the ring it is formed when the group is walked.
template <int NB>
__device__ __forceinline__ float ctc_prefix_recursion(const float* __restrict__ logp, const float* __restrict__ rp,
                                                      float* __restrict__ rn, int T, int V, int c, int blank, int ol, bool same) {
  __builtin_assume(T > 0 && V > 0);      // (every caller has checked or clamped them: row offsets t * V stay one scalar multiply)
  const int start = max(ol, 1);
  // rows before start-1 are never read by later steps; keep them at log-zero like the reference's r
  for (int t = 0; t < min(start - 1, T); ++t) *reinterpret_cast<float2*>(rn + 2 * t) = make_float2(kLogZero, kLogZero);
  float rn_n = ol == 0 ? logp[c] : kLogZero, rn_b = kLogZero;
  if (start - 1 < T) *reinterpret_cast<float2*>(rn + 2 * (start - 1)) = make_float2(rn_n, rn_b);
  float lpsi = rn_n;
  // the recursion over t is serial, its operands are not: the posteriors and the previous prefix's rows of the next PF frames
  // are requested together (each logp row is its own cache line, 20 KB apart: fetched inside the chain every frame cost a
  // memory round trip - 344 us for 249 frames), and only the log-add chain stays serial.
  // Same operations in the same order as a plain loop over the frames: results bit for bit.
  // ... and a RING of NB such groups is kept in flight (the group NB - 1 ahead is requested before the current one is walked).
  // Measured at config 2 (249 frames, 10 hypotheses x 15 candidates): 152 us with one group in flight, 157 us with the ring and
  // 8-byte state stores - neither the round trips nor the stores bound this kernel: it is ONE wave per hypothesis walking a
  // dependent chain of ~60 VALU + 8 transcendental instructions per frame with nothing else on its SIMD (0.6 us per frame).
  constexpr int PF = 8;
  constexpr bool kPhiOnArrival = NB == 1;
  float xv[NB][PF], bv[NB][PF], pn[NB][PF], pb[NB][PF];      // slots are indexed by unrolled constants only: registers
  auto phi_of = [&](float n_, float b_) __attribute__((always_inline)) { return same ? b_ : lae(n_, b_); };
  auto request = [&](int sl, int t0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int t = min(max(t0 + q, 1), T - 1);          // (frames behind the end: the last one again; T = 1: frame 0, never walked)
      const int tp = max(t - 1, 0);
      xv[sl][q] = logp[(long)t * V + c];
      bv[sl][q] = logp[(long)t * V + blank];
      pn[sl][q] = rp[2 * tp];
      pb[sl][q] = rp[2 * tp + 1];
      if (kPhiOnArrival) pb[sl][q] = phi_of(pn[sl][q], pb[sl][q]);      // (pn is then dead)
    }
  };
  auto walk = [&](int sl, int t0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int t = t0 + q;
      if (t < T) {
        const float phi = kPhiOnArrival ? pb[sl][q] : phi_of(pn[sl][q], pb[sl][q]);
        const float nn = lae(rn_n, phi) + xv[sl][q];
        const float nb = lae(rn_n, rn_b) + bv[sl][q];
        lpsi = lae(lpsi, phi + xv[sl][q]);
        rn_n = nn; rn_b = nb;
        *reinterpret_cast<float2*>(rn + 2 * t) = make_float2(nn, nb);        // one 8-byte store per frame
      }
    }
  };
  if constexpr (NB == 1) {      // (spelled out: as a ring of one the same loop is allocated 7 registers more)
    for (int t0 = start; t0 < T; t0 += PF) { request(0, t0); walk(0, t0); }
  } else {
#pragma unroll
    for (int k = 0; k < NB - 1; ++k) request(k, start + k * PF);
    for (int t0 = start; t0 < T; t0 += NB * PF) {
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        request((k + NB - 1) % NB, t0 + (k + NB - 1) * PF);
        walk(k, t0 + k * PF);
      }
    }
  }
  return lpsi;
}
// One thread = one (hypothesis, candidate) of SEVERAL utterances in one launch: hypothesis h belongs to utterance h / per_utt,
// whose posteriors are logp[u] ([Tmax, V], lens[u] valid frames); r_prev / r_new rows are padded to Tmax (rows from lens[u] on
// are never read).  lens == nullptr: every utterance has Tmax frames (eamd_ctc_prefix_score: one utterance, per_utt = nhyp).
__global__ void ctc_prefix_batch_kernel(const float* __restrict__ logp_all, const int* __restrict__ lens, int per_utt,
                                        const float* __restrict__ r_prev, const int* __restrict__ cand,
                                        const int* __restrict__ last, const int* __restrict__ olen, float* __restrict__ psi,
                                        float* __restrict__ r_new, int Tmax, int V, int ncand, int blank, int eos) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int h = blockIdx.y;
  if (j >= ncand) return;
  const int u = h / per_utt;
  const int T = lens ? min(max(lens[u], 1), Tmax) : Tmax;   // a length outside 1 .. Tmax never becomes an address
  const float* logp = logp_all + (long)u * Tmax * V;
  const int c = cand[(long)h * ncand + j];
  // a candidate outside the vocabulary is never dereferenced: its score is NaN (a selection treats NaN as -inf), its state untouched
  if (c < 0 || c >= V) { psi[(long)h * ncand + j] = __builtin_nanf(""); return; }
  const float* rp = r_prev + (long)h * Tmax * 2;
  const int ol = min(max(olen[h], 0), T);
  float lpsi = ctc_prefix_recursion<4>(logp, rp, r_new + ((long)h * ncand + j) * Tmax * 2, T, V, c, blank, ol, ol > 0 && last[h] == c);
  if (c == eos) lpsi = lae(rp[2 * (T - 1)], rp[2 * (T - 1) + 1]);
  if (c == blank) lpsi = kLogZero;
  psi[(long)h * ncand + j] = lpsi;
}
}  // namespace

// ---- the same scores without the serial chain on a beam step's critical path ------------------------------------------------
// log psi of a candidate is logsumexp over t of (phi(t-1) + x(t)) (ctc_prefix_score.py:290-296: log_psi never reads r[t]): a
// PARALLEL reduction over the frames.  Only the forward variables r^n / r^b of the NEXT step need the frame-by-frame recursion,
// and only for the `beam` continuations that survive the selection - so a step scores its candidates with ctc_prefix_psi_kernel
// (one wave per (hypothesis, candidate), lanes over frames) and the survivors' states are made by ctc_prefix_state_kernel at the
// START of the next step, on a second stream beside the decoder stack (160 us of serial recursion off the critical path).
namespace {
template <int NT>      // frames per lane: 64 NT >= Tmax
__global__ __launch_bounds__(64) void ctc_prefix_psi_kernel(const float* __restrict__ logp_all, const int* __restrict__ lens, int per_utt,
                                                            const float* __restrict__ r_prev, const int* __restrict__ cand,
                                                            const int* __restrict__ last, int ol, float* __restrict__ psi, int Tmax,
                                                            int V, int ncand, int blank, int eos, const int* __restrict__ ol_dev) {
  if (ol_dev) ol = ol_dev[0] + ol;                       // the prefix length from the device step index (+ host offset)
  const int j = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
  const int u = h / per_utt;
  const int T = min(max(lens[u], 1), Tmax);
  const float* logp = logp_all + (long)u * Tmax * V;
  const int c = cand[(long)h * ncand + j];
  if (c < 0 || c >= V) { if (lane == 0) psi[(long)h * ncand + j] = __builtin_nanf(""); return; }
  const float* rp = r_prev + (long)h * Tmax * 2;
  ol = min(max(ol, 0), T);
  const bool same = ol > 0 && last[h] == c;
  const int start = max(ol, 1);
  // terms phi(t-1) + x(t), t = start .. T-1, and the initial r[start-1, 0]; two passes: maximum, then the sum of exponentials
  float term[NT];                                  // Tmax <= 64 NT frames per wave (host check)
  float mx = (ol == 0 && lane == 0) ? logp[c] : kLogZero;
  const float init = mx;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int t = start + lane + 64 * q;
    term[q] = -INFINITY;
    if (t < T) {
      const float pn = rp[2 * (t - 1)], pb = rp[2 * (t - 1) + 1];
      const float m = fmaxf(pn, pb);
      const float phi = same ? pb : (m == -INFINITY ? -INFINITY : m + log1pf(expf(-fabsf(pn - pb))));
      term[q] = phi + logp[(long)t * V + c];
      mx = fmaxf(mx, term[q]);
    }
  }
  mx = wave_max(mx);
  float se = lane == 0 ? expf(init - mx) : 0.f;
#pragma unroll
  for (int q = 0; q < NT; ++q) se += (term[q] == -INFINITY) ? 0.f : expf(term[q] - mx);
  se = wave_sum(se);
  if (lane == 0) {
    float lpsi = mx == -INFINITY ? -INFINITY : mx + logf(se);
    if (c == eos) lpsi = lae(rp[2 * (T - 1)], rp[2 * (T - 1) + 1]);
    if (c == blank) lpsi = kLogZero;
    psi[(long)h * ncand + j] = lpsi;
  }
}

// forward variables of the surviving continuations: slot s continues the hypothesis of slot parent[s] with token tok[s]; the
// recursion (ctc_prefix_recursion) for that one (hypothesis, candidate) pair, written straight into r_out[s] ([n, Tmax, 2]).
// dead[s] != 0 (an ended or empty slot): the row is filled with log-zero.
__global__ __launch_bounds__(64) void ctc_prefix_state_kernel(const float* __restrict__ logp_all, const int* __restrict__ lens, int per_utt,
                                                              const float* __restrict__ r_prev, const long long* __restrict__ parent,
                                                              const long long* __restrict__ tok, const int* __restrict__ last, int ol,
                                                              const float* __restrict__ alive, float* __restrict__ r_out, int n, int Tmax,
                                                              int V, int blank, const int* __restrict__ ol_dev) {
  if (ol_dev) ol = ol_dev[0] + ol;
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= n) return;
  const int u = s / per_utt;
  const int T = min(max(lens[u], 1), Tmax);
  const float* logp = logp_all + (long)u * Tmax * V;
  float* rn = r_out + (long)s * Tmax * 2;
  long long hh = parent[s];
  hh = hh < 0 ? 0 : (hh >= n ? n - 1 : hh);
  const int c = (int)tok[s];
  if (c < 0 || c >= V || !(alive[s] > -INFINITY)) {                      // nothing continues in this slot
    for (int t = 0; t < T; ++t) *reinterpret_cast<float2*>(rn + 2 * t) = make_float2(kLogZero, kLogZero);
    return;
  }
  const float* rp = r_prev + hh * Tmax * 2;
  ol = min(max(ol, 0), T);
  // one group of 8 frames in flight: with the ring of four this kernel would take 128 registers more for its single wave
  ctc_prefix_recursion<1>(logp, rp, rn, T, V, c, blank, ol, ol > 0 && last[hh] == c);
}

// The same forward variables as a PARALLEL scan (Tmax <= 2048: 8 / 16 / 32 frames per lane): r^n does not read r^b -
//   r^n(t) = logaddexp(x(t) + r^n(t-1), x(t) + phi(t-1)),   then   r^b(t) = logaddexp(b(t) + r^b(t-1), b(t) + r^n(t-1))
// are two scalar recurrences s(t) = logaddexp(a(t) + s(t-1), c(t)); maps (a, c) compose as (a2 + a1, logaddexp(a2 + c1, c2)).
// One wave per slot, a lane owns Q consecutive frames: inclusive maps inside the lane, a six-step scan of the lanes' totals,
// then every frame applies its map to the state entering the lane - ~16 dependent logaddexp per recurrence instead of one per
// frame (130 us -> a few us at T = 249).  Same quantities; the order of the additions differs from the frame-by-frame recursion
// (both are within 1e-5 + 2e-6 |ref| of float64: test_ctc_prefix_score_vs_float64).
struct ScanMap { float a, c; };
__device__ __forceinline__ ScanMap scan_after(ScanMap later, ScanMap earlier) {     // later o earlier
  return ScanMap{later.a + earlier.a, lae(later.a + earlier.c, later.c)};
}
__device__ __forceinline__ ScanMap wave_scan_exclusive(ScanMap tot, int lane) {
  ScanMap inc = tot;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    ScanMap o{__shfl_up(inc.a, d, 64), __shfl_up(inc.c, d, 64)};
    if (lane >= d) inc = scan_after(inc, o);
  }
  ScanMap ex{__shfl_up(inc.a, 1, 64), __shfl_up(inc.c, 1, 64)};
  if (lane == 0) ex = ScanMap{0.f, -INFINITY};
  return ex;
}
template <int Q>       // consecutive frames per lane: 64 Q >= Tmax
__global__ __launch_bounds__(64) void ctc_prefix_state_scan_kernel(const float* __restrict__ logp_all, const int* __restrict__ lens,
                                                                   int per_utt, const float* __restrict__ r_prev,
                                                                   const long long* __restrict__ parent, const long long* __restrict__ tok,
                                                                   const int* __restrict__ last, int ol, const float* __restrict__ alive,
                                                                   float* __restrict__ r_out, int n, int Tmax, int V, int blank,
                                                                   const int* __restrict__ ol_dev) {
  if (ol_dev) ol = ol_dev[0] + ol;
  const int s = blockIdx.x, lane = threadIdx.x;
  const int u = s / per_utt;
  const int T = min(max(lens[u], 1), Tmax);
  const float* logp = logp_all + (long)u * Tmax * V;
  float* rn = r_out + (long)s * Tmax * 2;
  long long hh = parent[s];
  hh = hh < 0 ? 0 : (hh >= n ? n - 1 : hh);
  const int c = (int)tok[s];
  if (c < 0 || c >= V || !(alive[s] > -INFINITY)) {                      // nothing continues in this slot
    for (int t = lane; t < T; t += 64) *reinterpret_cast<float2*>(rn + 2 * t) = make_float2(kLogZero, kLogZero);
    return;
  }
  const float* rp = r_prev + hh * Tmax * 2;
  ol = min(max(ol, 0), T);
  const bool same = ol > 0 && last[hh] == c;
  const int start = max(ol, 1);
  for (int t = lane; t < min(start - 1, T); t += 64) *reinterpret_cast<float2*>(rn + 2 * t) = make_float2(kLogZero, kLogZero);
  const float n0 = ol == 0 ? logp[c] : kLogZero, b0 = kLogZero;
  if (lane == 0 && start - 1 < T) *reinterpret_cast<float2*>(rn + 2 * (start - 1)) = make_float2(n0, b0);
  float xv[Q], bv[Q], phi[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int t = start + Q * lane + q;
    xv[q] = 0.f; bv[q] = 0.f; phi[q] = -INFINITY;                        // past the last frame: the identity map
    if (t < T) {
      xv[q] = logp[(long)t * V + c];
      bv[q] = logp[(long)t * V + blank];
      const float2 p = *reinterpret_cast<const float2*>(rp + 2 * (t - 1));
      phi[q] = same ? p.y : lae(p.x, p.y);
    }
  }
  // r^n
  ScanMap mp[Q];
  mp[0] = ScanMap{xv[0], xv[0] + phi[0]};
#pragma unroll
  for (int q = 1; q < Q; ++q) mp[q] = scan_after(ScanMap{xv[q], xv[q] + phi[q]}, mp[q - 1]);
  ScanMap ex = wave_scan_exclusive(mp[Q - 1], lane);
  const float n_in = lae(ex.a + n0, ex.c);
  float nn[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) nn[q] = lae(mp[q].a + n_in, mp[q].c);
  // r^b
  mp[0] = ScanMap{bv[0], start + Q * lane < T ? bv[0] + n_in : -INFINITY};
#pragma unroll
  for (int q = 1; q < Q; ++q) mp[q] = scan_after(ScanMap{bv[q], start + Q * lane + q < T ? bv[q] + nn[q - 1] : -INFINITY}, mp[q - 1]);
  ex = wave_scan_exclusive(mp[Q - 1], lane);
  const float b_in = lae(ex.a + b0, ex.c);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int t = start + Q * lane + q;
    if (t < T) *reinterpret_cast<float2*>(rn + 2 * t) = make_float2(nn[q], lae(mp[q].a + b_in, mp[q].c));
  }
}
}  // namespace

extern "C" int eamd_ctc_prefix_psi_dyn(const float* logp, const int32_t* lens, int nutt, int per_utt, const float* r_prev,
                                       const int32_t* cand, const int32_t* last, int olen, const int32_t* olen_dev, float* psi, int ncand,
                                       int Tmax, int V, int blank, int eos, void* stream) {
  if (!logp || !lens || !r_prev || !cand || !last || !psi || nutt <= 0 || per_utt <= 0 || ncand <= 0 || Tmax <= 0 || V <= 0 ||
      (!olen_dev && olen < 0))
    return EAMD_EINVAL;
  const int* ol_dev = olen_dev;
  if (Tmax > 2048) return EAMD_EUNSUPPORTED;            // 8 / 16 / 32 frames per lane are held in registers
#define EAMD_PSI_(NT) hipLaunchKernelGGL(ctc_prefix_psi_kernel<NT>, dim3(ncand, nutt * per_utt), dim3(64), 0, (hipStream_t)stream, logp, lens, \
                                         per_utt, r_prev, cand, last, olen, psi, Tmax, V, ncand, blank, eos, ol_dev)
  if (Tmax <= 512) EAMD_PSI_(8);
  else if (Tmax <= 1024) EAMD_PSI_(16);
  else EAMD_PSI_(32);
#undef EAMD_PSI_
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

extern "C" int eamd_ctc_prefix_state_dyn(const float* logp, const int32_t* lens, int nutt, int per_utt, const float* r_prev,
                                         const int64_t* parent, const int64_t* tok, const int32_t* last, int olen, const int32_t* olen_dev,
                                         const float* alive, float* r_out, int Tmax, int V, int blank, void* stream) {
  if (!logp || !lens || !r_prev || !parent || !tok || !last || !alive || !r_out || nutt <= 0 || per_utt <= 0 || Tmax <= 0 || V <= 0 ||
      (!olen_dev && olen < 0))
    return EAMD_EINVAL;
  const int* ol_dev = olen_dev;
  const int n = nutt * per_utt;
  if (Tmax <= 2048) {
#define EAMD_SCAN_(Q) hipLaunchKernelGGL(ctc_prefix_state_scan_kernel<Q>, dim3(n), dim3(64), 0, (hipStream_t)stream, logp, lens, per_utt, r_prev, \
                                         (const long long*)parent, (const long long*)tok, last, olen, alive, r_out, n, Tmax, V, blank, ol_dev)
    if (Tmax <= 512) EAMD_SCAN_(8);
    else if (Tmax <= 1024) EAMD_SCAN_(16);
    else EAMD_SCAN_(32);
#undef EAMD_SCAN_
    EAMD_LAUNCH_CHECK();
    return EAMD_OK;
  }
  hipLaunchKernelGGL(ctc_prefix_state_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, logp, lens, per_utt, r_prev,
                     (const long long*)parent, (const long long*)tok, last, olen, alive, r_out, n, Tmax, V, blank, ol_dev);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

extern "C" int eamd_ctc_prefix_score_batch(const float* logp, const int32_t* lens, int nutt, int per_utt, const float* r_prev,
                                           const int32_t* cand, const int32_t* last, const int32_t* olen, float* psi,
                                           float* r_new, int ncand, int Tmax, int V, int blank, int eos, void* stream) {
  if (!logp || !lens || !r_prev || !cand || !last || !olen || !psi || !r_new || nutt <= 0 || per_utt <= 0 || ncand <= 0 ||
      Tmax <= 0 || V <= 0)
    return EAMD_EINVAL;
  hipLaunchKernelGGL(ctc_prefix_batch_kernel, dim3((ncand + 63) / 64, nutt * per_utt), dim3(64), 0, (hipStream_t)stream, logp,
                     lens, per_utt, r_prev, cand, last, olen, psi, r_new, Tmax, V, ncand, blank, eos);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

extern "C" int eamd_ctc_prefix_score(const float* logp, const float* r_prev, const int32_t* cand, const int32_t* last,
                                     const int32_t* olen, float* psi, float* r_new, int nhyp, int ncand, int T, int V,
                                     int blank, int eos, void* stream) {
  if (!logp || !r_prev || !cand || !last || !olen || !psi || !r_new || nhyp <= 0 || ncand <= 0 || T <= 0 || V <= 0)
    return EAMD_EINVAL;
  // one utterance of T frames whose hypotheses are all its own: no lengths array (nullptr = every utterance fills the buffer)
  hipLaunchKernelGGL(ctc_prefix_batch_kernel, dim3((ncand + 63) / 64, nhyp), dim3(64), 0, (hipStream_t)stream, logp,
                     (const int*)nullptr, nhyp, r_prev, cand, last, olen, psi, r_new, T, V, ncand, blank, eos);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}
