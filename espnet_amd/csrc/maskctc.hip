// Mask-CTC decoding (reference: espnet/nets/pytorch_backend/e2e_asr_maskctc.py:180-249, E2E.recognize), batched.
//
// eamd_maskctc_seed: greedy CTC of every utterance and the masked decoder input.
//   phase 1 (one workgroup per frame row b,t < hlens[b]): log-softmax of the CTC logits in fp32, p = expf(logp), first-index
//     argmax over p (torch max on the exponentiated row).  The row is swept twice (online max / sum, then p); the second sweep
//     reads what the first just brought into the caches.  Only the frame's id and p are written.
//   phase 2 (one workgroup per utterance): run starts, the segmented max of p per run, compaction of the non-blank runs;
//     a token whose p >= thr (fp32 value compared in double) keeps its id, the others become mask_token.
// eamd_maskctc_update: one mask-predict pass over the decoder logits of the batch.
//   phase 1 (one workgroup per masked row of an active utterance): max logit and first-index argmax over all V classes.
//   phase 2 (one workgroup per utterance): pass < niter-1: the kper masked positions with the largest scores get their argmax
//     (equal scores: the lower position first); pass == niter-1: every masked position gets its argmax; later passes: frozen.
#include "common.h"
#include "select.h"
#include "../../include/espnet_amd.h"

#include <float.h>

namespace {

constexpr int kRowThreads = 256;
constexpr int kSeqThreads = 1024;
constexpr int kSeqPer = EAMD_MASKCTC_MAX_FRAMES / kSeqThreads;   // frames (or positions) per thread in phase 2

// the six-step butterfly, not common.h's wave_sum: another order of the additions changes the last bits of p, and p is compared
// with a threshold
__device__ __forceinline__ float butterfly_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- seed, phase 1 ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRowThreads) void maskctc_frame_kernel(const float* __restrict__ logits,
                                                                    const int32_t* __restrict__ hlens, int32_t* __restrict__ fid,
                                                                    float* __restrict__ fp, int T, int V) {
  const int t = blockIdx.x, b = blockIdx.y;
  if (t >= min(hlens[b], T)) return;
  const float* x = logits + ((long)b * T + t) * V;
  __shared__ float sv[kRowThreads / 64], ss[kRowThreads / 64];
  __shared__ int si[kRowThreads / 64];
  // online max and sum of exp(x - max)
  float m = -FLT_MAX, s = 0.f;
  for (int v = threadIdx.x; v < V; v += kRowThreads) {
    const float xv = x[v];
    if (xv > m) { s = s * expf(m - xv) + 1.f; m = xv; } else { s += expf(xv - m); }
  }
  const float mw = wave_max(m);
  s = butterfly_sum(s * expf(m - mw));
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sv[w] = mw; ss[w] = s; }
  __syncthreads();
  float mb = sv[0];
  for (int k = 1; k < kRowThreads / 64; ++k) mb = fmaxf(mb, sv[k]);
  float sb = 0.f;
  for (int k = 0; k < kRowThreads / 64; ++k) sb += ss[k] * expf(sv[k] - mb);
  __syncthreads();
  const float lse = logf(sb);
  // p = exp(log-softmax) and its first-index argmax
  float pb = -1.f;
  int ib = 0x7fffffff;
  for (int v = threadIdx.x; v < V; v += kRowThreads) first_max(pb, ib, expf((x[v] - mb) - lse), v);
  block_first_max(pb, ib, sv, si, kRowThreads / 64);
  if (threadIdx.x == 0) {
    fid[(long)b * T + t] = ib;
    fp[(long)b * T + t] = pb;
  }
}

// ---- seed, phase 2 ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSeqThreads) void maskctc_collapse_kernel(
    const int32_t* __restrict__ fid, const float* __restrict__ fp, const int32_t* __restrict__ hlens, int64_t* __restrict__ y_in,
    float* __restrict__ tok_p, int32_t* __restrict__ len, int32_t* __restrict__ nmask, int32_t* __restrict__ niter,
    int32_t* __restrict__ kper, int T, int Lcap, int blank, int mask_token, int eos, double thr, int K) {
  const int b = blockIdx.x;
  const int Tb = max(0, min(hlens[b], T));
  const int32_t* id = fid + (long)b * T;
  const float* p = fp + (long)b * T;
  __shared__ unsigned sp[EAMD_MASKCTC_MAX_FRAMES];   // max p of each token's run (p >= 0: its bits order as the value)
  __shared__ int sid[EAMD_MASKCTC_MAX_FRAMES];
  __shared__ int sw[kSeqThreads / 64];
  const int t0 = threadIdx.x * kSeqPer;
  int c = 0;
  for (int j = 0; j < kSeqPer; ++j) {
    const int t = t0 + j;
    if (t < Tb && id[t] != blank && (t == 0 || id[t] != id[t - 1])) ++c;
  }
  int n;
  int k = block_excl_sum<kSeqThreads>(c, sw, &n) - 1;     // token index of the run the thread's first frame belongs to
  for (int i = threadIdx.x; i < n; i += kSeqThreads) sp[i] = 0u;
  __syncthreads();
  for (int j = 0; j < kSeqPer; ++j) {
    const int t = t0 + j;
    if (t >= Tb) break;
    const int v = id[t];
    if (v == blank) continue;
    if (t == 0 || v != id[t - 1]) {
      ++k;
      sid[k] = v;
    }
    atomicMax(&sp[k], __float_as_uint(p[t]));
  }
  __syncthreads();
  int m = 0;
  for (int i = threadIdx.x; i < Lcap; i += kSeqThreads) {
    long o = (long)b * Lcap + i;
    if (i < n) {
      const float pi = __uint_as_float(sp[i]);
      const bool keep = (double)pi >= thr;
      y_in[o] = keep ? sid[i] : mask_token;
      tok_p[o] = pi;
      m += keep ? 0 : 1;
    } else {
      y_in[o] = eos;
      tok_p[o] = 0.f;
    }
  }
  int M;
  block_excl_sum<kSeqThreads>(m, sw, &M);
  if (threadIdx.x == 0) {
    const int it = (M >= K && K > 0) ? K : M;
    len[b] = min(n, Lcap);
    nmask[b] = M;
    niter[b] = it;
    kper[b] = it > 0 ? M / it : 0;
  }
}

// ---- update, phase 1 -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRowThreads) void maskctc_row_argmax_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ y_in, const int32_t* __restrict__ len,
    const int32_t* __restrict__ niter, float* __restrict__ score, int32_t* __restrict__ arg, int pass, int L, int ldy, int V,
    int mask_token) {
  const int l = blockIdx.x, b = blockIdx.y;
  if (l >= min(len[b], L) || pass >= niter[b] || y_in[(long)b * ldy + l] != mask_token) return;
  const float* x = logits + ((long)b * L + l) * V;
  __shared__ float sv[kRowThreads / 64];
  __shared__ int si[kRowThreads / 64];
  float vb = -INFINITY;
  int ib = 0x7fffffff;
  for (int v = threadIdx.x; v < V; v += kRowThreads) first_max(vb, ib, x[v], v);
  block_first_max(vb, ib, sv, si, kRowThreads / 64);
  if (threadIdx.x == 0) {
    score[(long)b * L + l] = vb;
    arg[(long)b * L + l] = ib < V ? ib : 0;      // (a row of NaN: no value compares greater; class 0)
  }
}

// ---- update, phase 2 -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSeqThreads) void maskctc_select_kernel(
    int64_t* __restrict__ y_in, const int32_t* __restrict__ len, const int32_t* __restrict__ niter,
    const int32_t* __restrict__ kper, const float* __restrict__ score, const int32_t* __restrict__ arg, int pass, int L, int ldy,
    int mask_token) {
  const int b = blockIdx.x;
  const int it = niter[b];
  if (pass >= it) return;                              // frozen (block-uniform)
  const int n = min(len[b], L);
  int64_t* y = y_in + (long)b * ldy;
  const float* s = score + (long)b * L;
  const int32_t* a = arg + (long)b * L;
  if (pass == it - 1) {                                // last pass: every masked position
    for (int i = threadIdx.x; i < n; i += kSeqThreads)
      if (y[i] == mask_token) y[i] = a[i];
    return;
  }
  __shared__ float ss[EAMD_MASKCTC_MAX_FRAMES];
  __shared__ unsigned char sm[EAMD_MASKCTC_MAX_FRAMES];
  for (int i = threadIdx.x; i < n; i += kSeqThreads) {
    const bool mk = y[i] == mask_token;
    sm[i] = mk;
    ss[i] = mk ? s[i] : 0.f;
  }
  __syncthreads();
  const int k = kper[b];
  // a masked position is chosen when fewer than k masked positions rank before it (larger score, or equal score and lower
  // position)
  for (int i = threadIdx.x; i < n; i += kSeqThreads) {
    if (!sm[i]) continue;
    const float si = ss[i];
    int r = 0;
    for (int j = 0; j < n && r < k; ++j) r += (sm[j] && ranks_before(ss[j], j, si, i)) ? 1 : 0;
    if (r < k) y[i] = a[i];
  }
}

}  // namespace

int eamd_maskctc_seed(const float* logits, const int32_t* hlens, int32_t* frame_id, float* frame_p, int64_t* y_in, float* tok_p,
                      int32_t* len, int32_t* nmask, int32_t* niter, int32_t* kper, int B, int T, int V, int Lcap, int blank,
                      int mask_token, int eos, double thr, int K, void* stream) {
  if (!logits || !hlens || !frame_id || !frame_p || !y_in || !tok_p || !len || !nmask || !niter || !kper) return EAMD_EINVAL;
  if (B <= 0 || T <= 0 || V <= 0 || Lcap <= 0 || K < 0) return EAMD_EINVAL;
  if (T > EAMD_MASKCTC_MAX_FRAMES || Lcap > T || B > 65535) return EAMD_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(maskctc_frame_kernel, dim3(T, B), dim3(kRowThreads), 0, s, logits, hlens, frame_id, frame_p, T, V);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(maskctc_collapse_kernel, dim3(B), dim3(kSeqThreads), 0, s, frame_id, frame_p, hlens, y_in, tok_p, len, nmask,
                     niter, kper, T, Lcap, blank, mask_token, eos, thr, K);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_maskctc_update(int pass, const float* logits, int64_t* y_in, const int32_t* len, const int32_t* niter,
                        const int32_t* kper, float* score, int32_t* arg, int B, int L, int ldy, int V, int mask_token, void* stream) {
  if (!logits || !y_in || !len || !niter || !kper || !score || !arg) return EAMD_EINVAL;
  if (pass < 0 || B <= 0 || L <= 0 || V <= 0 || ldy < L) return EAMD_EINVAL;
  if (L > EAMD_MASKCTC_MAX_FRAMES || B > 65535) return EAMD_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(maskctc_row_argmax_kernel, dim3(L, B), dim3(kRowThreads), 0, s, logits, y_in, len, niter, score, arg, pass, L,
                     ldy, V, mask_token);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(maskctc_select_kernel, dim3(B), dim3(kSeqThreads), 0, s, y_in, len, niter, kper, score, arg, pass, L, ldy,
                     mask_token);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}
