// Second-pass n-best rescoring (include/espnet_amd.h, "Second-pass n-best rescoring"): the device glue between the
// packed n-best of eamd_ctc_prefix_beam, a teacher-forced decoder / LM forward and eamd_gemm's row-statistics
// epilogue.  Plain vector stores, no atomics, fixed reduction orders: two launches give the same bits.
#include "common.h"
#include "../../include/espnet_amd.h"

#define RESCORE_MAX_N 32
#define RESCORE_MAX_T 2048
#define RESCORE_MAX_WAVES 16

// one thread per (row, position): a pure index kernel.  L is read from the device and clamped to what the buffers hold.
__global__ __launch_bounds__(256) void nbest_pack_kernel(const int* __restrict__ nbest, long* __restrict__ ys_in,
                                                         int* __restrict__ col, int* __restrict__ ulen, long rows, int T, int U,
                                                         int V, int sos, int eos) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * U) return;
  const long r = e / U;
  const int u = (int)(e - r * U);
  const int* row = nbest + r * (2 + T);
  const int Lraw = row[1];
  const int L = min(min(Lraw, U - 1), T);
  // position u reads tok_{u-1} and predicts tok_u
  int prev = sos, next = -1;
  if (Lraw >= 0) {
    if (u >= 1) prev = (u - 1 < L) ? min(max(row[2 + u - 1], 0), V - 1) : eos;
    next = (u < L) ? min(max(row[2 + u], 0), V - 1) : (u == L ? eos : -1);
  } else if (u >= 1) {
    prev = eos;
  }
  ys_in[e] = prev;
  col[e] = next;
  if (u == 0) ulen[r] = Lraw >= 0 ? L + 1 : 0;
}

// log-sum-exp of one row from its tile partials (max, sum exp), tiles in order: the merge of rnnt_stats_combine_kernel
__device__ __forceinline__ float rescore_row_lse(const float2* __restrict__ pp, int tiles_n) {
  float m = -INFINITY;
  for (int j = 0; j < tiles_n; ++j) m = fmaxf(m, pp[j].x);
  float sm = 0.f;
  for (int j = 0; j < tiles_n; ++j) sm += (pp[j].x > -INFINITY) ? pp[j].y * expf(pp[j].x - m) : 0.f;
  return m + logf(sm);
}

// sum_i (zcol - lse) over the npos positions of one hypothesis: lane l adds positions l, l + 64, ... in that order, then
// the fixed butterfly of wave_sum
__device__ __forceinline__ float rescore_term(const float* __restrict__ part, const float* __restrict__ zcol, int tiles_n,
                                              long row0, int npos, int lane) {
  float acc = 0.f;
  for (int i = lane; i < npos; i += 64) {
    const long row = row0 + i;
    acc += zcol[row] - rescore_row_lse(reinterpret_cast<const float2*>(part) + row * tiles_n, tiles_n);
  }
  return wave_sum(acc);
}

// one workgroup per utterance, one wave per hypothesis (waves stride over n), lanes over positions
__global__ __launch_bounds__(64 * RESCORE_MAX_WAVES) void nbest_rescore_kernel(
    const int* __restrict__ nbest, const int* __restrict__ ulen, int N, int T, int U, int S, const float* __restrict__ part1,
    const float* __restrict__ zcol1, int tiles1, float w1, const float* __restrict__ part2, const float* __restrict__ zcol2,
    int tiles2, float w2, float w0, int* __restrict__ nbest_out, float* __restrict__ terms, int* __restrict__ order) {
  __shared__ float s_f[RESCORE_MAX_N], s_key[RESCORE_MAX_N], s_s1[RESCORE_MAX_N], s_t1[RESCORE_MAX_N], s_t2[RESCORE_MAX_N];
  __shared__ int s_here[RESCORE_MAX_N], s_order[RESCORE_MAX_N];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  const long W = 2 + T;
  const int* in = nbest + (long)b * N * W;
  for (int n = wave; n < N; n += nwave) {
    const long r = (long)b * N + n;
    const bool here = in[n * W + 1] >= 0;
    const int npos = here ? min(max(ulen[r], 0), U) : 0;
    const float s1 = __int_as_float(in[n * W]);
    const float t1 = rescore_term(part1, zcol1, tiles1, r * U, npos, lane);
    const float t2 = S == 2 ? rescore_term(part2, zcol2, tiles2, r * U, npos, lane) : 0.f;
    // f = w0 * s1 + w1 * term1 (+ w2 * term2): rounded products, added left to right, nothing contracted
    float f = __fadd_rn(__fmul_rn(w0, s1), __fmul_rn(w1, t1));
    if (S == 2) f = __fadd_rn(f, __fmul_rn(w2, t2));
    if (lane == 0) {
      s_here[n] = here;
      s_s1[n] = s1; s_t1[n] = t1; s_t2[n] = t2; s_f[n] = f;
      s_key[n] = f != f ? -INFINITY : f;          // a NaN (0 * -inf) ranks with -inf
    }
  }
  __syncthreads();
  // rank: f descending, equal f to the lower first-pass index, absent hypotheses last (in their first-pass order)
  if (threadIdx.x < N) {
    const int n = threadIdx.x;
    int rank = 0;
    for (int m = 0; m < N; ++m) {
      if (s_here[n]) rank += s_here[m] && (s_key[m] > s_key[n] || (s_key[m] == s_key[n] && m < n));
      else rank += s_here[m] || m < n;
    }
    s_order[rank] = n;
  }
  __syncthreads();
  int* out = nbest_out + (long)b * N * W;
  for (long e = threadIdx.x; e < N * W; e += blockDim.x) {
    const int k = (int)(e / W), wd = (int)(e - k * W), n = s_order[k];
    int v = in[n * W + wd];
    if (wd == 0 && s_here[n]) v = __float_as_int(s_f[n]);
    out[e] = v;
  }
  if (threadIdx.x < N) {
    const int k = threadIdx.x, n = s_order[k];
    float* tr = terms + ((long)b * N + k) * (1 + S);
    tr[0] = s_s1[n];
    tr[1] = s_t1[n];
    if (S == 2) tr[2] = s_t2[n];
    order[(long)b * N + k] = n;
  }
}

extern "C" int eamd_nbest_pack(const int32_t* nbest, int B, int N, int T, int U, int V, int sos, int eos, int64_t* ys_in,
                               int32_t* col, int32_t* ulen, void* stream) {
  if (!nbest || !ys_in || !col || !ulen || B <= 0 || N <= 0 || T <= 0 || U <= 0 || V <= 0) return EAMD_EINVAL;
  if (U > T + 1 || sos < 0 || sos >= V || eos < 0 || eos >= V) return EAMD_EINVAL;
  if (N > RESCORE_MAX_N || T > RESCORE_MAX_T) return EAMD_EUNSUPPORTED;
  const long n = (long)B * N * U;
  hipLaunchKernelGGL(nbest_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nbest,
                     reinterpret_cast<long*>(ys_in), col, ulen, (long)B * N, T, U, V, sos, eos);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

extern "C" int eamd_nbest_rescore(const int32_t* nbest, const int32_t* ulen, int B, int N, int T, int U, int S, const float* part1,
                                  const float* zcol1, int tiles1, float w1, const float* part2, const float* zcol2, int tiles2,
                                  float w2, float w0, int32_t* nbest_out, float* terms, int32_t* order, void* stream) {
  if (!nbest || !ulen || !nbest_out || !terms || !order || nbest == nbest_out || B <= 0 || N <= 0 || T <= 0 || U <= 0)
    return EAMD_EINVAL;
  if (S != 1 && S != 2) return EAMD_EUNSUPPORTED;
  if (!part1 || !zcol1 || tiles1 <= 0 || (S == 2 && (!part2 || !zcol2 || tiles2 <= 0))) return EAMD_EINVAL;
  if (U > T + 1) return EAMD_EINVAL;
  if (N > RESCORE_MAX_N || T > RESCORE_MAX_T) return EAMD_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(part1) & 7) || (S == 2 && (reinterpret_cast<uintptr_t>(part2) & 7))) return EAMD_EUNSUPPORTED;
  const int nwave = N < RESCORE_MAX_WAVES ? N : RESCORE_MAX_WAVES;
  hipLaunchKernelGGL(nbest_rescore_kernel, dim3(B), dim3(64 * nwave), 0, (hipStream_t)stream, nbest, ulen, N, T, U, S, part1, zcol1,
                     tiles1, w1, part2, zcol2, tiles2, w2, w0, nbest_out, terms, order);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}
