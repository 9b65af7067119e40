// The ONE ordering of every selection in the library - first-index argmax, top-k, rank by counting - and the block scan the
// compaction kernels share: the larger value ranks first and, of equal values, the lower index.  The bit-exact comparisons
// (greedy CTC against the oracle, the n-best lists of the beam searches, transducer_expand_rows against log_softmax_rows +
// topk_rows) rely on every kernel agreeing on it, so it is written here and nowhere else.
// Everything is __device__ __forceinline__ and nothing allocates LDS: callers pass their arrays, as block_sum's do.
#pragma once
#include "common.h"

// ---- keys: "ranks before" as ONE unsigned compare ----------------------------------------------------------------------------
// Order-preserving bits of a float: a < b <=> order_bits(a) < order_bits(b).  NaN counts as -inf and -0 as +0; no float maps
// to 0, which callers use for "no element".
__device__ __forceinline__ unsigned order_bits(float v) {
  v = (v != v) ? -INFINITY : v;
  if (v == 0.f) v = 0.f;
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float order_value(unsigned b) { return __uint_as_float((b & 0x80000000u) ? (b ^ 0x80000000u) : ~b); }
// (bits, ~index): the larger key is the larger value or, of equal values, the lower index
__device__ __forceinline__ unsigned long long order_key(unsigned bits, unsigned i) { return ((unsigned long long)bits << 32) | (0xFFFFFFFFu - i); }
__device__ __forceinline__ unsigned key_index(unsigned long long key) { return 0xFFFFFFFFu - (unsigned)key; }

// ---- first maximum on (value, index) pairs -----------------------------------------------------------------------------------
// On pairs with distinct indices and no NaN value ranks_before is a strict total order, so a reduction gives the same pair in
// any order of its steps.  A NaN compares false both ways: it neither replaces a pair nor is replaced, so with one in play the
// lanes of a butterfly end up disagreeing and the order of the steps decides what the reading lane holds.  Every site but one
// starts from -inf (or -1) and takes an element only through this compare, and so never holds a NaN (beam_select_kernel maps it to
// -inf first); rnnt_greedy_joint_kernel starts each lane from its own, possibly NaN, logit - which is why the wave step walks the
// offsets in that kernel's order, ascending (1, 2, 4, ...), and must keep doing so.
template <typename I>
__device__ __forceinline__ bool ranks_before(float va, I ia, float vb, I ib) { return va > vb || (va == vb && ia < ib); }
template <typename I>
__device__ __forceinline__ void first_max(float& v, I& i, float v2, I i2) {
  if (ranks_before(v2, i2, v, i)) { v = v2; i = i2; }
}
// over the aligned groups of WIDTH (16 or 64) lanes; the result in every lane of the group
template <int WIDTH, typename I>
__device__ __forceinline__ void wave_first_max(float& v, I& i) {
  static_assert(WIDTH == 16 || WIDTH == 64, "a 16-lane row or the wave");
#pragma unroll
  for (int off = 1; off < WIDTH; off <<= 1) {
    const float v2 = __shfl_xor(v, off, 64);
    const I i2 = __shfl_xor(i, off, 64);
    first_max(v, i, v2, i2);
  }
}
// over the nw waves of the workgroup; the result in every thread.  sv / si: nw entries of LDS.  Two barriers: every thread must
// call it, and sv / si may be reused right after.
template <typename I>
__device__ __forceinline__ void block_first_max(float& v, I& i, float* sv, I* si, int nw) {
  wave_first_max<64>(v, i);
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = sv[0]; i = si[0];
  for (int k = 1; k < nw; ++k) first_max(v, i, sv[k], si[k]);
  __syncthreads();
}

// ---- the k first of a row, by one workgroup of 256 threads ---------------------------------------------------------------------
// Rows of up to TOPK_RMAX * 256 elements are register-resident as order bits: reg[q] = bits_at(q) = those of element t + 256 q,
// 0 = no element (past the end, or excluded by the caller).  The caller's loading is that callable, evaluated inside the one
// branch on the row length: a separate branch in the kernel cost topk_rows_kernel 24 moves and a jump per wave, 0.6 % of its
// 9.3 us.  The row is cut down first: every element of the answer is >= the k-th largest of the 256 per-thread maxima (those k
// maxima alone are k elements that large), so the elements at or above that threshold - a few dozen in general - are gathered
// in LDS and ranked by counting.  Longer rows, and rows with more than TOPK_CAP elements at the threshold, take k rounds of
// "largest key below the previous winner"; a long row is re-read through key_at(i), i = first .. n - 1.  emit(rank, key) is
// called once per rank 0 .. k - 1, by whichever thread finds it.
constexpr int TOPK_CAP = 1024;
constexpr int TOPK_RMAX = 24;
struct TopkLds {
  unsigned* tmax;               // [256], 16-byte aligned
  unsigned long long* cand;     // [TOPK_CAP]
  unsigned long long* sk;       // [4]
  unsigned long long* wk;
  unsigned* tau;
  int* cnt;
};
template <typename BitsAt, typename KeyAt, typename Emit>
__device__ __forceinline__ void block_topk(int first, int n, int k, const TopkLds s, BitsAt bits_at, KeyAt key_at, Emit emit) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned reg[TOPK_RMAX];
  const bool inreg = n <= TOPK_RMAX * 256;
  if (inreg) {
    unsigned tm = 0;
#pragma unroll
    for (int q = 0; q < TOPK_RMAX; ++q) {
      reg[q] = bits_at(q);
      tm = max(tm, reg[q]);
    }
    s.tmax[t] = tm;
    if (t == 0) { *s.tau = 0xFFFFFFFFu; *s.cnt = 0; }
    __syncthreads();
    int above = 0;                               // thread maxima strictly above mine
#pragma unroll 8
    for (int j = 0; j < 256; j += 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(&s.tmax[j]);
      above += (v.x > tm) + (v.y > tm) + (v.z > tm) + (v.w > tm);
    }
    if (above < k && tm != 0u) atomicMin(s.tau, tm);
    __syncthreads();
    const unsigned th = *s.tau;
#pragma unroll
    for (int q = 0; q < TOPK_RMAX; ++q) {
      if (reg[q] >= th && reg[q] != 0u) {
        const int p = atomicAdd(s.cnt, 1);
        if (p < TOPK_CAP) s.cand[p] = order_key(reg[q], (unsigned)(t + 256 * q));
      }
    }
    __syncthreads();
    const int c = *s.cnt;
    if (c <= TOPK_CAP) {
      for (int j = t; j < c; j += 256) {
        const unsigned long long my = s.cand[j];
        int r = 0;
        for (int q = 0; q < c; ++q) r += s.cand[q] > my;
        if (r < k) emit(r, my);
      }
      return;
    }
    __syncthreads();
  }
  unsigned long long prev = 0xFFFFFFFFFFFFFFFFull;      // previous winner: every element ranks after it
  for (int r = 0; r < k; ++r) {
    unsigned long long best = 0;
    if (inreg) {
#pragma unroll
      for (int q = 0; q < TOPK_RMAX; ++q) {
        const unsigned long long key = order_key(reg[q], (unsigned)(t + 256 * q));
        if (reg[q] != 0u && key < prev && key > best) best = key;
      }
    } else {
      for (long i = first + t; i < n; i += 256) {
        const unsigned long long key = key_at(i);
        if (key < prev && key > best) best = key;
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const unsigned long long o = __shfl_xor(best, m);
      best = o > best ? o : best;
    }
    if (lane == 0) s.sk[w] = best;
    __syncthreads();
    if (t == 0) {
      unsigned long long f = s.sk[0];
#pragma unroll
      for (int q = 1; q < 4; ++q) f = s.sk[q] > f ? s.sk[q] : f;
      *s.wk = f;
      emit(r, f);
    }
    __syncthreads();
    prev = *s.wk;
  }
}

// ---- block exclusive prefix sum ----------------------------------------------------------------------------------------------
// of v over the THREADS threads of the workgroup; *total = the sum.  s_w: THREADS / 64 ints of LDS.  Two barriers: every thread
// must call it, and s_w may be reused right after.
template <int THREADS>
__device__ __forceinline__ int block_excl_sum(int v, int* s_w, int* total) {
  const int lane = threadIdx.x & (EAMD_WAVE - 1), w = threadIdx.x / EAMD_WAVE;
  int inc = v;
#pragma unroll
  for (int d = 1; d < EAMD_WAVE; d <<= 1) {
    const int o = __shfl_up(inc, d, EAMD_WAVE);
    if (lane >= d) inc += o;
  }
  if (lane == EAMD_WAVE - 1) s_w[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < THREADS / EAMD_WAVE; ++k) {
    const int s = s_w[k];
    if (k < w) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}
