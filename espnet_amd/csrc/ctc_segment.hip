// CTC segmentation of long recordings (Kuerzinger et al. 2020): where each utterance of a transcript starts and ends in a whole
// recording, and how much to trust it.  The reference leaves this to the external ctc_segmentation package (called from
// espnet/bin/asr_align.py); here it runs on the device over a batch of recordings.  Per window attempt, on the caller's stream:
//   emissions : the U distinct tokens of each transcript (row 0: blank) gathered out of lpz [T,V] into rows em [U,T], so that every
//               later read runs along t                                                  (eamd_ctc_segment_emissions, once per call)
//   fill      : one workgroup per recording, the characters (columns) in order; within a column the window's W rows satisfy
//               x_t = max(sw_t, x_{t-1} + b_t), a max-plus linear recurrence, done as a block scan: kRpt rows per thread in
//               registers, a wave scan of the threads' (a, b) pairs, the waves' totals through LDS.  Only the last S + 1 columns
//               of values are kept (a ring, in LDS when it fits, else in global memory); per cell one backpointer byte is stored
//   backtrack : one wave per recording; a run of "stay" cells is skipped 64 rows at a time (ballot over 64 backpointer bytes)
//   prefix    : float64 prefix sums of char_probs per recording
//   segments  : one wave per utterance: start, end and the minimum of the sliding means of char_probs
// Unreachable cells are -inf.  Every loop is bounded by T, L, W or S; workgroups never wait for each other.
#include <limits.h>
#include "common.h"
#include "select.h"
#include "../../include/espnet_amd.h"

namespace {
constexpr int kRpt = 8;                 // window rows per thread and tile
constexpr int kMaxS = 16;               // longest token, in characters
constexpr int kMaxThreads = 1024;
constexpr int kScratch = 128;           // floats of LDS in front of the ring: wave totals (2 x 2 x 16), column maxima (2 x 16)
constexpr int kLdsBytes = 160 * 1024;
enum { kOk = 0, kNoPath = 1, kBadArg = 2, kBadWalk = 3 };

// ring / LDS row index: one pad word per 32 rows, so the 8-row stride of neighbouring lanes spreads over the banks
__device__ __host__ __forceinline__ int pad_row(int r) { return r + (r >> 5); }
__device__ __host__ __forceinline__ int64_t ring_stride(int W) { return (int64_t)pad_row(W) + 1; }

__global__ __launch_bounds__(256) void seg_emissions_kernel(const float* __restrict__ lpz, const int* __restrict__ lens,
                                                            const int* __restrict__ tok, float* __restrict__ em, int Tmax, int V,
                                                            int Umax, int blank, int gratis) {
  const int t = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y, b = blockIdx.z;
  if (t >= min(lens[b], Tmax)) return;
  const int g = u == 0 ? blank : tok[(int64_t)b * Umax + u];
  if (g < 0) return;                                                  // an unused row
  float v = -INFINITY;
  if (u == 0 && gratis) v = 0.f;
  else if (g < V) v = lpz[((int64_t)b * Tmax + t) * V + g];
  em[((int64_t)b * Umax + u) * Tmax + t] = v;
}

// a thread's kRpt consecutive emissions row[t0 ..]: two 16-byte loads at 4-byte alignment (the window offset is arbitrary) where
// all of them lie in the window - eight 4-byte loads would each touch the 2 KB a wave's rows span; else row by row, rows behind
// the window reading row W - 1
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void load_rows(const float* __restrict__ row, int t0, int W, float (&e)[kRpt]) {
  static_assert(kRpt == 8, "two float4 per thread");
  if (t0 + kRpt <= W) {
    const f32x4u a = *reinterpret_cast<const f32x4u*>(row + t0), b = *reinterpret_cast<const f32x4u*>(row + t0 + 4);
    e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w;
    e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < kRpt; ++j) e[j] = row[min(t0 + j, W - 1)];
  }
}

template <bool kLds>
__global__ __launch_bounds__(kMaxThreads) void seg_fill_kernel(
    const float* __restrict__ em, const int* __restrict__ gtu, const int* __restrict__ lens, const int* __restrict__ llens,
    const int* __restrict__ sel, unsigned char* __restrict__ bp, float* __restrict__ gring, int* __restrict__ info,
    int* __restrict__ offsets, int* __restrict__ timings, float* __restrict__ cprobs, int* __restrict__ states, int Tmax, int Lmax,
    int S, int Umax, int window, int Wmax) {
  extern __shared__ float smem[];
  float* comp_a = smem;                    // [2][16] wave totals of the scan, by parity of the scan
  float* comp_b = smem + 32;               // [2][16]
  float* am_v = smem + 64;                 // [16] column maximum of each wave
  int* am_r = reinterpret_cast<int*>(smem + 80);
  const int blk = blockIdx.x, b = sel[blk], tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
  const int T = min(lens[b], Tmax), L = llens[b];
  int* inf = info + (int64_t)b * 4;
  int* off_b = offsets + (int64_t)b * Lmax;
  for (int t = tid; t < Tmax; t += nt) { cprobs[(int64_t)b * Tmax + t] = 0.f; states[(int64_t)b * Tmax + t] = -2; }
  for (int i = tid; i < Lmax; i += nt) { timings[(int64_t)b * Lmax + i] = 0; off_b[i] = 0; }
  if (T < 1 || L < 1 || L > T || L > Lmax) {
    if (tid == 0) { inf[0] = kBadArg; inf[1] = 0; inf[2] = 0; inf[3] = 0; }
    return;
  }
  const int W = min(window, T);
  const int64_t rs = ring_stride(Wmax);
  float* ring = kLds ? smem + kScratch : gring + (int64_t)blk * (S + 1) * rs;
  unsigned char* bp_b = bp + (int64_t)blk * Wmax * Lmax;
  const float* em_b = em + (int64_t)b * Umax * Tmax;
  const int* gt_b = gtu + (int64_t)b * Lmax * S;
  const int higher = (T - W) / L + 1;
  const int tile = nt * kRpt;
  // the package's window offsets of the S spans, cur[s]: cur[0] = this column's offset, cur[s >= 1] = cur[0] of the column
  // before + s x this column's offset (its loop runs over s ascending, in place); all -1 in front of column 1
  int osum = 0, last_arg = 0, par = 0, off = -1, off_prev = -1, slot = 0;
  float best_v = -INFINITY;
  for (int c = 0; c < L; ++c) {
    if (c > 0) {
      off_prev = off;
      off = min(max(0, last_arg - W / 2), min(higher, (T - W) - osum));
      osum += off;
      slot = slot == S ? 0 : slot + 1;                          // c % (S + 1)
    }
    if (tid == 0) off_b[c] = osum;
    const int first = c == 0 ? 1 : 0;
    const int* g_c = gt_b + (int64_t)c * S;
    const float* eb = em_b + osum;                              // blank row from this column's first frame on
    float* ring_c = ring + (int64_t)slot * rs;
    unsigned char* bp_c = bp_b + (int64_t)c * W;
    float mv = -INFINITY;                                       // this thread's column maximum over the visited rows
    int mr = INT_MAX;
    float xc = -INFINITY;                                       // x of the row in front of the tile
    for (int r0 = 0; r0 < W; r0 += tile) {
      const int t0 = r0 + tid * kRpt;
      float sw[kRpt], mx[kRpt];
      int sb[kRpt];
#pragma unroll
      for (int j = 0; j < kRpt; ++j) { sw[j] = -INFINITY; mx[j] = -INFINITY; sb[j] = 0; }
      float bl[kRpt];
      load_rows(eb, t0, W, bl);                                 // the blank row, in flight beside the tokens' rows
      for (int s = 0; s < S; ++s) {
        const int g = g_c[s];                                   // block-uniform
        if (g < 0) continue;
        const float* er = em_b + (int64_t)g * Tmax + osum;
        const int cs = s == 0 ? off : off_prev + s * off;
        const bool col_ok = c - 1 - s >= 0;
        const int ps = slot - 1 - s;
        const float* prev = ring + (int64_t)(ps < 0 ? ps + S + 1 : ps) * rs;      // column c - 1 - s
        const int wlim = W - (cs - 1);
        // straight-line code, no branch per row: a row behind the window reads row W - 1 and is dropped below, a cell that may
        // not switch reads a clamped row and selects -inf
        float e8[kRpt];
        load_rows(er, t0, W, e8);
#pragma unroll
        for (int j = 0; j < kRpt; ++j) {
          const int t = min(t0 + j, W - 1);
          const float e = e8[j];
          mx[j] = fmaxf(mx[j], e);
          const int r = t - 1 + cs;
          const float pv = prev[pad_row(min(max(r, 0), W - 1))];
          const float p = (col_ok && r >= 0 && t < wlim) ? pv + e : -INFINITY;
          const bool better = p > sw[j];
          sw[j] = better ? p : sw[j];
          sb[j] = better ? s : sb[j];
        }
      }
      float A = -INFINITY, Bs = 0.f;
#pragma unroll
      for (int j = 0; j < kRpt; ++j) {
        const int t = t0 + j;
        const bool in = t < W;
        bl[j] = in ? fmaxf(bl[j], mx[j]) : 0.f;                 // behind the window: the scan's identity (-inf, 0)
        sw[j] = in ? sw[j] : -INFINITY;
        if (c == 0 && t == 0) sw[j] = 0.f;                       // table[0, 0] = 0, the one cell the recursion does not visit
        A = fmaxf(sw[j], A + bl[j]);
        Bs += bl[j];
      }
      // inclusive wave scan of (A, Bs) under (a2, b2) o (a1, b1) = (max(a2, a1 + b2), b1 + b2)
      float Ai = A, Bi = Bs;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const float a1 = __shfl_up(Ai, d, 64), b1 = __shfl_up(Bi, d, 64);
        if (lane >= d) { Ai = fmaxf(Ai, a1 + Bi); Bi = b1 + Bi; }
      }
      float Ae = __shfl_up(Ai, 1, 64), Be = __shfl_up(Bi, 1, 64);
      if (lane == 0) { Ae = -INFINITY; Be = 0.f; }
      if (lane == 63) { comp_a[par * 16 + wv] = Ai; comp_b[par * 16 + wv] = Bi; }
      __syncthreads();
      float x = xc, xw = xc;
      for (int i = 0; i < nw; ++i) {
        x = fmaxf(comp_a[par * 16 + i], x + comp_b[par * 16 + i]);
        if (i == wv - 1) xw = x;
      }
      xc = x;                                                   // x of the tile's last row
      par ^= 1;
      x = fmaxf(Ae, xw + Be);                                   // x of the row in front of this thread's rows
      unsigned long long word = 0;
#pragma unroll
      for (int j = 0; j < kRpt; ++j) {
        const int t = t0 + j;
        const float st = x + bl[j];                             // row 0: x = -inf; behind the window: x + 0 >= -inf, a stay
        const bool stay = st >= sw[j];
        x = stay ? st : sw[j];
        const unsigned code = (stay || (c == 0 && t == 0)) ? 0u : 1u + (unsigned)sb[j];
        word |= (unsigned long long)code << (8 * j);
        if (t < W) ring_c[pad_row(t)] = x;
        const bool top = t < W && t >= first && x > mv;
        mv = top ? x : mv;
        mr = top ? t : mr;
      }
      if (t0 + kRpt <= W && ((reinterpret_cast<uintptr_t>(bp_c + t0) & 7) == 0)) {
        *reinterpret_cast<unsigned long long*>(bp_c + t0) = word;
      } else {
#pragma unroll
        for (int j = 0; j < kRpt; ++j)
          if (t0 + j < W) bp_c[t0 + j] = (unsigned char)(word >> (8 * j));
      }
    }
    // the column's first maximum over the visited rows (select.h: the larger value, of equal values the smaller row)
    wave_first_max<64>(mv, mr);
    if (lane == 0) { am_v[wv] = mv; am_r[wv] = mr; }
    __syncthreads();                                            // also: this column's ring values are written
    float cv = am_v[0];
    int cr = am_r[0];
    for (int i = 1; i < nw; ++i) first_max(cv, cr, am_v[i], am_r[i]);
    last_arg = cr == INT_MAX ? first : cr;
    best_v = cv;
  }
  if (tid == 0) {
    int end_row = last_arg;
    if (L == 1 && !(best_v > 0.f)) { end_row = 0; best_v = 0.f; }       // column 0 also holds table[0, 0] = 0, its first row
    inf[0] = best_v > -INFINITY ? kOk : kNoPath;
    inf[1] = end_row;
    inf[2] = W;
    inf[3] = osum;
  }
}

// the walk back from (end row, L - 1) to (0, 0): lane l looks at the backpointer l rows up the column
__global__ __launch_bounds__(64) void seg_backtrack_kernel(const float* __restrict__ em, const int* __restrict__ gtu,
                                                           const int* __restrict__ tok, const int* __restrict__ lens,
                                                           const int* __restrict__ llens, const int* __restrict__ sel,
                                                           const unsigned char* __restrict__ bp, int* __restrict__ info,
                                                           const int* __restrict__ offsets, int* __restrict__ timings,
                                                           float* __restrict__ cprobs, int* __restrict__ states, int Tmax, int Lmax,
                                                           int S, int Umax, int Wmax) {
  const int blk = blockIdx.x, b = sel[blk], lane = threadIdx.x;
  int* inf = info + (int64_t)b * 4;
  if (inf[0] != kOk) return;
  const int T = min(lens[b], Tmax), L = llens[b], W = inf[2];
  const unsigned char* bp_b = bp + (int64_t)blk * Wmax * Lmax;
  const float* em_b = em + (int64_t)b * Umax * Tmax;
  const int* gt_b = gtu + (int64_t)b * Lmax * S;
  const int* off_b = offsets + (int64_t)b * Lmax;
  const int* tok_b = tok + (int64_t)b * Umax;
  int* tm_b = timings + (int64_t)b * Lmax;
  float* cp_b = cprobs + (int64_t)b * Tmax;
  int* st_b = states + (int64_t)b * Tmax;
  int t = inf[1], c = L - 1;
  bool done = false;
  const int max_it = L + T / 64 + 2;
  for (int it = 0; it < max_it; ++it) {
    if (c == 0) {                                               // column 0: stay cells down to row 1
      for (int r = 1 + lane; r <= t; r += 64) { cp_b[r] = em_b[r]; st_b[r] = -1; }
      done = true;
      break;
    }
    const int oc = off_b[c];
    const int* g_c = gt_b + (int64_t)c * S;
    const int r = t - lane;
    const unsigned code = r >= 0 ? bp_b[(int64_t)c * W + r] : 0u;
    const unsigned long long mask = __ballot(code != 0u);
    const int nstay = mask ? __ffsll((long long)mask) - 1 : 64;
    float mx = -INFINITY;
    if (r >= 0 && lane <= nstay) {
      for (int s = 0; s < S; ++s) {
        const int g = g_c[s];
        if (g >= 0) mx = fmaxf(mx, em_b[(int64_t)g * Tmax + oc + r]);
      }
    }
    if (r >= 0 && lane < nstay) { cp_b[oc + r] = fmaxf(em_b[oc + r], mx); st_b[oc + r] = -1; }
    if (!mask) {
      t -= 64;
      if (t < 0) break;
      continue;
    }
    const int s = (int)__shfl(code, nstay, 64) - 1;
    const int tsw = t - nstay, f = oc + tsw;
    if (lane == nstay) { cp_b[f] = mx; st_b[f] = tok_b[g_c[s]]; }
    if (lane <= s) tm_b[c - lane] = f;
    const int d = oc - (c - s > 0 ? off_b[c - 1 - s] : 0);
    c -= 1 + s;
    t = tsw - 1 + d;
    if (c < 0 || t < 0 || t >= W) break;
  }
  if (!done && lane == 0) inf[0] = kBadWalk;
}

// psum[t] = sum of char_probs[0 .. t) in float64, one workgroup per recording
__global__ __launch_bounds__(kMaxThreads) void seg_prefix_kernel(const float* __restrict__ cprobs, const int* __restrict__ lens,
                                                                 const int* __restrict__ sel, double* __restrict__ psum, int Tmax) {
  __shared__ double part[2][kMaxThreads];
  const int b = sel[blockIdx.x], tid = threadIdx.x;
  const int T = min(lens[b], Tmax);
  const float* cp = cprobs + (int64_t)b * Tmax;
  double* ps = psum + (int64_t)b * (Tmax + 1);
  const int chunk = (T + kMaxThreads - 1) / kMaxThreads;
  const int lo = min(tid * chunk, T), hi = min(lo + chunk, T);
  double sum = 0.0;
  for (int t = lo; t < hi; ++t) sum += (double)cp[t];
  part[0][tid] = sum;
  __syncthreads();
  int p = 0;
  for (int d = 1; d < kMaxThreads; d <<= 1) {
    part[p ^ 1][tid] = tid >= d ? part[p][tid] + part[p][tid - d] : part[p][tid];
    p ^= 1;
    __syncthreads();
  }
  double run = part[p][tid] - sum;                              // exclusive
  if (tid == 0) ps[0] = 0.0;
  for (int t = lo; t < hi; ++t) { run += (double)cp[t]; ps[t + 1] = run; }
}

// one wave per utterance: start and end in seconds, confidence = min(0, least mean of n_mean consecutive char_probs)
__global__ __launch_bounds__(256) void seg_segments_kernel(const int* __restrict__ timings, const double* __restrict__ psum,
                                                           const int* __restrict__ lens, const int* __restrict__ llens,
                                                           const int* __restrict__ sel, const int* __restrict__ utt,
                                                           const int* __restrict__ nutt, const int* __restrict__ info,
                                                           double* __restrict__ seg, int Tmax, int Lmax, int NU, int n_mean,
                                                           double idur) {
#pragma clang fp contract(off)
  const int b = sel[blockIdx.y], lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= NU) return;
  double* out = seg + ((int64_t)b * NU + i) * 3;
  if (i >= nutt[b] || info[(int64_t)b * 4] != kOk) {
    if (lane < 3) out[lane] = 0.0;
    return;
  }
  const int T = min(lens[b], Tmax), L = llens[b];
  const int* tm_b = timings + (int64_t)b * Lmax;
  const double* ps = psum + (int64_t)b * (Tmax + 1);
  const int ub = utt[(int64_t)b * (NU + 1) + i], ue = utt[(int64_t)b * (NU + 1) + i + 1];
  auto tm = [&](int k) { return __dmul_rn((double)tm_b[min(max(k, 0), L - 1)], idur); };
  const double start = fmax(tm(ub + 1) - 0.5, (tm(ub) + tm(ub - 1)) / 2.0);
  const double end = fmin(tm(ue - 1) + 0.5, (tm(ue) + tm(ue - 1)) / 2.0);
  const long a = min(max((long)rint(start / idur), 0L), (long)T), z = min(max((long)rint(end / idur), 0L), (long)T);
  double conf;
  if (z <= a) {
    conf = -INFINITY;
  } else if (z - a <= n_mean) {
    conf = (ps[z] - ps[a]) / (double)(z - a);
  } else {
    double m = INFINITY;
    for (long t = a + lane; t < z - n_mean; t += 64) m = fmin(m, (ps[t + n_mean] - ps[t]) / (double)n_mean);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) m = fmin(m, __shfl_xor(m, d, 64));
    conf = fmin(0.0, m);
  }
  if (lane == 0) { out[0] = start; out[1] = end; out[2] = conf; }
}

int fill_threads(int Wmax) {
  const int need = (Wmax + kRpt - 1) / kRpt;
  const int nt = (need + 63) / 64 * 64;
  return nt < 64 ? 64 : (nt > kMaxThreads ? kMaxThreads : nt);
}
int64_t ring_lds_bytes(int S, int Wmax) { return ((int64_t)kScratch + (int64_t)(S + 1) * ring_stride(Wmax)) * 4; }
}  // namespace

extern "C" {

int eamd_ctc_segment_ring_in_lds(int S, int W) {
  if (S < 1 || S > kMaxS || W < 1) return EAMD_EINVAL;
  return ring_lds_bytes(S, W) <= kLdsBytes ? 1 : 0;
}

int eamd_ctc_segment_emissions(const float* lpz, const int32_t* lens, const int32_t* tok, float* em, int B, int Tmax, int V,
                               int Umax, int blank, int gratis_blank, void* stream) {
  if (!lpz || !lens || !tok || !em || B < 1 || Tmax < 1 || V < 1 || Umax < 1 || blank < 0 || blank >= V) return EAMD_EINVAL;
  if (Umax > 65535 || B > 65535) return EAMD_EUNSUPPORTED;
  hipLaunchKernelGGL(seg_emissions_kernel, dim3((Tmax + 255) / 256, Umax, B), dim3(256), 0, (hipStream_t)stream, lpz, lens, tok, em,
                     Tmax, V, Umax, blank, gratis_blank ? 1 : 0);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_ctc_segment_run(const float* em, const int32_t* gtu, const int32_t* tok, const int32_t* lens, const int32_t* llens,
                         const int32_t* sel, const int32_t* utt, const int32_t* nutt, uint8_t* bp, float* ring, double* psum,
                         int32_t* info, int32_t* offsets, int32_t* timings, float* char_probs, int32_t* states, double* seg,
                         int nsel, int B, int Tmax, int Lmax, int S, int Umax, int NU, int window, int n_mean,
                         double index_duration, int ring_global, void* stream) {
  if (!em || !gtu || !tok || !lens || !llens || !sel || !utt || !nutt || !bp || !psum || !info || !offsets || !timings ||
      !char_probs || !states || !seg)
    return EAMD_EINVAL;
  if (nsel < 1 || B < 1 || nsel > B || Tmax < 1 || Lmax < 1 || S < 1 || Umax < 1 || NU < 1 || window < 1 || n_mean < 1 ||
      !(index_duration > 0.0))
    return EAMD_EINVAL;
  if (S > kMaxS) return EAMD_EUNSUPPORTED;
  const int Wmax = window < Tmax ? window : Tmax;
  const bool lds = !ring_global && ring_lds_bytes(S, Wmax) <= kLdsBytes;
  if (!lds && !ring) return EAMD_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int nt = fill_threads(Wmax);
  if (lds) {
    const int bytes = (int)ring_lds_bytes(S, Wmax);
    if (bytes > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&seg_fill_kernel<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
      if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(seg_fill_kernel<true>, dim3(nsel), dim3(nt), bytes, s, em, gtu, lens, llens, sel, bp, ring, info, offsets,
                       timings, char_probs, states, Tmax, Lmax, S, Umax, window, Wmax);
  } else {
    hipLaunchKernelGGL(seg_fill_kernel<false>, dim3(nsel), dim3(nt), kScratch * 4, s, em, gtu, lens, llens, sel, bp, ring, info,
                       offsets, timings, char_probs, states, Tmax, Lmax, S, Umax, window, Wmax);
  }
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_backtrack_kernel, dim3(nsel), dim3(64), 0, s, em, gtu, tok, lens, llens, sel, bp, info, offsets, timings,
                     char_probs, states, Tmax, Lmax, S, Umax, Wmax);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_prefix_kernel, dim3(nsel), dim3(kMaxThreads), 0, s, char_probs, lens, sel, psum, Tmax);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_segments_kernel, dim3((NU + 3) / 4, nsel), dim3(256), 0, s, timings, psum, lens, llens, sel, utt, nutt, info,
                     seg, Tmax, Lmax, NU, n_mean, index_duration);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
