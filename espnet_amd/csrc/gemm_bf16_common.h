// Shared pieces of the bf16-operand GEMM kernels (gemm_bf16.hip: general tiles; gemm_persist.hip: persistent
// short-K variant): LDS swizzles, packed-bf16 helpers, the dropout hash and the fused result epilogue.
#pragma once
#include <type_traits>
#include "common.h"
#include "../../include/espnet_amd.h"

namespace {


constexpr int BK = 64;
constexpr int NT_ = 256;
typedef __attribute__((ext_vector_type(4))) short s16x4;

// LDS images are unpadded and XOR-swizzled at 16-byte chunk granularity so that both the staging
// stores (ds_write_b128) and the fragment reads are bank-conflict free:
//   k-contiguous image [row][64]: chunk' = chunk ^ ((row >> 1) & 7)          (ds_read_b128, 16-lane groups)
//   k-strided image   [k][W]    : 32-byte slot' = slot ^ f(k)                (ds_read_b64_tr_b16, 32-lane halves)
//       W = 128: f(k) = (k & 3) | ((k >> 3) & 1) << 2 ;  W = 64: f(k) = ((k >> 1) & 1) | ((k >> 3) & 1) << 1
template <bool T, int W>
__device__ __forceinline__ int lds_chunk_off(int r, int c16) {
  if constexpr (!T) {
    return r * 64 + ((c16 ^ ((r >> 1) & 7)) << 3);
  } else if constexpr (W == 128) {
    const int f = (r & 3) | (((r >> 3) & 1) << 2);
    return r * 128 + (((((c16 >> 1) ^ f) << 1) | (c16 & 1)) << 3);
  } else {
    const int f = ((r >> 1) & 1) | (((r >> 3) & 1) << 1);
    return r * 64 + (((((c16 >> 1) ^ f) << 1) | (c16 & 1)) << 3);
  }
}

template <int BM, int BN, bool TA, bool TB>
struct SmemB {
  static constexpr int LDA = TA ? BM : BK;
  static constexpr int RA = TA ? BK : BM;
  static constexpr int LDB = TB ? BN : BK;
  static constexpr int RB = TB ? BK : BN;
  bf16_t a[2][RA * LDA];
  bf16_t b[2][RB * LDB];
  float cpad[(BM * (BN + 4) * 4 > 2 * (RA * LDA + RB * LDB) * 2) ? (BM * (BN + 4) - (RA * LDA + RB * LDB)) : 1];
  int poff[8][BK];
};

struct RowStateB { int base, ih, jw, ok; };

__device__ __forceinline__ RowStateB decompose_b(const eamd_gather_t& g, int row, int nrows) {
  RowStateB s;
  s.ok = row < nrows;
  int r = s.ok ? row : 0;
  int j = r % g.Wo; int t = r / g.Wo; int i = t % g.Ho; int b = t / g.Ho;
  s.base = b * g.Hin * g.Win; s.ih = i * g.sh; s.jw = j * g.sw;
  return s;
}
__device__ __forceinline__ long gather_off_b(const eamd_gather_t& g, const RowStateB& s, int tap) {
  int hh = s.ih + g.dh[tap], ww = s.jw + g.dw[tap];
  bool ok = s.ok && hh >= 0 && hh < g.Hin && ww >= 0 && ww < g.Win;
  return ok ? ((long)(s.base + hh * g.Win + ww)) * g.C : -1L;
}

// The tap offsets of a gather descriptor as 4-bit fields of two 64-bit scalars (host check: -8 <= dh, dw <= 7, gather_taps_fit):
// indexing eamd_gather_t.dh[tap] with a run-time tap makes the compiler keep the whole kernel argument in memory and fetch
// fields with s_load inside the K loop - and the s_waitcnt lgkmcnt(0) behind each of them also drains the wave's LDS reads.
struct GatherRegs { unsigned long long dh, dw; int C, Hin, Win; };
__device__ __forceinline__ GatherRegs gather_regs(const eamd_gather_t& g) {
  GatherRegs r;
  r.dh = 0ull; r.dw = 0ull;
#pragma unroll
  for (int tp = 0; tp < 9; ++tp) {
    r.dh |= (unsigned long long)((unsigned)(g.dh[tp] + 8) & 15u) << (4 * tp);
    r.dw |= (unsigned long long)((unsigned)(g.dw[tp] + 8) & 15u) << (4 * tp);
  }
  r.C = g.C; r.Hin = g.Hin; r.Win = g.Win;
  return r;
}
__device__ __forceinline__ long gather_off_r(const GatherRegs& g, const RowStateB& s, int tap) {
  const int hh = s.ih + (int)((g.dh >> (4 * tap)) & 15ull) - 8, ww = s.jw + (int)((g.dw >> (4 * tap)) & 15ull) - 8;
  const bool ok = s.ok && hh >= 0 && hh < g.Hin && ww >= 0 && ww < g.Win;
  return ok ? ((long)(s.base + hh * g.Win + ww)) * g.C : -1L;
}
inline bool gather_taps_fit(const eamd_gather_t& g) {
  for (int tp = 0; tp < g.ntap; ++tp)
    if (g.dh[tp] < -8 || g.dh[tp] > 7 || g.dw[tp] < -8 || g.dw[tp] > 7) return false;
  return true;
}

// 8 consecutive bf16 starting at p[idx]; `nvalid` of them are in range (0..8); vec = 16-byte path usable
__device__ __forceinline__ uint4 load8(const bf16_t* __restrict__ p, long idx, int nvalid, bool vec) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (nvalid >= 8 && vec) {
    v = *reinterpret_cast<const uint4*>(p + idx);
  } else if (nvalid > 0) {
    bf16_t e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = j < nvalid ? p[idx + j] : (bf16_t)0;
    v.x = e[0] | ((unsigned)e[1] << 16); v.y = e[2] | ((unsigned)e[3] << 16);
    v.z = e[4] | ((unsigned)e[5] << 16); v.w = e[6] | ((unsigned)e[7] << 16);
  }
  return v;
}

// Branch-free form used when every chunk start is 16-byte aligned and lies inside the tensor
// (host-checked: ld % 8 == 0, ld >= extent): invalid chunks read element 0 and are masked to zero,
// partially valid chunks are masked per element.  No control flow => the compiler keeps all of a
// tile's loads in flight behind one counted s_waitcnt instead of draining after each guarded load.
__device__ __forceinline__ unsigned mask2(int nvalid, int d) {
  const int r = nvalid - 2 * d;
  return r >= 2 ? 0xffffffffu : (r == 1 ? 0x0000ffffu : 0u);
}
// The load itself must not be followed by any use of its result (the masking happens when the
// chunk is moved to LDS, one or more MFMA phases later), otherwise hipcc waits for it on the spot.
__device__ __forceinline__ uint4 load8_fast(const bf16_t* __restrict__ p, long idx, int nvalid) {
  return *reinterpret_cast<const uint4*>(p + (nvalid > 0 ? idx : 0L));
}
__device__ __forceinline__ uint4 mask8(uint4 v, int nvalid) {
  return make_uint4(v.x & mask2(nvalid, 0), v.y & mask2(nvalid, 1), v.z & mask2(nvalid, 2), v.w & mask2(nvalid, 3));
}

// prologue activations on packed bf16 pairs; the activation kind is tested ONCE per chunk group
// (a per-element runtime switch costs hundreds of scalar branches per tile and fences the stores)
__device__ __forceinline__ unsigned swish2(unsigned w) {
  float lo = eamd_swish(__uint_as_float(w << 16));
  float hi = eamd_swish(__uint_as_float(w & 0xffff0000u));
  return (unsigned)eamd_f2bf(lo) | ((unsigned)eamd_f2bf(hi) << 16);
}
__device__ __forceinline__ unsigned relu2(unsigned w) {
  return (w & 0x00008000u ? 0u : (w & 0x0000ffffu)) | (w & 0x80000000u ? 0u : (w & 0xffff0000u));
}
__device__ __forceinline__ uint4 swish8(uint4 v) { return make_uint4(swish2(v.x), swish2(v.y), swish2(v.z), swish2(v.w)); }
__device__ __forceinline__ uint4 relu8(uint4 v) { return make_uint4(relu2(v.x), relu2(v.y), relu2(v.z), relu2(v.w)); }

// max / sum over the G = 16 or 32 adjacent lanes that hold one row of a staged result tile (DPP row operations; one
// LDS-crossbar step joins the two 16-lane rows of a 32-lane group); every lane of the group gets the result
template <int G>
__device__ __forceinline__ float rowgroup_max(float v) {
  v = fmaxf(v, eamd_dpp<0xB1>(v));
  v = fmaxf(v, eamd_dpp<0x4E>(v));
  v = fmaxf(v, eamd_dpp<0x141>(v));
  v = fmaxf(v, eamd_dpp<0x140>(v));
  if constexpr (G == 32) v = fmaxf(v, __shfl_xor(v, 16, 64));
  return v;
}
template <int G>
__device__ __forceinline__ float rowgroup_sum(float v) {
  v += eamd_dpp<0xB1>(v);
  v += eamd_dpp<0x4E>(v);
  v += eamd_dpp<0x141>(v);
  v += eamd_dpp<0x140>(v);
  if constexpr (G == 32) v += __shfl_xor(v, 16, 64);
  return v;
}

// Result tile -> global memory.  The accumulators go through an LDS staging area so that every lane stores 16
// contiguous bytes of one output row (1 KiB per wave-instruction instead of four 64-byte segments); the residual /
// aux operands are read the same way.  Fused here: bias, activation, aux-derivative masks, dropout / dual output,
// alpha, residual, beta.  `cl` must hold BM * (BN + 4) floats and be free of other readers (callers barrier before).
// PREFETCH: request the aux / residual operands of four row passes together before consuming them (costs up to
// 32 VGPRs while the epilogue runs: free in the general kernel whose ring registers are dead by then, not in the
// persistent kernel whose ring keeps running).
template <int BM, int BN, bool PREFETCH, bool ROWEPI = false>
__device__ __forceinline__ void store_c_tile(const eamd_gemm_t& p, f32x4 (&acc)[BM / 32][BN / 32], float* cl, int m0,
                                             int n0, long coff) {
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int MT = WM / 16, NTL = WN / 16;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  bf16_t* __restrict__ Cb = reinterpret_cast<bf16_t*>(p.Cb);
  const bf16_t* __restrict__ auxb = reinterpret_cast<const bf16_t*>(p.aux);
  constexpr int LDC = BN + 4;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NTL; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        cl[(wm * WM + i * 16 + fq * 4 + r) * LDC + wn * WN + j * 16 + fr] = acc[i][j][r];
  __syncthreads();

  constexpr int V4_PER_ROW = BN / 4;
  constexpr int ROWS_PER_PASS = NT_ / V4_PER_ROW;
  const int c4 = t % V4_PER_ROW;
  const int n = n0 + c4 * 4;
  const bool cvec = (p.ldc % 4 == 0) && (coff % 4 == 0) &&
                    (!p.C || (reinterpret_cast<uintptr_t>(p.C) & 15) == 0) &&
                    (!Cb || (reinterpret_cast<uintptr_t>(Cb) & 7) == 0) &&
                    (!p.Hb || (reinterpret_cast<uintptr_t>(p.Hb) & (p.h_dtype ? 15 : 7)) == 0) &&
                    (!p.R || ((p.ldr % 4 == 0) && (reinterpret_cast<uintptr_t>(p.R) & 15) == 0)) &&
                    (!p.aux || (p.ldaux % 4 == 0 && (reinterpret_cast<uintptr_t>(p.aux) & 15) == 0));
  bf16_t* __restrict__ Hb = reinterpret_cast<bf16_t*>(p.Hb);
  const unsigned drop_seed = p.drop_p > 0.f ? eamd_drop_seed((const unsigned long long*)p.drop_step, p.drop_salt) : 0u;
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if (p.bias) {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (n + e < p.N) bv[e] = p.bias[n + e];
  }
  // (ROWEPI: the two row epilogues are compiled into their own kernel instantiations only - inlined everywhere they cost
  // the ordinary epilogues 1 % of the config-2 step)
  if (ROWEPI && p.epilogue == 7) {
    // row statistics instead of the result (see eamd_gemm_t.stats): the V4_PER_ROW lanes of a row reduce their four
    // columns each to the tile's (max, sum exp) for that row; the two gathered columns leave from whichever lane holds them
    static_assert(V4_PER_ROW == 16 || V4_PER_ROW == 32, "a staged row is one or two DPP rows of lanes");
    const int tiles_n = (p.N + BN - 1) / BN, tile_n = n0 / BN;
    for (int rr = t / V4_PER_ROW; rr < BM; rr += ROWS_PER_PASS) {      // same trip count for every lane: no early exits
      const int m = m0 + rr;
      const float4 a4 = *reinterpret_cast<const float4*>(&cl[rr * LDC + c4 * 4]);
      const float v[4] = {a4.x + bv[0], a4.y + bv[1], a4.z + bv[2], a4.w + bv[3]};
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 4; ++e) if (n + e < p.N) mx = fmaxf(mx, v[e]);
      mx = rowgroup_max<V4_PER_ROW>(mx);
      float sm = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) if (n + e < p.N) sm += expf(v[e] - mx);
      sm = rowgroup_sum<V4_PER_ROW>(sm);
      if (m < p.M) {
        if (c4 == 0) {
          float* pp = p.stats.part + ((long)m * tiles_n + tile_n) * 2;
          pp[0] = mx; pp[1] = sm;
        }
        const int lc = p.stats.col ? p.stats.col[m] : -1;
        if (lc >= n && lc < n + 4 && lc < p.N) p.stats.zcol[m] = v[lc - n];
        if (p.stats.fix >= n && p.stats.fix < n + 4 && p.stats.fix < p.N) p.stats.zfix[m] = v[p.stats.fix - n];
      }
    }
    return;
  }
  if (ROWEPI && p.epilogue == 8) {
    // softmax-gradient rows (see eamd_gemm_t.stats): the recomputed logits leave as their gradient
    const float sc = p.stats.scale * (p.stats.gscale ? p.stats.gscale[0] : 1.f);
    for (int rr = t / V4_PER_ROW; rr < BM; rr += ROWS_PER_PASS) {
      const int m = m0 + rr;
      if (m >= p.M || n >= p.N) continue;
      const float4 a4 = *reinterpret_cast<const float4*>(&cl[rr * LDC + c4 * 4]);
      const float* rc = p.stats.rowc + (long)m * 3;
      const float tot = rc[0], gb = rc[1], gl = rc[2];
      const int lc = p.stats.col ? p.stats.col[m] : -1;
      float gq[4] = {a4.x + bv[0], a4.y + bv[1], a4.z + bv[2], a4.w + bv[3]};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float gv = tot > -INFINITY ? expf(gq[e] + tot) : 0.f;
        if (n + e == p.stats.fix) gv -= gb;
        if (n + e == lc) gv -= gl;
        gq[e] = tot > -INFINITY ? sc * gv : 0.f;
      }
      const long ci = coff + (long)m * p.ldc + n;
      if (cvec && n + 3 < p.N) {
        if (p.C) *reinterpret_cast<float4*>(p.C + ci) = make_float4(gq[0], gq[1], gq[2], gq[3]);
        if (Cb) {
          uint2 o;
          o.x = eamd_f2bf(gq[0]) | ((unsigned)eamd_f2bf(gq[1]) << 16);
          o.y = eamd_f2bf(gq[2]) | ((unsigned)eamd_f2bf(gq[3]) << 16);
          *reinterpret_cast<uint2*>(Cb + ci) = o;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (n + e < p.N) {
            if (p.C) p.C[ci + e] = gq[e];
            if (Cb) Cb[ci + e] = eamd_f2bf(gq[e]);
          }
      }
    }
    return;
  }
  // per-pass arithmetic + stores on values already in registers
  auto emit = [&](long ci, int nn, bool full, float (&v)[4], const float (&ax)[4], const float (&rv)[4],
                  const float (&cold)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += bv[e];
    if (p.epilogue == 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
    } else if (p.epilogue == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = eamd_swish(v[e]);
    } else if (p.epilogue == 3) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ax[e] > 0.f ? v[e] : 0.f;
    } else if (p.epilogue == 4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= eamd_dswish(ax[e]);
    } else if (p.epilogue == 5) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= ax[e];
    }
    if (p.drop_p > 0.f) {
      // wave-uniform branch; mask index = element index of the contiguous [M, N] result
      const unsigned thr = eamd_drop_thr16(p.drop_p);
      const float inv = eamd_drop_inv(thr);
      const unsigned long long base = (unsigned long long)ci;
      bool keep[4];
      if (full) {          // ci is a multiple of 4 on the vector path
        eamd_drop_keep4(drop_seed, base, thr, keep);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) keep[e] = eamd_drop_keep(drop_seed, base + e, thr);
      }
      if (Hb) {
        float h[4];
        if (p.epilogue == 6) {
          // the first output becomes the BACKWARD factor d h / d v = mask / (1 - p) * act'(v) instead of v
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float a, d;
            eamd_act_dact(v[e], p.h_act, a, d);
            h[e] = keep[e] ? a * inv : 0.f;
            v[e] = keep[e] ? d * inv : 0.f;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float a = eamd_act(v[e], p.h_act);
            h[e] = keep[e] ? a * inv : 0.f;
          }
        }
        if (p.h_dtype) {       // fp32 second output (reference-precision mode)
          float* Hf = reinterpret_cast<float*>(p.Hb);
          if (full) {
            *reinterpret_cast<float4*>(Hf + ci) = make_float4(h[0], h[1], h[2], h[3]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (nn + e < p.N) Hf[ci + e] = h[e];
          }
        } else if (full) {
          uint2 o;
          o.x = eamd_f2bf(h[0]) | ((unsigned)eamd_f2bf(h[1]) << 16);
          o.y = eamd_f2bf(h[2]) | ((unsigned)eamd_f2bf(h[3]) << 16);
          *reinterpret_cast<uint2*>(Hb + ci) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (nn + e < p.N) Hb[ci + e] = eamd_f2bf(h[e]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = keep[e] ? v[e] * inv : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] * p.alpha + rv[e] + p.beta * cold[e];
    if (full) {
      if (p.C) *reinterpret_cast<float4*>(p.C + ci) = make_float4(v[0], v[1], v[2], v[3]);
      if (Cb) {
        uint2 o;
        o.x = eamd_f2bf(v[0]) | ((unsigned)eamd_f2bf(v[1]) << 16);
        o.y = eamd_f2bf(v[2]) | ((unsigned)eamd_f2bf(v[3]) << 16);
        *reinterpret_cast<uint2*>(Cb + ci) = o;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (nn + e < p.N) {
          if (p.C) p.C[ci + e] = v[e];
          if (Cb) Cb[ci + e] = eamd_f2bf(v[e]);
        }
      }
    }
  };

  const bool want_aux = p.epilogue >= 3 && p.epilogue <= 5, want_r = p.R != nullptr, want_c = p.C && p.beta != 0.f;
  if (PREFETCH && !want_c && cvec && !p.cmap.enabled && n + 3 < p.N) {
    // fast path (aligned rows, tile column inside N): the aux / residual / beta operands of GRP row passes are
    // requested together BEFORE they are consumed, so a tile pays one memory round trip per group instead of
    // one per pass (4 dependent HBM latencies per 64-row tile dominated the epilogue of every residual GEMM)
    constexpr int PASSES = BM / ROWS_PER_PASS;
    constexpr int GRP = 4;
    static_assert(PASSES % GRP == 0, "row passes come in groups of 4");
    const int r_first = t / V4_PER_ROW;
#pragma unroll 1
    for (int g0 = 0; g0 < PASSES; g0 += GRP) {
      float4 a32[GRP], r32[GRP];      // bf16 aux rows occupy .x/.y
#pragma unroll
      for (int q = 0; q < GRP; ++q) {
        const int m = min(m0 + r_first + (g0 + q) * ROWS_PER_PASS, p.M - 1);       // clamped: always a legal row
        if (want_aux) {
          const long ai = coff + (long)m * p.ldaux + n;
          if (p.aux_dtype) {
            const uint2 u = *reinterpret_cast<const uint2*>(auxb + ai);
            a32[q].x = __uint_as_float(u.x); a32[q].y = __uint_as_float(u.y);
          } else a32[q] = *reinterpret_cast<const float4*>(p.aux + ai);
        }
        if (want_r) r32[q] = *reinterpret_cast<const float4*>(p.R + coff + (long)m * p.ldr + n);
      }
#pragma unroll
      for (int q = 0; q < GRP; ++q) {
        const int rr = r_first + (g0 + q) * ROWS_PER_PASS;
        const int m = m0 + rr;
        if (m >= p.M) continue;
        const float4 a4 = *reinterpret_cast<const float4*>(&cl[rr * LDC + c4 * 4]);
        float v[4] = {a4.x, a4.y, a4.z, a4.w};
        float ax[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f}, cold[4] = {0.f, 0.f, 0.f, 0.f};
        if (want_aux) {
          if (p.aux_dtype) {
            const unsigned ux = __float_as_uint(a32[q].x), uy = __float_as_uint(a32[q].y);
            ax[0] = bf2f(ux & 0xffff); ax[1] = bf2f(ux >> 16); ax[2] = bf2f(uy & 0xffff); ax[3] = bf2f(uy >> 16);
          } else { ax[0] = a32[q].x; ax[1] = a32[q].y; ax[2] = a32[q].z; ax[3] = a32[q].w; }
        }
        if (want_r) { rv[0] = r32[q].x; rv[1] = r32[q].y; rv[2] = r32[q].z; rv[3] = r32[q].w; }
        emit(coff + (long)m * p.ldc + n, n, true, v, ax, rv, cold);
      }
    }
    return;
  }
  for (int rr = t / V4_PER_ROW; rr < BM; rr += ROWS_PER_PASS) {
    const int m = m0 + rr;
    if (m >= p.M || n >= p.N) continue;
    long prow = m;
    if (p.cmap.enabled) {
      const eamd_rowmap_t& c = p.cmap;
      int jj = m % c.Wo; int tt = m / c.Wo; int ii = tt % c.Ho; int bb = tt / c.Ho;
      prow = ((long)bb * c.Hc + ii * c.sh + c.oh) * c.Wc + jj * c.sw + c.ow;
    }
    const float4 a4 = *reinterpret_cast<const float4*>(&cl[rr * LDC + c4 * 4]);
    float v[4] = {a4.x, a4.y, a4.z, a4.w};
    const bool full = cvec && (n + 3 < p.N);
    const long ci = coff + prow * p.ldc + n;
    float ax[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f}, cold[4] = {0.f, 0.f, 0.f, 0.f};
    if (want_aux) {
      const long ai = coff + prow * p.ldaux + n;
      if (full) {
        if (p.aux_dtype) {
          uint2 u = *reinterpret_cast<const uint2*>(auxb + ai);
          ax[0] = bf2f(u.x & 0xffff); ax[1] = bf2f(u.x >> 16); ax[2] = bf2f(u.y & 0xffff); ax[3] = bf2f(u.y >> 16);
        } else {
          float4 u = *reinterpret_cast<const float4*>(p.aux + ai);
          ax[0] = u.x; ax[1] = u.y; ax[2] = u.z; ax[3] = u.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (n + e < p.N) ax[e] = p.aux_dtype ? bf2f(auxb[ai + e]) : p.aux[ai + e];
      }
    }
    if (want_r) {
      const long ri = coff + prow * p.ldr + n;
      if (full) { float4 u = *reinterpret_cast<const float4*>(p.R + ri); rv[0] = u.x; rv[1] = u.y; rv[2] = u.z; rv[3] = u.w; }
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (n + e < p.N) rv[e] = p.R[ri + e];
      }
    }
    if (want_c) {
      if (full) { float4 u = *reinterpret_cast<const float4*>(p.C + ci); cold[0] = u.x; cold[1] = u.y; cold[2] = u.z; cold[3] = u.w; }
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (n + e < p.N) cold[e] = p.C[ci + e];
      }
    }
    emit(ci, n, full, v, ax, rv, cold);
  }
}



}  // namespace
