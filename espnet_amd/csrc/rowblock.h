// What the row-block kernels share (ffn_f32.hip, ffn_bf16.hip, rowproj_f32.hip): one workgroup of RB_NT threads takes RB_M rows
// through a whole product - the rows staged once in LDS (optionally normalised on the way), the weights read from a packed image
// in MFMA fragment order through a ring of four register sets, the results leaving through bias / dropout / alpha / residual or
// through the LayerNorm backward (ln_bwd_rows.h).  Device and host code, everything inlined, no LDS of its own: callers pass
// their arrays and register arrays by reference, and keep their own step / period structure, barriers and request order.
#pragma once
#include <stdint.h>
#include "common.h"
#include "../../include/espnet_amd.h"
#include "ln_bwd_rows.h"

// ---- geometry ----
constexpr int RB_M = 32;         // rows per workgroup: two 16-row MFMA tiles
constexpr int RB_NT = 512;       // threads per workgroup: 8 waves, two per SIMD
constexpr int RB_D = 256;        // model width: the row length of every LayerNorm and of the feed-forward block
// LDS row stride of a staged [RB_M][K] tile, in elements.  The 8 elements of padding make the row stride 2 mod 16 16-byte chunks
// (fp32), so the 16 rows x 4 k-groups of an A-fragment read (ds_read_b128) fall into distinct bank groups: conflict-free.
__host__ __device__ constexpr int rb_ld(int K) { return K + 8; }

inline bool rb_al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// ---- staging ----
// LayerNorm of the RB_M input rows while they are staged (p.ln_x [M, RB_D] fp32; eamd_ffn_t and eamd_rowproj_t name the ln_* fields alike).
// reference: transformer/layer_norm.py:12-38 in front of positionwise_feed_forward.py:12-32 / attention.py / convolution.py
// (conformer/encoder_layer.py:96-135).
// Thread t owns row t >> 4, columns 4 (l + 16 j) .. + 3 (l = t & 15, j = 0 .. 3) - a row is 16 lanes of one wave, so both row
// sums are four DPP exchanges.  Same arithmetic as layernorm_fwd_vec_kernel (rowops.hip): mean, then the centred sum of squares
// of the values held in registers, rsqrt(var + eps).  put(row, col, y4) stores a normalised piece in the caller's LDS image;
// keep(global_row, col, y4) stores it for backward's weight gradient (rows of this launch only); mean / rstd go to ln_mean / ln_rstd.
template <typename P, typename Put, typename Keep>
__device__ __forceinline__ void rb_stage_ln(const P& p, const int m0, const int t, Put&& put, Keep&& keep) {
  constexpr int D = RB_D;
  const int row = t >> 4, l = t & 15;
  const bool live = m0 + row < p.M;
  const long gr = (long)min(m0 + row, p.M - 1);
  const float4* __restrict__ xr = reinterpret_cast<const float4*>(p.ln_x + gr * D);
  float4 v[4];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[j] = xr[l + 16 * j]; s += v[j].x + v[j].y + v[j].z + v[j].w; }
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) s += __shfl_xor(s, m);
  const float mean = s / D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, d = v[j].w - mean;
    q += a * a + b * b + c * c + d * d;
  }
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) q += __shfl_xor(q, m);
  const float rstd = rsqrtf(q / D + p.ln_eps);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(p.ln_w);
  const float4* __restrict__ b4 = reinterpret_cast<const float4*>(p.ln_b);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 g = g4[l + 16 * j], b = b4[l + 16 * j];
    float4 o;
    o.x = (v[j].x - mean) * rstd * g.x + b.x;
    o.y = (v[j].y - mean) * rstd * g.y + b.y;
    o.z = (v[j].z - mean) * rstd * g.z + b.z;
    o.w = (v[j].w - mean) * rstd * g.w + b.w;
    const int col = (l + 16 * j) * 4;
    put(row, col, o);
    if (live) keep(gr, col, o);
  }
  if (live && l == 0) { p.ln_mean[gr] = mean; p.ln_rstd[gr] = rstd; }
}

// the RB_M fp32 rows m0 .. of a [M, K] (row stride lda) as they are -> xs[RB_M][ld]; rows past M repeat the last one
__device__ __forceinline__ void rb_stage_rows(float* xs, const int ld, const float* a, const long lda, const int K, const int m0,
                                              const int M, const int t) {
  const int c4n = K >> 2;             // 16-byte pieces per row
  for (int idx = t; idx < RB_M * c4n; idx += RB_NT) {
    const int row = idx / c4n, c4 = idx - row * c4n;
    *reinterpret_cast<f32x4*>(&xs[row * ld + c4 * 4]) = *reinterpret_cast<const f32x4*>(a + (long)min(m0 + row, M - 1) * lda + c4 * 4);
  }
}

// ---- the weight ring and the fp32 32 x 32 wave tile (v_mfma_f32_16x16x4_f32) ----
// one K-step's operand fragments of this lane from a packed image: 4 x 16 bytes, 1 KB apart (a wave instruction reads 1 KB of
// consecutive bytes); `base` = the step's block + the wave's + lane * 16, the step clamped to the last by the caller
template <int SET>
__device__ __forceinline__ void rb_load_b(f32x4 (&bs)[4][4], const char* base) {
#pragma unroll
  for (int v = 0; v < 4; ++v) bs[SET][v] = *reinterpret_cast<const f32x4*>(base + v * 1024);
}

// A fragments of half HALF (16 k) of a K-step for both row tiles: row i * 16 + fr, 4 k-elements at col + HALF * 16 (col = the
// step's first column + fq * 4)
template <int HALF>
__device__ __forceinline__ void rb_read_a(float (&fA)[2][2][4], const float* xs, const int ld, const int fr, const int col) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float4 v = *reinterpret_cast<const float4*>(&xs[(i * 16 + fr) * ld + col + HALF * 16]);
    fA[HALF][i][0] = v.x; fA[HALF][i][1] = v.y; fA[HALF][i][2] = v.z; fA[HALF][i][3] = v.w;
  }
}

// 16 MFMAs: half Q of a K-step onto the 2 x 2 accumulator tiles.  bs[SET][Q * 2 + j] = 4 k-elements of column tile j (weights
// contiguous along k); KSTRIDED (weights contiguous along n): bs[SET][Q * 2 + e / 2] = (e even: j0 j1, e odd: j0 j1)
template <int SET, int Q, bool KSTRIDED>
__device__ __forceinline__ void rb_mfma_half(f32x4 (&acc)[2][2], const float (&fA)[2][2][4], const f32x4 (&bs)[4][4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float b = KSTRIDED ? bs[SET][Q * 2 + (e >> 1)][(e & 1) * 2 + j] : bs[SET][Q * 2 + j][e];
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fA[Q][i][e], b, acc[i][j], 0, 0, 0);
      }
}

// ---- output pieces ----
struct RbDrop { unsigned thr; float inv; unsigned seed; bool on; };
// eamd_dropout's mask parameters for probability prob (0: off; the step counter is not read then)
__device__ __forceinline__ RbDrop rb_drop_setup(const float prob, const unsigned long long salt, const void* drop_step) {
  RbDrop d;
  d.thr = eamd_drop_thr16(prob);
  d.inv = eamd_drop_inv(d.thr);
  d.on = prob > 0.f;
  d.seed = d.on ? eamd_drop_seed((const unsigned long long*)drop_step, salt) : 0u;
  return d;
}

// one 16-byte output piece: (a + bias), dropout by the mask of element gi .. gi + 3 of the contiguous result, * alpha + r.
// bias / R = base pointers that are the same for the whole workgroup, or NULL for none (the NULL tests stay scalar branches:
// a pointer selected per lane made them vector compares in rowproj_f32_kernel); b_off / r_off = this piece's offset in floats.
__device__ __forceinline__ float4 rb_out4(const float4 a, const float* bias, const long b_off, const RbDrop& d,
                                          const unsigned long long gi, const float alpha, const float* R, const long r_off) {
  float v[4] = {a.x, a.y, a.z, a.w};
  if (bias) {
    const float4 b4 = *reinterpret_cast<const float4*>(bias + b_off);
    v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w;
  }
  if (d.on) {
    bool keep[4];
    eamd_drop_keep4(d.seed, gi, d.thr, keep);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = keep[e] ? v[e] * d.inv : 0.f;
  }
  float4 r4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (R) r4 = *reinterpret_cast<const float4*>(R + r_off);
  return make_float4(v[0] * alpha + r4.x, v[1] * alpha + r4.y, v[2] * alpha + r4.z, v[3] * alpha + r4.w);
}

// ---- the LayerNorm in front / the LayerNorm backward behind: arguments and host-side checks (P = eamd_ffn_t or eamd_rowproj_t) ----
template <typename P>
__device__ __forceinline__ EamdLnbArgs rb_lnb_args(const P& p, float* out, const long ldo) {
  return EamdLnbArgs{p.lnb_x, p.lnb_gamma, p.lnb_mean, p.lnb_rstd, p.lnb_dres, p.lnb_ws, p.lnb_drop_out, p.lnb_drop_p,
                     (unsigned long long)p.lnb_drop_salt, p.drop_step, out, ldo, p.M};
}

template <typename P>
int rb_check_ln(const P& p) {       // p.ln_x is set; the caller's own conditions (all EAMD_EINVAL) come first
  if (!p.ln_w || !p.ln_b || !p.ln_mean || !p.ln_rstd) return EAMD_EINVAL;
  if (!rb_al16(p.ln_x) || !rb_al16(p.ln_w) || !rb_al16(p.ln_b)) return EAMD_EUNSUPPORTED;
  return EAMD_OK;
}

template <typename P>
int rb_check_lnb(const P& p) {      // p.lnb_x is set; the caller's own conditions (all EAMD_EINVAL) come first
  if (!p.lnb_gamma || !p.lnb_mean || !p.lnb_rstd || !p.lnb_ws) return EAMD_EINVAL;
  if (p.lnb_drop_out && (!p.drop_step || p.lnb_drop_p < 0.f || p.lnb_drop_p >= 1.f)) return EAMD_EINVAL;
  if (!rb_al16(p.lnb_x) || !rb_al16(p.lnb_gamma) || (p.lnb_dres && !rb_al16(p.lnb_dres)) || (p.lnb_drop_out && !rb_al16(p.lnb_drop_out)))
    return EAMD_EUNSUPPORTED;
  return EAMD_OK;
}
