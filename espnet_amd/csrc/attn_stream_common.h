// What the memory-linear attention kernels share (attn_stream.hip: forward, attn_stream_bwd.hip: backward): the tile geometry, the
// fragment loads and the matrix-core product of 64-channel rows, and the operand rules of the host-side checks.  A workgroup of
// four waves owns 64 rows (queries; keys on the backward's key side), 16 per wave, and sweeps the other side in staged tiles of
// 32 rows kept as [row][STR_PLD] floats.  The header owns no LDS: tiles, barriers and the order of the global requests belong to
// the kernels.  So do the register -> LDS staging loops and the forward's context product: moved into functions here they
// compiled to other instruction streams than written out in the kernels (register allocation and schedule of the whole kernel).
#pragma once
#include "attn_common.h"

constexpr int STR_QB = 64;                        // rows a workgroup owns
constexpr int STR_KT = 32;                        // rows per staged tile
constexpr int STR_NW = STR_QB / 16;               // waves: 16 owned rows each
constexpr int STR_NT = 64 * STR_NW;
constexpr int STR_PLD = ATT_PLD;                  // row stride (floats) of a staged tile in LDS
constexpr int STR_NKT = STR_KT / 16;              // 16-row pieces of a staged tile
constexpr int STR_KQ = STR_KT * 16 / STR_NT;      // 16-byte pieces per thread of a staged tile

template <typename T>
__device__ __forceinline__ void frag_global(const T* row, int fq, float4 (&f)[4]) {   // this lane's share of a 64-channel row: chunks 4 j + fq
#pragma unroll
  for (int j = 0; j < 4; ++j) f[j] = ld4(row + 16 * j + 4 * fq);
}
__device__ __forceinline__ void frag_lds(const float* row, int fq, float4 (&f)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) f[j] = *reinterpret_cast<const float4*>(row + 16 * j + 4 * fq);
}
// c[r] += sum over the 64 channels of x[row 4 fq + r] y[row fr]: x rows / y rows held as frag_* leave them
__device__ __forceinline__ f32x4 dot64(const float4 (&x)[4], const float4 (&y)[4], f32x4 c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j].x, y[j].x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j].y, y[j].y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j].z, y[j].z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j].w, y[j].w, c, 0, 0, 0);
  }
  return c;
}

// the staged band of the legacy rel_shift: row n of the band of key tile j0 holds element c = c0 + n of the flat [0 | bd] rows
// (forward: c0 = Ts + j0 - r0w - 63); the position row behind it, clamped into [0, Ts) where the band leaves the matrix (c <= 0,
// c == Ts + 1, c > 2 Ts + 1: never used)
__device__ __forceinline__ int band_pos_row(int c, int Ts) {
  const int m = c <= Ts ? c - 1 : c - Ts - 2;
  return min(max(m, 0), Ts - 1);
}

// ---- attention dropout (the *_drop entry points) ----
// No probability is stored, but the keep bits are those the stored route draws (attn_f32.hip / attn_fused.hip, ops.dropout on P):
// element (z = h B + b, i, j) of P in ITS layout [H*B][T1][ldp] is kept iff eamd_dropout keeps index (z T1 + i) ldp + j at
// (drop_step, drop_salt) - a 64-bit index: H B T1 ldp passes 2^32 at the lengths these kernels exist for.  The generator is
// counter-based, so forward and the three backward sweeps regenerate a tile's bits from the indices of the score elements a lane
// holds in its accumulator, and the two routes are interchangeable at a given (step, salt).
// the row stride the stored route gives P (functional._ldp): T2 rounded up to 8 elements
inline long stream_ldp(int T2) { return ((long)T2 + 7) / 8 * 8; }
// a row's layout (query side): w[kt][r] = key j0 + 16 kt + 4 fq + r of the query whose P row starts at element pro - eight
// four-key pieces of a staged tile per row, two per lane, each drawn as attn_keep4 draws it (clamped at the row's last piece:
// only pieces wholly past T2 are, and their probabilities are zero by index).  w <- keep ? w / (1 - p) : 0
__device__ __forceinline__ void stream_drop_row(const AttnDrop& d, long pro, int j0, int fq, long ldp, f32x4 (&w)[STR_NKT]) {
#pragma unroll
  for (int kt = 0; kt < STR_NKT; ++kt) {
    bool kp[4];
    attn_keep4(d, pro, j0 + 16 * kt + 4 * fq, ldp, kp);
#pragma unroll
    for (int r = 0; r < 4; ++r) w[kt][r] = kp[r] ? w[kt][r] * d.dinv : 0.f;
  }
}
// a column's layout (key side, position side): the lane's four elements lie `stride` apart in P (ldp: four queries of one key;
// ldp + 1: four queries of one diagonal), so each takes the half of its own pair's hash.  m[r] = keep ? 1 / (1 - p) : 0 of
// element e0 + r stride; elements outside the matrix draw bits nobody uses (their probability is zero by index)
__device__ __forceinline__ void stream_keep_col(const AttnDrop& d, long e0, long stride, float (&m)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) m[r] = eamd_drop_keep(d.seed, (unsigned long long)(e0 + r * stride), d.thr) ? d.dinv : 0.f;
}

// operand rules of both directions; a matrix that breaks one makes the entry point decline (EAMD_EUNSUPPORTED) before any launch.
// Read in 16-byte pieces: 16-byte aligned, row stride a multiple of 16 bytes
template <typename T>
inline bool stream_in_ok(const T* p, long ld) { return ld % (16 / (long)sizeof(T)) == 0 && al16(p); }
// written in pieces of four elements inside its 64 columns
template <typename T>
inline bool stream_out_ok(const T* p, long ld) { return ld % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0; }
