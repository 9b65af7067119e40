// What the fused attention kernels share (attn_f32.hip: fp32 short rows, long rows in both storage types, fp32 key side;
// attn_fused.hip: bf16 short rows, bf16 key side): everything about attention that is not a matrix product - the argument
// structs, the decoding of a workgroup, the legacy rel_shift's length and inverse map, mask and score, the dropout of a
// four-key piece, and the host-side checks and launch.  Device and host code, everything
// inlined, no LDS of its own: callers pass their arrays by reference and keep their MFMA products, fragment loads, staging,
// LDS layouts, barriers and request order.
// reference: transformer/attention.py:63-114 (forward_attention), :141-206 (rel_shift, (ac + bd) / sqrt(d_k)).
#pragma once
#include "common.h"

constexpr int ATT_DK = 64;
constexpr int ATT_MAXK = 512;          // keys per row of the short kernels: 8 / 16 key tiles of 16 at two workgroups per CU, 32 at one (LDS)
constexpr int ATT_LONG_MAXK = 4096;    // of the long-row kernels
constexpr int ATT_PLD = 68;            // row stride (floats) of an fp32 V / K panel or tile in LDS

// ---- arguments: T = storage type of the operands and of P / dS / dbd / ctx (float, or bf16_t = bf16 bits) ----
template <typename T>
struct AttnArgs {
  const T* qu; const T* qv; const T* k; const T* v; const T* pos;
  const unsigned char* mask;
  T* P; T* ctx;
  long ldq, ldqv, ldk, ldv, ldpos, ldc, ldp, mb, mi;
  int B, H, T1, T2, nqb;
  float scale;
  // attention dropout (attention.py:91): Pd = dropout(P) feeds the context; mask index = element index in P
  T* Pd; float drop_p; const unsigned long long* drop_step; unsigned long long drop_salt;
  const int* tshift;     // device scalar: length the legacy rel_shift works on (NULL: T2) - see attn_shift_len
};
// (the short bf16 backward takes a copy of this struct in its own field order, AttnBwdArgs16 in attn_fused.hip: a field added
// here must be added there)
template <typename T>
struct AttnBwdArgs {
  const T* dctx; const T* k; const T* v; const T* P;
  T* dS; T* dbd; void* dq;                       // dq: fp32, or bf16 where the launch's dq_bf16 says so (bf16 operands only)
  long ldd, ldk, ldv, ldp, ldo;
  int B, H, T1, T2, nqb;
  float scale;
  float drop_p; const unsigned long long* drop_step; unsigned long long drop_salt;   // the forward's attention dropout
  const int* tshift;
};

// bf16-operand mode, rows of 513 .. ATT_LONG_MAXK keys: defined in attn_f32.hip beside the kernels, called by eamd_attn_fwd /
// eamd_attn_bwd_q (attn_fused.hip), which have validated the operands
int eamd_attn_long_fwd_bf16(const AttnArgs<bf16_t>& a, hipStream_t stream);
int eamd_attn_long_bwd_q_bf16(const AttnBwdArgs<bf16_t>& a, int dq_bf16, hipStream_t stream);

// ---- element access for the two storage types ----
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4(const bf16_t* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  return make_float4(bf2f(u.x & 0xffffu), bf2f(u.x >> 16), bf2f(u.y & 0xffffu), bf2f(u.y >> 16));
}
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void st4(bf16_t* p, float4 v) { *reinterpret_cast<uint2*>(p) = eamd_pack_bf16x4(v); }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(bf16_t* p, float v) { *p = eamd_f2bf(v); }
__device__ __forceinline__ float rnd(const float*, float v) { return v; }                      // value as the storage type keeps it
__device__ __forceinline__ float rnd(const bf16_t*, float v) { return bf2f(eamd_f2bf(v)); }
__device__ __forceinline__ float4 f4(const f32x4& c) { return make_float4(c[0], c[1], c[2], c[3]); }

// reductions over the four 16-lane groups of a wave (a softmax row is spread over lanes fr, fr + 16, fr + 32, fr + 48)
__device__ __forceinline__ float attn_max16_32(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float attn_sum16_32(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// ---- geometry ----
// (batch, head) pairs are dealt to the XCDs in contiguous runs, so the blocks of one pair share an L2: workgroup `bid` of a
// grid of nblk x (pairs rounded up to 8) is block `blk` of pair z = h * B + b, as the score tensors are laid out
__device__ __forceinline__ int attn_xcd_pair(unsigned bid, int nblk) {
  const int xcd = bid & 7, jb = bid >> 3;
  return (jb / nblk) * 8 + xcd;
}
__device__ __forceinline__ int attn_xcd_block(unsigned bid, int nblk) {
  const int jb = bid >> 3;
  return jb % nblk;
}
// a query-side workgroup of LQ queries.  live: whole workgroup (dead ones only keep the barriers company, on pair 0);
// r0w: its first query; nq = T1 - r0w: the queries from there on - it may exceed LQ (callers clamp rows with min(.., nq - 1))
struct AttnGeom { bool live; int zz, h, b, r0w, nq; };
__device__ __forceinline__ AttnGeom attn_geom(unsigned bid, int nqb, int B, int H, int T1, int LQ) {
  AttnGeom g;
  const int z = attn_xcd_pair(bid, nqb);
  g.live = z < B * H;
  g.zz = g.live ? z : 0;
  g.h = g.zz / B; g.b = g.zz % B;
  g.r0w = min(attn_xcd_block(bid, nqb) * LQ, T1 - 1);
  g.nq = T1 - g.r0w;
  return g;
}

// ---- the legacy rel_shift (attention.py:141-162) for T1 == T2 ----
// It is a flat re-indexing of bd padded with a zero column: shifted[i][j] = bd[i][Ts-1-i+j] for j <= i, 0 for j = i + 1,
// bd[i+1][j-i-2] above - one-to-one, so the forward STORES the bd tiles at their shifted place and the backward scatters the
// score gradient back.  (eamd_softmax_fwd / bwd in rowops.hip do the same map in its flat-index form.)
// The forward kernels write the map out at their stores - bd[i][m] goes to (i, m - lim) if m >= lim = Ts - 1 - i, else to
// (i - 1, m + i + 1), under the guard m < Ts && i < Ts && row >= 0 - because as a function it changed their code; the inverse is here.
// Ts: the length the shift is taken over.  A batch padded beyond its own longest utterance (shape-bucketed graphs) passes that
// utterance's length: the shift then maps bd exactly as the reference's Ts x Ts matrix does; keys from Ts on are masked by the
// caller's mask, and the forward clears its score matrix first so that what the shift no longer reaches holds zeros.
__device__ __forceinline__ int attn_shift_len(const int* tshift, int T2) { return tshift ? min(max(tshift[0], 1), T2) : T2; }
// the inverse: shifted[i][j] (i, j < Ts) comes from column c of row R of [0 | bd], i.e. from bd[R][c - 1], or from the zero column (c == 0)
__host__ __device__ __forceinline__ void attn_shift_src(int i, int j, int Ts, int& R, int& c) {
  R = j <= i ? i : i + 1;
  c = j <= i ? Ts + j - i : j - i - 1;
}
// backward: gradient g of shifted[i][j] -> dbd (this (batch, head)'s [T][ldp] starts at zo), element by element exactly as
// eamd_softmax_bwd does; everything outside the Ts x Ts square is zero: the pad columns of row i are written here ...
template <typename T>
__device__ __forceinline__ void attn_dbd_put(T* dbd, long zo, long ldp, int i, int j, int Ts, float g) {
  if (j < Ts && i < Ts) {
    int R, c;
    attn_shift_src(i, j, Ts, R, c);
    if (c != 0) st1(dbd + zo + (long)R * ldp + (c - 1), g);
  } else if (j < (int)ldp) {
    st1(dbd + zo + (long)i * ldp + j, 0.f);
  }
}
// ... and the head of row 0, which the scatter never reaches, by the nt threads that own query 0
template <typename T>
__device__ __forceinline__ void attn_dbd_zero_head(T* dbd, long zo, int Ts, int t, int nt) {
  for (int f = 1 + t; f < Ts; f += nt) st1(&dbd[zo + (f - 1)], 0.f);
}

// ---- mask and scores ----
// mask bytes of keys j0 .. j0 + 3 of one mask row, one per byte: unconditional clamped loads (a load behind a lane-dependent
// guard is waited for on the spot); keys past T2 are masked by index in attn_score
__device__ __forceinline__ unsigned attn_mask4(const unsigned char* mr, int j0, int T2) {
  return mr[min(j0, T2 - 1)] | (mr[min(j0 + 1, T2 - 1)] << 8) | (mr[min(j0 + 2, T2 - 1)] << 16) | (mr[min(j0 + 3, T2 - 1)] << 24);
}
// the scaled score of key j = piece element r of mask word mk; -inf past T2 or where masked
__device__ __forceinline__ float attn_score(float x, float scale, int j, int T2, unsigned mk, int r) {
  x *= scale;
  if (j >= T2 || ((mk >> (8 * r)) & 0xffu) == 0u) x = -INFINITY;
  return x;
}

// ---- attention dropout of a four-key piece ----
// The backward must draw exactly the forward's bits: both index the piece of row offset `pro` at key j0 as the 16-byte access
// to P does, clamped to the row's last piece.
struct AttnDrop { unsigned seed, thr; float dinv; bool on; };
__device__ __forceinline__ AttnDrop attn_drop_setup(float p, const unsigned long long* step, unsigned long long salt) {
  AttnDrop d;
  d.on = p > 0.f;                                    // wave-uniform
  d.seed = p > 0.f ? eamd_drop_seed(step, salt) : 0u;
  d.thr = eamd_drop_thr16(p);
  d.dinv = eamd_drop_inv(d.thr);
  return d;
}
__device__ __forceinline__ void attn_keep4(const AttnDrop& d, long pro, int j0, long ldp, bool (&kp)[4]) {
  eamd_drop_keep4(d.seed, (unsigned long long)(pro + min(j0, (int)ldp - 4)), d.thr, kp);
}

// ---- host ----
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int attn_nkt(int T2) { return T2 <= 128 ? 8 : T2 <= 256 ? 16 : 32; }      // key tiles of 16 a short instantiation covers
inline unsigned attn_grid(int nblk, int B, int H) { return (unsigned)(nblk * ((B * H + 7) / 8 * 8)); }
// LDS bytes of a long-row workgroup: X[lq][16 nkt + 4], a tile buffer per wave, the two reduction arrays
inline size_t attn_long_lds(int lq, int nw, int nkt) {
  return ((size_t)lq * (nkt * 16 + 4) + nw * 16 * ATT_PLD + 2 * nw * lq) * sizeof(float);
}

// the C entry points' parameters, in their order, as the argument structs (nqb: blocks of 64 queries; the long rows set their own)
template <typename T>
inline AttnArgs<T> attn_args(const void* qu, int64_t ldq, const void* qv, int64_t ldqv, const void* k, int64_t ldk, const void* v,
                             int64_t ldv, const void* pos, int64_t ldpos, const unsigned char* mask, int64_t mb, int64_t mi, void* P,
                             int64_t ldp, void* ctx, int64_t ldc, int B, int H, int T1, int T2, float scale, void* Pd, float drop_p,
                             const uint64_t* drop_step, uint64_t drop_salt, const int32_t* shift_len) {
  AttnArgs<T> a;
  a.qu = (const T*)qu; a.qv = (const T*)qv; a.k = (const T*)k; a.v = (const T*)v; a.pos = (const T*)pos;
  a.mask = mask; a.P = (T*)P; a.ctx = (T*)ctx;
  a.ldq = ldq; a.ldqv = ldqv; a.ldk = ldk; a.ldv = ldv; a.ldpos = ldpos; a.ldc = ldc; a.ldp = ldp; a.mb = mb; a.mi = mi;
  a.B = B; a.H = H; a.T1 = T1; a.T2 = T2; a.nqb = (T1 + 63) / 64; a.scale = scale;
  a.Pd = (T*)Pd; a.drop_p = drop_p; a.drop_step = (const unsigned long long*)drop_step; a.drop_salt = drop_salt;
  a.tshift = shift_len;
  return a;
}
template <typename T>
inline AttnBwdArgs<T> attn_bwd_args(const void* dctx, int64_t ldd, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* P,
                                    int64_t ldp, void* dS, void* dbd, void* dq, int64_t ldo, int B, int H, int T1, int T2,
                                    float scale, float drop_p, const uint64_t* drop_step, uint64_t drop_salt, const int32_t* shift_len) {
  AttnBwdArgs<T> a;
  a.dctx = (const T*)dctx; a.k = (const T*)k; a.v = (const T*)v; a.P = (const T*)P;
  a.dS = (T*)dS; a.dbd = (T*)dbd; a.dq = dq;
  a.ldd = ldd; a.ldk = ldk; a.ldv = ldv; a.ldp = ldp; a.ldo = ldo;
  a.B = B; a.H = H; a.T1 = T1; a.T2 = T2; a.nqb = (T1 + 63) / 64; a.scale = scale;
  a.drop_p = drop_p; a.drop_step = (const unsigned long long*)drop_step; a.drop_salt = drop_salt;
  a.tshift = shift_len;
  return a;
}

// The argument checks of the query-side entry points; they return before anything is launched.  Leading dimensions of the
// operands and of P are multiples of the 16-byte unit U (4 fp32 / 8 bf16 elements) and the pointers 16-byte aligned; ctx / dq
// rows are written in pieces of four elements.
inline int attn_check_common(bool operands, int B, int H, int T1, int T2, float drop_p, const void* drop_step) {
  if (!operands || B <= 0 || H <= 0 || T1 <= 0 || T2 <= 0) return EAMD_EINVAL;
  if (drop_p < 0.f || drop_p >= 1.f || (drop_p > 0.f && !drop_step)) return EAMD_EINVAL;
  return EAMD_OK;
}
// the grid limit, counted in the blocks each file always has: 64 queries (fp32), 16 (bf16: its long rows included)
template <typename T>
inline bool attn_too_many(int B, int H, int T1) {
  constexpr int QB = sizeof(T) == 4 ? 64 : 16;
  return (long)B * H * ((T1 + QB - 1) / QB) >= (1L << 28);
}
template <typename T>
inline int attn_check_fwd(const AttnArgs<T>& a, int dk) {
  constexpr int U = 16 / sizeof(T);
  if (const int rc = attn_check_common(a.qu && a.k && a.v && a.P && a.ctx, a.B, a.H, a.T1, a.T2, a.drop_p, a.drop_step)) return rc;
  if (a.drop_p > 0.f && (!a.Pd || !al16(a.Pd))) return EAMD_EINVAL;
  if ((a.pos == nullptr) != (a.qv == nullptr)) return EAMD_EINVAL;
  if (dk != ATT_DK || a.T2 > ATT_LONG_MAXK || (a.pos && a.T1 != a.T2)) return EAMD_EUNSUPPORTED;
  if (a.ldq % U || a.ldk % U || a.ldv % U || a.ldc % 4 || a.ldp % U || a.ldp < a.T2 || (a.pos && (a.ldqv % U || a.ldpos % U)))
    return EAMD_EUNSUPPORTED;
  if (!al16(a.qu) || !al16(a.k) || !al16(a.v) || !al16(a.P) || (reinterpret_cast<uintptr_t>(a.ctx) & (4 * sizeof(T) - 1)) ||
      (a.pos && (!al16(a.qv) || !al16(a.pos))))
    return EAMD_EUNSUPPORTED;
  return attn_too_many<T>(a.B, a.H, a.T1) ? EAMD_EUNSUPPORTED : EAMD_OK;
}
template <typename T>
inline int attn_check_bwd(const AttnBwdArgs<T>& a, int dk, int dq_bf16) {
  constexpr int U = 16 / sizeof(T);
  if (const int rc = attn_check_common(a.dctx && a.k && a.v && a.P && a.dS && a.dq, a.B, a.H, a.T1, a.T2, a.drop_p, a.drop_step)) return rc;
  if (dk != ATT_DK || a.T2 > ATT_LONG_MAXK || (a.dbd && a.T1 != a.T2)) return EAMD_EUNSUPPORTED;
  if (a.ldd % U || a.ldk % U || a.ldv % U || a.ldp % U || a.ldp < a.T2 || a.ldo % 4) return EAMD_EUNSUPPORTED;
  if (!al16(a.dctx) || !al16(a.k) || !al16(a.v) || !al16(a.P) || !al16(a.dS) || (reinterpret_cast<uintptr_t>(a.dq) & (dq_bf16 ? 7 : 15)))
    return EAMD_EUNSUPPORTED;
  return attn_too_many<T>(a.B, a.H, a.T1) ? EAMD_EUNSUPPORTED : EAMD_OK;
}

// One launch: KERNEL's dynamic-LDS ceiling is raised once per instantiation, then the grid goes out
template <auto KERNEL, typename... A>
inline int attn_launch(int lds_ceiling, unsigned grid, unsigned block, size_t smem, hipStream_t stream, const A&... args) {
  static const hipError_t attr_err = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, lds_ceiling);
  if (attr_err != hipSuccess) return (int)attr_err;
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(block), smem, stream, args...);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}
