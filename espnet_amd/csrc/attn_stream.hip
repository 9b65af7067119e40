// Memory-linear attention forward for inference, d_k = 64, any number of keys, fp32 or bf16 storage, on the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32): ctx = softmax(mask(scale (qu k^T + rel_shift(qv pos^T)))) v with an ONLINE softmax - no score and
// no probability ever reaches global memory, so the only output is ctx and memory is O(T).  Forward only: the kernels of
// attn_f32.hip / attn_fused.hip store P because training reads it again, and keep a query block's whole score row in LDS,
// which is why they stop at ATT_LONG_MAXK keys.
// reference: transformer/attention.py:63-114 (forward_attention), :141-206 (rel_shift, (ac + bd) / sqrt(d_k)).
//
// One workgroup = one (batch, head) pair x QB = 64 queries, four waves; pairs are dealt to the XCDs as in the other attention
// kernels (attn_xcd_pair / attn_xcd_block).  Wave w owns queries 16 w .. 16 w + 15 for the whole sweep over the keys: running row
// maximum, running denominator and the 16 x 64 context accumulator (transposed, C^T[channel][query]: a lane holds four adjacent
// channels of query fr, so the per-query rescale is lane-local) stay in registers and no wave ever waits for another one's
// numbers.  The keys are walked in tiles of KT = 32:
//   * the workgroup stages K, V and - with positions - the band of `pos` rows the (query block, key tile) needs in LDS, once,
//     for its four waves ([row][68] floats, bf16 widened on the way).  Staging is register-staged: the global loads of tile
//     t + 1 are issued right after tile t has been stored to LDS, ahead of tile t's products, and land in registers while the
//     matrix cores work.  Two LDS copies of every buffer (87 KB) would leave one workgroup per CU; one copy is 56.8 KB with
//     positions (17.4 KB without), so TWO workgroups share a CU's 160 KB - eight waves per CU, where the long-row kernels
//     were measured to be bound by fragment-load latency at four;
//   * scores S^T[key][query] = K_tile qu^T: A operand from the K tile in LDS (16-byte reads), B operand the wave's query
//     fragments, loaded once from global memory; the accumulator holds four adjacent keys of query fr - which IS the B-operand
//     layout of the context product C^T += V_tile^T P^T, so the probabilities never leave their registers;
//   * the legacy rel_shift is applied by its inverse, as a gather.  shifted[i][j] is element c = Ts + j - i of row i of [0 | bd]
//     read flat: bd[i][c - 1] for c <= Ts, the zero column for c == Ts + 1, bd[i + 1][c - Ts - 2] above.  For a query block
//     r0 .. r0 + 63 and keys j0 .. j0 + KT - 1, c runs over ONE contiguous band of KT + 63 values, so the staged band is
//     pos row c - 1 (or c - Ts - 2) for c = c0 .. c0 + KT + 62, every row index clamped into [0, Ts).  A wave takes KT + 16 band
//     rows (KT / 16 + 1 column tiles) against its qv rows i (lower part) or i + 1 (upper part; the one column tile that holds
//     c == Ts + 1 is computed against both and selected per element), writes G[query][band row] to a private LDS tile and
//     reads its skewed slice back: shifted[a][jj] = G[a][jj + 15 - a].  Tiles wholly below / above the diagonal cost
//     KT / 16 + 1 products, the few on it one more.
// Hazards: a key tile that is entirely masked while the running maximum is still -inf subtracts 0 instead of -inf (every
// exponential is then exp(-inf) = 0 and the accumulator stays 0); a row masked everywhere ends with denominator 0 and is
// written as zeros; V rows past T2 are staged as zeros, K / pos / q rows are clamped re-reads whose scores are masked or
// whose queries are never stored.
#include "attn_stream_common.h"

namespace {

constexpr int SBR = STR_KT + STR_QB;             // band rows staged (KT + QB - 1 are used)
constexpr int SNBT = STR_NKT + 1;                // 16-row column tiles of a wave's band
constexpr int SGLD = 16 * SNBT + 4;           // row stride of a wave's band tile G[16][KT + 16]
constexpr int SBQ = SBR * 16 / STR_NT;           // 16-byte pieces per thread of the band

// LSE (training, attn_stream_bwd.hip): each wave also writes lse[z][i] = running maximum + log(denominator) of its 16 queries - the
// row statistic of the scaled, masked scores the streamed backward rebuilds P from; 0 for a row masked everywhere
// DROP (attention dropout, the *_drop entry points; lse may then be NULL): the tile's weights e_ij go into the running denominator
// as they are - row maximum, denominator and lse stay those of the undropped scores - and the copy that feeds the context product
// takes the stored route's keep bits and 1 / (1 - p) (stream_drop_row): ctx = (P o M / (1 - p)) v after the final 1 / denominator
template <typename T, bool REL, bool LSE, bool DROP = false>
__global__ __launch_bounds__(STR_NT, 2) void attn_stream_kernel(const AttnArgs<T> a, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) float Ks[STR_KT * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Vs[STR_KT * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Ps[REL ? SBR * STR_PLD : 4];
  __shared__ __attribute__((aligned(16))) float Gs[REL ? STR_NW * 16 * SGLD : 4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int z = attn_xcd_pair(blockIdx.x, a.nqb);            // z = h * B + b
  if (z >= a.B * a.H) return;                                // whole workgroup
  const int h = z / a.B, b = z % a.B;
  const int T1 = a.T1, T2 = a.T2;
  const int r0w = attn_xcd_block(blockIdx.x, a.nqb) * STR_QB;   // < T1: nqb = ceil(T1 / QB)
  const int i0 = r0w + 16 * wave;
  const bool active = i0 < T1;                               // wave-uniform; idle waves still stage and keep the barriers
  const int i = i0 + fr;                                     // this lane's query (rows past T1 are clamped re-reads, never stored)
  const int qi = min(i, T1 - 1);
  const int Ts = REL ? attn_shift_len(a.tshift, T2) : T2;
  const int ntile = (T2 + STR_KT - 1) / STR_KT;
  const T* ks = a.k + (long)b * T2 * a.ldk + h * ATT_DK;
  const T* vs = a.v + (long)b * T2 * a.ldv + h * ATT_DK;
  const T* ps = REL ? a.pos + h * ATT_DK : nullptr;
  const unsigned char* mr = a.mask ? a.mask + (long)b * a.mb + (long)qi * a.mi : nullptr;

  float4 qf[4], qlo[4], qhi[4];                              // qu row i; qv rows i (lower part of the shift) and i + 1 (upper part)
  frag_global(a.qu + ((long)b * T1 + qi) * a.ldq + h * ATT_DK, fq, qf);
  if (REL) {
    frag_global(a.qv + ((long)b * T1 + qi) * a.ldqv + h * ATT_DK, fq, qlo);
    frag_global(a.qv + ((long)b * T1 + min(i + 1, T1 - 1)) * a.ldqv + h * ATT_DK, fq, qhi);
  }

  // ---- register stage: one key tile's K, V, band and mask words on their way to LDS ----
  float4 kr[STR_KQ], vr[STR_KQ], pr[REL ? SBQ : 1];
  unsigned mkn[STR_NKT];
  auto request = [&](int jt) {
    const int j0 = jt * STR_KT;
#pragma unroll
    for (int q = 0; q < STR_KQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      const long key = min(j0 + row, T2 - 1);
      kr[q] = ld4(ks + key * a.ldk + 4 * c4);
      vr[q] = ld4(vs + key * a.ldv + 4 * c4);
      if (j0 + row >= T2) vr[q] = make_float4(0.f, 0.f, 0.f, 0.f);     // a zero probability times a stale value may not be NaN
    }
    if (REL) {
      const int c0 = Ts + j0 - r0w - (STR_QB - 1);
#pragma unroll
      for (int q = 0; q < SBQ; ++q) {
        const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
        pr[q] = ld4(ps + (long)band_pos_row(c0 + row, Ts) * a.ldpos + 4 * c4);
      }
    }
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) mkn[kt] = mr ? attn_mask4(mr, j0 + 16 * kt + 4 * fq, T2) : 0x01010101u;
  };

  const AttnDrop drop = DROP ? attn_drop_setup(a.drop_p, a.drop_step, a.drop_salt) : AttnDrop{};
  const long pro = ((long)z * T1 + qi) * a.ldp;              // DROP: where this query's row of P would start
  float mrun = -INFINITY, lrun = 0.f;                        // running maximum of query fr; this lane's share of its denominator
  f32x4 C[4];                                                // C[dt][r]: channel 16 dt + 4 fq + r of query fr
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) C[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  request(0);
  for (int jt = 0; jt < ntile; ++jt) {
    const int j0 = jt * STR_KT;
    __syncthreads();                                         // the previous tile's reads are done
#pragma unroll
    for (int q = 0; q < STR_KQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      *reinterpret_cast<float4*>(&Ks[row * STR_PLD + 4 * c4]) = kr[q];
      *reinterpret_cast<float4*>(&Vs[row * STR_PLD + 4 * c4]) = vr[q];
    }
    if (REL) {
#pragma unroll
      for (int q = 0; q < SBQ; ++q) {
        const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
        *reinterpret_cast<float4*>(&Ps[row * STR_PLD + 4 * c4]) = pr[q];
      }
    }
    unsigned mk[STR_NKT];
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) mk[kt] = mkn[kt];
    __syncthreads();
    if (jt + 1 < ntile) request(jt + 1);                     // in flight under this tile's products
    if (!active) continue;

    f32x4 S[STR_NKT];                                           // S[kt][r]: key j0 + 16 kt + 4 fq + r, query fr
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) S[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (REL) {
      float* G = Gs + wave * 16 * SGLD;
      const int nw0 = (STR_QB - 16) - 16 * wave;                // this wave's first row of the staged band
      const int cw = Ts + j0 - r0w - (STR_QB - 1) + nw0;        // ... and the flat column it stands for
#pragma unroll
      for (int bt = 0; bt < SNBT; ++bt) {
        const int cb = cw + 16 * bt;
        float4 pf[4];
        frag_lds(&Ps[(nw0 + 16 * bt + fr) * STR_PLD], fq, pf);
        f32x4 g;                                             // g[r] = G[query fr][band row 16 bt + 4 fq + r]
        if (cb + 15 <= Ts) {                                 // wave-uniform: wholly in the lower part (bd row i)
          g = dot64(pf, qlo, (f32x4){0.f, 0.f, 0.f, 0.f});
        } else if (cb > Ts) {                                // wholly in the upper part (bd row i + 1)
          g = dot64(pf, qhi, (f32x4){0.f, 0.f, 0.f, 0.f});
        } else {                                             // the zero column falls inside
          const f32x4 lo = dot64(pf, qlo, (f32x4){0.f, 0.f, 0.f, 0.f}), hi = dot64(pf, qhi, (f32x4){0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int r = 0; r < 4; ++r) g[r] = cb + 4 * fq + r <= Ts ? lo[r] : hi[r];
        }
        *reinterpret_cast<float4*>(&G[fr * SGLD + 16 * bt + 4 * fq]) = f4(g);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int kt = 0; kt < STR_NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int jj = 16 * kt + 4 * fq + r, j = j0 + jj;
          const float x = G[fr * SGLD + jj + 15 - fr];       // the skewed slice: band row (j - j0) + 15 - a of query a = fr
          S[kt][r] = (i < Ts && j < Ts && j != i + 1) ? x : 0.f;
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();                       // the next tile's G stores come after these reads
    }
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) {
      float4 kf[4];
      frag_lds(&Ks[(16 * kt + fr) * STR_PLD], fq, kf);
      S[kt] = dot64(kf, qf, S[kt]);
    }
    // ---- scale, mask, online softmax ----
    float tmax = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        S[kt][r] = attn_score(S[kt][r], a.scale, j0 + 16 * kt + 4 * fq + r, T2, mk[kt], r);
        tmax = fmaxf(tmax, S[kt][r]);
      }
    const float mnew = fmaxf(mrun, attn_max16_32(tmax));
    const float msub = mnew == -INFINITY ? 0.f : mnew;       // nothing live so far: exp(-inf - 0) = 0, never exp(-inf + inf)
    const float alpha = __expf(mrun - msub);                 // 0 while mrun is -inf: the accumulator it scales is still 0
    mrun = mnew;
    float psum = 0.f;
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __expf(S[kt][r] - msub);
        S[kt][r] = e;
        psum += e;
      }
    lrun = lrun * alpha + psum;
    if (DROP) stream_drop_row(drop, pro, j0, fq, a.ldp, S);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) C[dt] *= alpha;
    // ---- C^T[channel][query] += V_tile^T[channel][key] P^T[key][query] ----
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* row = &Vs[(16 * kt + 4 * fq + r) * STR_PLD + fr];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) C[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[dt * 16], S[kt][r], C[dt], 0, 0, 0);
      }
  }
  if (!active || i >= T1) return;
  const float den = attn_sum16_32(lrun);
  const float inv = den > 0.f ? 1.f / den : 0.f;             // every key masked: zeros
  T* crow = a.ctx + ((long)b * T1 + i) * a.ldc + h * ATT_DK;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) st4(crow + dt * 16 + fq * 4, f4(C[dt] * inv));
  if (LSE && (!DROP || lse) && fq == 0) lse[(long)z * T1 + i] = den > 0.f ? mrun + logf(den) : 0.f;
}

// the checks of the stored forward (attn_check_fwd) without P, Pd and the bound on T2
template <typename T>
int stream_check(const AttnArgs<T>& a, int dk) {
  if (const int rc = attn_check_common(a.qu && a.k && a.v && a.ctx, a.B, a.H, a.T1, a.T2, a.drop_p, a.drop_step)) return rc;
  if ((a.pos == nullptr) != (a.qv == nullptr)) return EAMD_EINVAL;
  if (dk != ATT_DK || (a.pos && a.T1 != a.T2)) return EAMD_EUNSUPPORTED;
  if (!stream_in_ok(a.qu, a.ldq) || !stream_in_ok(a.k, a.ldk) || !stream_in_ok(a.v, a.ldv) || !stream_out_ok(a.ctx, a.ldc) ||
      (a.pos && (!stream_in_ok(a.qv, a.ldqv) || !stream_in_ok(a.pos, a.ldpos))))
    return EAMD_EUNSUPPORTED;
  return attn_too_many<T>(a.B, a.H, a.T1) ? EAMD_EUNSUPPORTED : EAMD_OK;
}

template <typename T>
int stream_entry(const void* qu, int64_t ldq, const void* qv, int64_t ldqv, const void* k, int64_t ldk, const void* v, int64_t ldv,
                 const void* pos, int64_t ldpos, const unsigned char* mask, int64_t mb, int64_t mi, void* ctx, int64_t ldc, int B,
                 int H, int T1, int T2, int dk, float scale, const int32_t* shift_len, void* stream, float* lse = nullptr,
                 bool want_lse = false, float drop_p = 0.f, const uint64_t* drop_step = nullptr, uint64_t drop_salt = 0) {
  if (want_lse && !lse) return EAMD_EINVAL;
  AttnArgs<T> a = attn_args<T>(qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mb, mi, nullptr, stream_ldp(T2), ctx, ldc, B, H, T1,
                               T2, scale, nullptr, drop_p, drop_step, drop_salt, shift_len);
  if (const int rc = stream_check(a, dk)) return rc;
  a.nqb = (T1 + STR_QB - 1) / STR_QB;
  const unsigned grid = attn_grid(a.nqb, B, H);
  hipStream_t s = (hipStream_t)stream;
  if (drop_p > 0.f && pos) hipLaunchKernelGGL((attn_stream_kernel<T, true, true, true>), dim3(grid), dim3(STR_NT), 0, s, a, lse);
  else if (drop_p > 0.f) hipLaunchKernelGGL((attn_stream_kernel<T, false, true, true>), dim3(grid), dim3(STR_NT), 0, s, a, lse);
  else if (want_lse && pos) hipLaunchKernelGGL((attn_stream_kernel<T, true, true>), dim3(grid), dim3(STR_NT), 0, s, a, lse);
  else if (want_lse) hipLaunchKernelGGL((attn_stream_kernel<T, false, true>), dim3(grid), dim3(STR_NT), 0, s, a, lse);
  else if (pos) hipLaunchKernelGGL((attn_stream_kernel<T, true, false>), dim3(grid), dim3(STR_NT), 0, s, a, nullptr);
  else hipLaunchKernelGGL((attn_stream_kernel<T, false, false>), dim3(grid), dim3(STR_NT), 0, s, a, nullptr);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // namespace

extern "C" int eamd_attn_stream_qb(void) { return STR_QB; }
extern "C" int eamd_attn_stream_kt(void) { return STR_KT; }

extern "C" int eamd_attn_fwd_stream_f32(const float* qu, int64_t ldq, const float* qv, int64_t ldqv, const float* k, int64_t ldk,
                                        const float* v, int64_t ldv, const float* pos, int64_t ldpos, const unsigned char* mask,
                                        int64_t mask_bstride, int64_t mask_qstride, float* ctx, int64_t ldc, int B, int H, int T1,
                                        int T2, int dk, float scale, const int32_t* shift_len, void* stream) {
  return stream_entry<float>(qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mask_bstride, mask_qstride, ctx, ldc, B, H, T1, T2,
                             dk, scale, shift_len, stream);
}

extern "C" int eamd_attn_fwd_stream(const void* qu, int64_t ldq, const void* qv, int64_t ldqv, const void* k, int64_t ldk,
                                    const void* v, int64_t ldv, const void* pos, int64_t ldpos, const unsigned char* mask,
                                    int64_t mask_bstride, int64_t mask_qstride, void* ctx_bf16, int64_t ldc, int B, int H, int T1,
                                    int T2, int dk, float scale, const int32_t* shift_len, void* stream) {
  return stream_entry<bf16_t>(qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mask_bstride, mask_qstride, ctx_bf16, ldc, B, H, T1,
                              T2, dk, scale, shift_len, stream);
}

// the same launches with the row statistic lse [H*B][T1] (fp32, z = h * B + b) written beside ctx: what the streamed backward
// (attn_stream_bwd.hip) keeps instead of the probabilities.  ctx has the bits of the entry points above.
extern "C" int eamd_attn_fwd_stream_lse_f32(const float* qu, int64_t ldq, const float* qv, int64_t ldqv, const float* k, int64_t ldk,
                                            const float* v, int64_t ldv, const float* pos, int64_t ldpos, const unsigned char* mask,
                                            int64_t mask_bstride, int64_t mask_qstride, float* ctx, int64_t ldc, int B, int H, int T1,
                                            int T2, int dk, float scale, const int32_t* shift_len, float* lse, void* stream) {
  return stream_entry<float>(qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mask_bstride, mask_qstride, ctx, ldc, B, H, T1, T2,
                             dk, scale, shift_len, stream, lse, true);
}

extern "C" int eamd_attn_fwd_stream_lse(const void* qu, int64_t ldq, const void* qv, int64_t ldqv, const void* k, int64_t ldk,
                                        const void* v, int64_t ldv, const void* pos, int64_t ldpos, const unsigned char* mask,
                                        int64_t mask_bstride, int64_t mask_qstride, void* ctx_bf16, int64_t ldc, int B, int H, int T1,
                                        int T2, int dk, float scale, const int32_t* shift_len, float* lse, void* stream) {
  return stream_entry<bf16_t>(qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mask_bstride, mask_qstride, ctx_bf16, ldc, B, H, T1,
                              T2, dk, scale, shift_len, stream, lse, true);
}

// the same with attention dropout (attention.py:91): ctx = dropout(P) v under the keep bits the stored route draws at
// (drop_step, drop_salt) - see attn_stream_common.h; lse (NULL: not wanted) stays the statistic of the undropped scores.
// drop_p == 0 launches the kernels of the entry points above: their bits
extern "C" int eamd_attn_fwd_stream_drop_f32(const float* qu, int64_t ldq, const float* qv, int64_t ldqv, const float* k, int64_t ldk,
                                             const float* v, int64_t ldv, const float* pos, int64_t ldpos, const unsigned char* mask,
                                             int64_t mask_bstride, int64_t mask_qstride, float* ctx, int64_t ldc, int B, int H, int T1,
                                             int T2, int dk, float scale, const int32_t* shift_len, float* lse, float drop_p,
                                             const uint64_t* drop_step, uint64_t drop_salt, void* stream) {
  return stream_entry<float>(qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mask_bstride, mask_qstride, ctx, ldc, B, H, T1, T2,
                             dk, scale, shift_len, stream, lse, lse != nullptr, drop_p, drop_step, drop_salt);
}

extern "C" int eamd_attn_fwd_stream_drop(const void* qu, int64_t ldq, const void* qv, int64_t ldqv, const void* k, int64_t ldk,
                                         const void* v, int64_t ldv, const void* pos, int64_t ldpos, const unsigned char* mask,
                                         int64_t mask_bstride, int64_t mask_qstride, void* ctx_bf16, int64_t ldc, int B, int H, int T1,
                                         int T2, int dk, float scale, const int32_t* shift_len, float* lse, float drop_p,
                                         const uint64_t* drop_step, uint64_t drop_salt, void* stream) {
  return stream_entry<bf16_t>(qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mask_bstride, mask_qstride, ctx_bf16, ldc, B, H, T1,
                              T2, dk, scale, shift_len, stream, lse, lse != nullptr, drop_p, drop_step, drop_salt);
}
