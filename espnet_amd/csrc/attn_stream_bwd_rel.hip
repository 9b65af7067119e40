// Memory-linear attention backward for training WITH the legacy relative positions, d_k = 64, T1 == T2 = T, any T, fp32 or bf16
// storage, on the fp32 matrix cores (v_mfma_f32_16x16x4_f32).  The forward (attn_stream_kernel<T, true, true>) kept ctx and the row
// statistic lse_i of the scaled, masked scores s_ij = scale (qu_i . k_j + bd_ij); the kernels here rebuild P_ij = exp(s_ij - lse_i)
// tile by tile, position term included, so no [T, T] and no [T, band]-per-row matrix exists in either direction.  No atomics: every
// output element has one owner that sums in a fixed order - the same bits on every launch.
//   bd_ij = qv_i . pos[Ts-1-i+j] (j <= i),  0 (j == i + 1),  qv_{i+1} . pos[j-i-2] (j >= i + 2);  0 unless i < Ts and j < Ts
//   dS = scale P (dctx v^T - delta),  delta_i = dctx_i . ctx_i,  g = dS where the position term applies, 0 elsewhere
//   dqu = dS k,  dk = dS^T qu,  dv = P^T dctx,
//   dqv_i = sum_{j <= i} g_ij pos[Ts-1-i+j] + sum_{j >= i+1} g_{i-1,j} pos[j-i-1],
//   dpos[n] += sum_b ( sum_i g_{i,i-(Ts-1-n)} qv_i + sum_i g_{i,i+n+2} qv_{i+1} ).
// reference: autograd of transformer/attention.py:63-114 (forward_attention), :141-206 (rel_shift).
// Everything is phrased in the flat column c = Ts + j - i of the rows [0 | bd] the legacy shift reads (attn_stream.hip): c <= Ts is
// the lower part (bd row i, pos row c - 1), c == Ts + 1 the zero column, c >= Ts + 2 the upper part (bd row i + 1, pos row c - Ts - 2).
//
// Query side (rel_bwd_q_kernel).  One workgroup = one (batch, head) pair x 64 queries, wave w owns 16 of them and sweeps key tiles of
// 32; K, V and the forward's band of KT + 63 pos rows are register-staged into LDS exactly as in the forward.  Per tile: the
// position term by the forward's gather (band products against qv rows i / i + 1 into a per-wave tile G[16][KT + 16], skewed
// read), + K_tile qu^T, scale, mask, - lse -> P; dS^T[key][query] in registers; dqu^T += K_tile^T dS^T.  Then g goes back into the
// same G tile by the inverse of the forward's read (scalar stores at G[a][jj + 15 - a]) and is read back as float4 - four adjacent
// band rows of query fr, the B operand of dqv_lo^T += Pband^T g_lo^T (c <= Ts, row i) and dqv_hi^T += Pband^T g_hi^T (c >= Ts + 2,
// row i + 1); the one column tile with the zero column feeds both, selected per element.  dqv_lo is written to dqv row i, dqv_hi to
// an fp32 workspace row i, and rel_bwd_dqv_shift_kernel adds workspace row i - 1 into dqv row i.  The kernel also writes delta:
// fp32 storage from dctx . ctx; bf16 storage from a launch of its own in front (rel_bwd_q_kernel<E, true>: the same sweep up to P
// and dP, delta_i = sum_j P_ij dP_ij in fp32), because the half-ulp of a bf16 ctx in delta does not cancel along a row the way dS
// does - measured on a 2-layer Conformer, the bias gradients (column sums of dqu, dqv) moved 1.1 - 1.6e-2 with it, 4 - 6e-3 without.
//   LDS 55.5 KB (56 832 B), 246 VGPRs (bf16: 252; its delta launch 200), no spills: two workgroups (eight waves, two per SIMD) per CU.
// Key side (rel_bwd_kv_kernel).  One workgroup = one pair x 64 keys, wave w owns 16 and keeps their K / V fragments in registers;
// the workgroup sweeps query tiles of 32: qu, dctx, the qv rows of the tile plus the one after it, lse / delta, and the ONE
// contiguous band of 64 + 32 - 1 pos rows the (key block, query tile) pair touches (row n = flat column Ts + jb - i0 - 31 + n, clamped
// as in the forward).  Per 16-query piece a wave multiplies two band tiles against the qv rows, writes G[query][band row] and reads
// G[a][key + 15 - a] back; the rest is the backward without positions: dv^T += dCtx^T P, dk^T += Q^T dS.
//   LDS 60.5 KB (61 968 B, static), 248 VGPRs (bf16: 246), no spills: two workgroups per CU.
// Position side (rel_bwd_dpos_kernel).  One workgroup = one pair x 64 flat columns c (diagonals j - i = c - Ts), wave w keeps the pos
// rows of its 16 columns in registers and sweeps query tiles of 16 (only those whose diagonal lies inside the Ts x Ts square).  The
// keys of a (tile, column block) are ONE band of 64 + 16 - 1 rows; K and V bands, qu, dctx and 17 qv rows are staged.  qu . k and
// dctx . v on a wave's 31 band keys go through the matrix cores into two per-wave tiles and come back skewed, G[a][a + column], in
// (query, column) layout; qv_i . pos (lower) or qv_{i+1} . pos (upper) is a plain tile; g is formed per element (mask byte read per
// element) and dflat^T[channel][c] += QV_tile^T g.  Each workgroup owns its 64 rows of the fp32 workspace [B][2 T][H * 64];
// rel_bwd_dpos_sum_kernel adds sum_b (dflat[b][n + 1] + dflat[b][n + Ts + 2]) in ascending b INTO dpos row n.
//   LDS 73.6 KB (75 408 B, dynamic), 178 VGPRs (bf16: 182), no spills: two workgroups per CU (32-query tiles would need 88 KB: one).
// (figures of the gfx950 cross-compile, .vgpr_count / .group_segment_fixed_size; at eight waves per CU a wave may hold 256 VGPRs)
// Hazards:
//   * keys / queries >= T: masked by index (attn_score, or the selection on the index), never by a clamped re-read's value; V and
//     qu / dctx rows past T are staged as zeros where a zero probability meets them;
//   * rows >= Ts take no position term and give no position gradient: the guard i < Ts && j < Ts && j != i + 1 sits on every read
//     of the skewed tiles and on g; band rows outside the matrix are clamped re-reads (finite) that only ever meet g = 0;
//   * a dead row (every key masked) has lse = 0 and P = 0: dS = 0 exactly, so dqu = dqv = 0 and nothing is added elsewhere;
//   * qv row i + 1 is clamped at T - 1 but used only where j >= i + 2 and j < Ts, i.e. i + 1 < Ts;
//   * T = 1 (one column, c = 1) and T = 2 (no upper part: the first upper column is Ts + 2 = 4 > 2 Ts - 1);
//   * G elements a wave's skewed stores do not reach still hold the forward's products: the float4 read selects them to zero by
//     index (band row n of query a is written iff 15 - a <= n < KT + 15 - a).
#include "attn_stream_common.h"

namespace {

template <typename E>
struct RelBwdArgs {
  const E* dctx; const E* ctx; const E* qu; const E* qv; const E* k; const E* v; const E* pos;
  const unsigned char* mask;
  const float* lse; const int* tshift;
  float* delta; float* hi; float* dflat;                     // workspaces: [H*B][T], [B*T][H*64], [B][2T][H*64]
  float* dqu; float* dqv; E* dk; E* dv; float* dpos;
  long ldd, ldc, ldq, ldqv, ldk, ldv, ldpos, mb, mi, lddqu, lddqv, lddk, lddv, lddpos;
  int B, H, T, nqb, ndb;
  float scale;
  // the forward's attention dropout (DROP kernels): the keep bits of P's stored layout [H*B][T][ldp], attn_stream_common.h
  float drop_p; const unsigned long long* drop_step; unsigned long long drop_salt; long ldp;
};

constexpr int RQ_BR = STR_KT + STR_QB;           // query side: band rows staged (KT + QB - 1 are used)
constexpr int RQ_NBT = STR_NKT + 1;              // 16-row column tiles of a wave's band
constexpr int RQ_GLD = 16 * RQ_NBT + 4;          // row stride of a wave's band tile G[16][KT + 16]
constexpr int RQ_BQ = RQ_BR * 16 / STR_NT;       // 16-byte pieces per thread of the band
constexpr int KV_BR = STR_QB + STR_KT;           // key side: band rows staged (QB + KT - 1 are used)
constexpr int KV_QVR = STR_KT + 1;               // qv rows staged: the tile and the row after it
constexpr int KV_QVQ = (KV_QVR * 16 + STR_NT - 1) / STR_NT;
constexpr int KV_BQ = KV_BR * 16 / STR_NT;
constexpr int KV_GLD = 36;                       // row stride of a wave's tile G[16][32]
constexpr int DP_QT = 16;                        // position side: queries per staged tile
constexpr int DP_BR = STR_QB + DP_QT;            // band keys staged (QB + QT - 1 are used)
constexpr int DP_BQ = DP_BR * 16 / STR_NT;
constexpr int DP_GLD = 36;
constexpr int DP_LDS = (2 * DP_BR * STR_PLD + 2 * DP_QT * STR_PLD + (DP_QT + 1) * STR_PLD + 2 * STR_NW * 16 * DP_GLD + 2 * DP_QT) *
                       (int)sizeof(float);

// acc^T[channel 16 dt + 4 fq + r][column fr] += sum over 16 rows of X[row][channel] w[row 4 fq + r][column fr]
__device__ __forceinline__ void baccum16(const float* X, int fr, int fq, const f32x4& w, f32x4 (&acc)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float* row = &X[(4 * fq + r) * STR_PLD + fr];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[dt * 16], w[r], acc[dt], 0, 0, 0);
  }
}

// a wave's LDS tile changes hands between its lanes: stores before, loads after
__device__ __forceinline__ void wave_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// band rows x (against qv rows i: lo, i + 1: hi) for the 16 flat columns cb .. cb + 15: g[r] = column cb + 4 fq + r of query fr
__device__ __forceinline__ f32x4 band_product(const float4 (&pf)[4], const float4 (&qlo)[4], const float4 (&qhi)[4], int cb, int fq,
                                              int Ts) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (cb + 15 <= Ts) return dot64(pf, qlo, zero);            // wave-uniform: wholly in the lower part
  if (cb > Ts) return dot64(pf, qhi, zero);                  // wholly in the upper part
  const f32x4 lo = dot64(pf, qlo, zero), hi = dot64(pf, qhi, zero);      // the zero column falls inside
  f32x4 g;
#pragma unroll
  for (int r = 0; r < 4; ++r) g[r] = cb + 4 * fq + r <= Ts ? lo[r] : hi[r];
  return g;
}

// DROP (query, key and position side): the forward built ctx from Pd = P o M / (1 - p), so dP <- M / (1 - p) o (dctx v^T) wherever
// dS is formed - g and the position side's dbd are that dS -, dv takes Pd, and the DELTA sweep sums P (M / (1 - p) o dP) =
// Pd dPd.  M is regenerated per tile from the element indices a lane holds (stream_drop_row / stream_keep_col)
template <typename E, bool DELTA, bool DROP>
__global__ __launch_bounds__(STR_NT, 2) void rel_bwd_q_kernel(const RelBwdArgs<E> a) {
  __shared__ __attribute__((aligned(16))) float Ks[STR_KT * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Vs[STR_KT * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Ps[RQ_BR * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Gs[STR_NW * 16 * RQ_GLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int z = attn_xcd_pair(blockIdx.x, a.nqb);            // z = h * B + b
  if (z >= a.B * a.H) return;                                // whole workgroup
  const int h = z / a.B, b = z % a.B;
  const int T = a.T;
  const int r0w = attn_xcd_block(blockIdx.x, a.nqb) * STR_QB;
  const int i0 = r0w + 16 * wave;
  const bool active = i0 < T;                                // wave-uniform; idle waves still stage and keep the barriers
  const int i = i0 + fr;                                     // this lane's query (rows past T: clamped re-reads, never stored)
  const int qi = min(i, T - 1);
  const int Ts = attn_shift_len(a.tshift, T);
  const int ntile = (T + STR_KT - 1) / STR_KT;
  const E* ks = a.k + (long)b * T * a.ldk + h * ATT_DK;
  const E* vs = a.v + (long)b * T * a.ldv + h * ATT_DK;
  const E* ps = a.pos + h * ATT_DK;
  const unsigned char* mr = a.mask ? a.mask + (long)b * a.mb + (long)qi * a.mi : nullptr;

  float4 qf[4], df[4], qlo[4], qhi[4];                       // qu, dctx of row i; qv rows i and i + 1
  frag_global(a.qu + ((long)b * T + qi) * a.ldq + h * ATT_DK, fq, qf);
  frag_global(a.dctx + ((long)b * T + qi) * a.ldd + h * ATT_DK, fq, df);
  frag_global(a.qv + ((long)b * T + qi) * a.ldqv + h * ATT_DK, fq, qlo);
  frag_global(a.qv + ((long)b * T + min(i + 1, T - 1)) * a.ldqv + h * ATT_DK, fq, qhi);
  const float lse = a.lse[(long)z * T + qi];
  // delta_i: from the forward's ctx where that is stored in fp32.  A bf16 ctx carries a half-ulp 2^-9 |ctx| into dctx . ctx, the
  // same for every key of the row, and the gradients whose terms cancel along a row (sum_j dS_ij = 0: the column sums behind
  // the Conformer's position and query biases) keep it; bf16 storage therefore takes delta = sum_j P_ij dP_ij from a first
  // launch of this kernel (DELTA: the sweep up to P and dP, nothing else), in fp32, and the gradient launch reads it back
  constexpr bool PRE = sizeof(E) == 2;
  float delta = 0.f, dsum = 0.f;                             // dsum (DELTA): this lane's share of sum_j P_ij dP_ij
  if (PRE) {
    if (!DELTA) delta = a.delta[(long)z * T + qi];
  } else {
    float4 cf[4];
    frag_global(a.ctx + ((long)b * T + qi) * a.ldc + h * ATT_DK, fq, cf);
#pragma unroll
    for (int j = 0; j < 4; ++j) delta += df[j].x * cf[j].x + df[j].y * cf[j].y + df[j].z * cf[j].z + df[j].w * cf[j].w;
    delta = attn_sum16_32(delta);
    if (active && fq == 0 && i < T) a.delta[(long)z * T + i] = delta;
  }

  float4 kr[STR_KQ], vr[STR_KQ], pr[RQ_BQ];                  // register stage: one key tile's K, V and band on their way to LDS
  unsigned mkn[STR_NKT];
  auto request = [&](int jt) {
    const int j0 = jt * STR_KT;
#pragma unroll
    for (int q = 0; q < STR_KQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      const long key = min(j0 + row, T - 1);
      kr[q] = ld4(ks + key * a.ldk + 4 * c4);
      vr[q] = ld4(vs + key * a.ldv + 4 * c4);
      if (j0 + row >= T) vr[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int c0 = Ts + j0 - r0w - (STR_QB - 1);
#pragma unroll
    for (int q = 0; q < RQ_BQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      pr[q] = ld4(ps + (long)band_pos_row(c0 + row, Ts) * a.ldpos + 4 * c4);
    }
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) mkn[kt] = mr ? attn_mask4(mr, j0 + 16 * kt + 4 * fq, T) : 0x01010101u;
  };

  f32x4 DQ[4], DLO[4], DHI[4];                               // [dt][r]: channel 16 dt + 4 fq + r of query fr
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) DQ[dt] = DLO[dt] = DHI[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float* G = Gs + wave * 16 * RQ_GLD;
  const int nw0 = (STR_QB - 16) - 16 * wave;                 // this wave's first row of the staged band
  const AttnDrop drop = DROP ? attn_drop_setup(a.drop_p, a.drop_step, a.drop_salt) : AttnDrop{};

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
#pragma unroll
    for (int q = 0; q < RQ_BQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      *reinterpret_cast<float4*>(&Ps[row * STR_PLD + 4 * c4]) = pr[q];
    }
    unsigned mk[STR_NKT];
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) mk[kt] = mkn[kt];
    __syncthreads();
    if (jt + 1 < ntile) request(jt + 1);                     // in flight under this tile's products
    if (!active) continue;

    // ---- the position term, by the forward's gather ----
    const int cw = Ts + j0 - r0w - (STR_QB - 1) + nw0;       // the flat column of the wave's first band row
#pragma unroll
    for (int bt = 0; bt < RQ_NBT; ++bt) {
      float4 pf[4];
      frag_lds(&Ps[(nw0 + 16 * bt + fr) * STR_PLD], fq, pf);
      *reinterpret_cast<float4*>(&G[fr * RQ_GLD + 16 * bt + 4 * fq]) = f4(band_product(pf, qlo, qhi, cw + 16 * bt, fq, Ts));
    }
    wave_handover();
    f32x4 S[STR_NKT], dP[STR_NKT];                           // [kt][r]: key j0 + 16 kt + 4 fq + r, query fr
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jj = 16 * kt + 4 * fq + r, j = j0 + jj;
        const float x = G[fr * RQ_GLD + jj + 15 - fr];
        S[kt][r] = (i < Ts && j < Ts && j != i + 1) ? x : 0.f;
      }
    wave_handover();                                         // g's skewed stores come after these reads
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) {
      float4 xf[4];
      frag_lds(&Ks[(16 * kt + fr) * STR_PLD], fq, xf);
      S[kt] = dot64(xf, qf, S[kt]);
      frag_lds(&Vs[(16 * kt + fr) * STR_PLD], fq, xf);
      dP[kt] = dot64(xf, df, (f32x4){0.f, 0.f, 0.f, 0.f});
    }
    if (DROP) stream_drop_row(drop, ((long)z * T + qi) * a.ldp, j0, fq, a.ldp, dP);     // the row offset is re-formed here: registers
    if (DELTA) {
#pragma unroll
      for (int kt = 0; kt < STR_NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          dsum += __expf(attn_score(S[kt][r], a.scale, j0 + 16 * kt + 4 * fq + r, T, mk[kt], r) - lse) * dP[kt][r];
      continue;
    }
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jj = 16 * kt + 4 * fq + r, j = j0 + jj;
        const float p = __expf(attn_score(S[kt][r], a.scale, j, T, mk[kt], r) - lse);
        const float ds = a.scale * p * (dP[kt][r] - delta);  // dS^T[key][query]
        S[kt][r] = ds;
        G[fr * RQ_GLD + jj + 15 - fr] = (i < Ts && j < Ts && j != i + 1) ? ds : 0.f;      // the inverse of the read above
      }
      baccum16(&Ks[16 * kt * STR_PLD], fr, fq, S[kt], DQ);   // dqu^T[channel][query] += K_tile^T[channel][key] dS^T[key][query]
    }
    wave_handover();
    // ---- dqv^T[channel][query] += Pband^T[channel][band row] g^T[band row][query], lower part to row i, upper to row i + 1 ----
#pragma unroll
    for (int bt = 0; bt < RQ_NBT; ++bt) {
      const int cb = cw + 16 * bt;
      const float4 g4 = *reinterpret_cast<const float4*>(&G[fr * RQ_GLD + 16 * bt + 4 * fq]);
      f32x4 g = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = 16 * bt + 4 * fq + r;
        if (n < 15 - fr || n >= STR_KT + 15 - fr) g[r] = 0.f;            // not reached by the skewed stores: still the forward's product
      }
      const float* X = &Ps[(nw0 + 16 * bt) * STR_PLD];
      if (cb + 15 <= Ts) {
        baccum16(X, fr, fq, g, DLO);
      } else if (cb > Ts) {
        baccum16(X, fr, fq, g, DHI);
      } else {
        f32x4 glo, ghi;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool low = cb + 4 * fq + r <= Ts;
          glo[r] = low ? g[r] : 0.f;
          ghi[r] = low ? 0.f : g[r];
        }
        baccum16(X, fr, fq, glo, DLO);
        baccum16(X, fr, fq, ghi, DHI);
      }
    }
    wave_handover();                                         // the next tile's G stores come after these reads
  }
  if (DELTA) {
    dsum = attn_sum16_32(dsum);
    if (active && fq == 0 && i < T) a.delta[(long)z * T + i] = dsum;
    return;
  }
  if (!active || i >= T) return;
  const long row = (long)b * T + i;
  float* urow = a.dqu + row * a.lddqu + h * ATT_DK;
  float* vrow = a.dqv + row * a.lddqv + h * ATT_DK;
  float* hrow = a.hi + row * ((long)a.H * ATT_DK) + h * ATT_DK;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    st4(urow + dt * 16 + fq * 4, f4(DQ[dt]));
    st4(vrow + dt * 16 + fq * 4, f4(DLO[dt]));
    st4(hrow + dt * 16 + fq * 4, f4(DHI[dt]));
  }
}

// dqv row i += the upper-part sums of row i - 1 (the query side's workspace): one owner per element
template <typename E>
__global__ __launch_bounds__(256) void rel_bwd_dqv_shift_kernel(const RelBwdArgs<E> a) {
  const int D4 = a.H * ATT_DK / 4;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.B * a.T * D4) return;
  const long row = idx / D4;
  const int c4 = (int)(idx % D4);
  if (row % a.T == 0) return;                                // a batch's first row has no row above it
  float4* d = reinterpret_cast<float4*>(a.dqv + row * a.lddqv + 4 * c4);
  const float4 x = *reinterpret_cast<const float4*>(a.hi + (row - 1) * (4L * D4) + 4 * c4);
  float4 y = *d;
  y.x += x.x; y.y += x.y; y.z += x.z; y.w += x.w;
  *d = y;
}

template <typename E, bool DROP>
__global__ __launch_bounds__(STR_NT, 2) void rel_bwd_kv_kernel(const RelBwdArgs<E> a) {
  __shared__ __attribute__((aligned(16))) float Qs[STR_KT * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Ds[STR_KT * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Vq[KV_QVR * STR_PLD];                         // qv rows i0 .. i0 + KT
  __shared__ __attribute__((aligned(16))) float Pb[KV_BR * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Gs[STR_NW * 16 * KV_GLD];
  __shared__ __attribute__((aligned(16))) float Ls[STR_KT], Es[STR_KT];                       // lse and delta of the staged queries
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int z = attn_xcd_pair(blockIdx.x, a.nqb);
  if (z >= a.B * a.H) return;                                // whole workgroup
  const int h = z / a.B, b = z % a.B;
  const int T = a.T;
  const int jb = attn_xcd_block(blockIdx.x, a.nqb) * STR_QB;
  const int j0w = jb + 16 * wave;
  const bool active = j0w < T;                               // wave-uniform
  const int j = j0w + fr;                                    // this lane's key (past T: a clamped re-read, masked by index, never stored)
  const int kj = min(j, T - 1);
  const int Ts = attn_shift_len(a.tshift, T);
  const int ntile = (T + STR_KT - 1) / STR_KT;
  const E* qs = a.qu + (long)b * T * a.ldq + h * ATT_DK;
  const E* ws = a.qv + (long)b * T * a.ldqv + h * ATT_DK;
  const E* ds = a.dctx + (long)b * T * a.ldd + h * ATT_DK;
  const E* ps = a.pos + h * ATT_DK;
  const float* ls = a.lse + (long)z * T;
  const float* es = a.delta + (long)z * T;
  const unsigned char* mc = a.mask ? a.mask + (long)b * a.mb + kj : nullptr;     // this key's column of the pair's mask rows

  float4 kf[4], vf[4];
  frag_global(a.k + ((long)b * T + kj) * a.ldk + h * ATT_DK, fq, kf);
  frag_global(a.v + ((long)b * T + kj) * a.ldv + h * ATT_DK, fq, vf);

  float4 qr[STR_KQ], dr[STR_KQ], wr[KV_QVQ], pr[KV_BQ];      // register stage: one query tile on its way to LDS
  float sr = 0.f;                                            // threads 0 .. 31: lse, 32 .. 63: delta of tile row t & 31
  unsigned mkn[STR_NKT];
  auto request = [&](int it) {
    const int i0 = it * STR_KT;
#pragma unroll
    for (int q = 0; q < STR_KQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      const long qrow = min(i0 + row, T - 1);
      qr[q] = ld4(qs + qrow * a.ldq + 4 * c4);
      dr[q] = ld4(ds + qrow * a.ldd + 4 * c4);
      if (i0 + row >= T) qr[q] = dr[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int q = 0; q < KV_QVQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      if (row < KV_QVR) wr[q] = ld4(ws + (long)min(i0 + row, T - 1) * a.ldqv + 4 * c4);
    }
    const int c0 = Ts + jb - i0 - (STR_KT - 1);              // the flat column of band row 0
#pragma unroll
    for (int q = 0; q < KV_BQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      pr[q] = ld4(ps + (long)band_pos_row(c0 + row, Ts) * a.ldpos + 4 * c4);
    }
    if (t < 2 * STR_KT) {
      const int row = t & (STR_KT - 1);
      sr = (t < STR_KT ? ls : es)[min(i0 + row, T - 1)];
      if (i0 + row >= T) sr = 0.f;
    }
#pragma unroll
    for (int qt = 0; qt < STR_NKT; ++qt) {
      unsigned w = 0x01010101u;
      if (mc) {
        w = 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) w |= (unsigned)mc[(long)min(i0 + 16 * qt + 4 * fq + r, T - 1) * a.mi] << (8 * r);
      }
      mkn[qt] = w;
    }
  };

  f32x4 DV[4], DK[4];                                        // [dt][r]: channel 16 dt + 4 fq + r of key fr
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) DV[dt] = DK[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float* G = Gs + wave * 16 * KV_GLD;
  const AttnDrop drop = DROP ? attn_drop_setup(a.drop_p, a.drop_step, a.drop_salt) : AttnDrop{};

  request(0);
  for (int it = 0; it < ntile; ++it) {
    const int i0 = it * STR_KT;
    __syncthreads();                                         // the previous tile's reads are done
#pragma unroll
    for (int q = 0; q < STR_KQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      *reinterpret_cast<float4*>(&Qs[row * STR_PLD + 4 * c4]) = qr[q];
      *reinterpret_cast<float4*>(&Ds[row * STR_PLD + 4 * c4]) = dr[q];
    }
#pragma unroll
    for (int q = 0; q < KV_QVQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      if (row < KV_QVR) *reinterpret_cast<float4*>(&Vq[row * STR_PLD + 4 * c4]) = wr[q];
    }
#pragma unroll
    for (int q = 0; q < KV_BQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      *reinterpret_cast<float4*>(&Pb[row * STR_PLD + 4 * c4]) = pr[q];
    }
    if (t < STR_KT) Ls[t] = sr;
    else if (t < 2 * STR_KT) Es[t - STR_KT] = sr;
    unsigned mk[STR_NKT];
#pragma unroll
    for (int qt = 0; qt < STR_NKT; ++qt) mk[qt] = mkn[qt];
    __syncthreads();
    if (it + 1 < ntile) request(it + 1);                     // in flight under this tile's products
    if (!active) continue;

    f32x4 P[STR_NKT], dS[STR_NKT];                           // [qt][r]: query i0 + 16 qt + 4 fq + r, key fr
    // ---- the position term of (16 queries x 16 keys): flat columns cq .. cq + 30, band rows nb0 .. nb0 + 30 ----
#pragma unroll
    for (int qt = 0; qt < STR_NKT; ++qt) {
      const int nb0 = 16 * (wave - qt + 1);
      const int cq = Ts + jb - i0 - (STR_KT - 1) + nb0;
      float4 qlo[4], qhi[4];
      frag_lds(&Vq[(16 * qt + fr) * STR_PLD], fq, qlo);
      frag_lds(&Vq[(16 * qt + fr + 1) * STR_PLD], fq, qhi);
#pragma unroll
      for (int bt = 0; bt < 2; ++bt) {
        float4 pf[4];
        frag_lds(&Pb[(nb0 + 16 * bt + fr) * STR_PLD], fq, pf);
        *reinterpret_cast<float4*>(&G[fr * KV_GLD + 16 * bt + 4 * fq]) = f4(band_product(pf, qlo, qhi, cq + 16 * bt, fq, Ts));
      }
      wave_handover();
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int aq = 4 * fq + r, ii = i0 + 16 * qt + aq;
        const float x = G[aq * KV_GLD + fr + 15 - aq];       // the skewed slice: band row (key - query) + 15 of the piece
        P[qt][r] = (ii < Ts && j < Ts && j != ii + 1) ? x : 0.f;
      }
      wave_handover();                                       // the next piece's G stores come after these reads
    }
#pragma unroll
    for (int qt = 0; qt < STR_NKT; ++qt) {
      float4 xf[4];
      frag_lds(&Qs[(16 * qt + fr) * STR_PLD], fq, xf);
      P[qt] = dot64(xf, kf, P[qt]);
      frag_lds(&Ds[(16 * qt + fr) * STR_PLD], fq, xf);
      dS[qt] = dot64(xf, vf, (f32x4){0.f, 0.f, 0.f, 0.f});
    }
#pragma unroll
    for (int qt = 0; qt < STR_NKT; ++qt) {
      const float4 l4 = *reinterpret_cast<const float4*>(&Ls[16 * qt + 4 * fq]);
      const float4 e4 = *reinterpret_cast<const float4*>(&Es[16 * qt + 4 * fq]);
      const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, eq[4] = {e4.x, e4.y, e4.z, e4.w};
      float m[4];
      if (DROP) stream_keep_col(drop, ((long)z * T + i0 + 16 * qt + 4 * fq) * a.ldp + j, a.ldp, m);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = __expf(attn_score(P[qt][r], a.scale, j, T, mk[qt], r) - lq[r]);
        if (i0 + 16 * qt + 4 * fq + r >= T) p = 0.f;         // by index: a clamped row would carry a live lse and delta
        P[qt][r] = DROP ? p * m[r] : p;                      // Pd for dv
        dS[qt][r] = a.scale * p * ((DROP ? dS[qt][r] * m[r] : dS[qt][r]) - eq[r]);
      }
      baccum16(&Ds[16 * qt * STR_PLD], fr, fq, P[qt], DV);   // dv^T[channel][key] += dCtx_tile^T[channel][query] P[query][key]
      baccum16(&Qs[16 * qt * STR_PLD], fr, fq, dS[qt], DK);  // dk^T[channel][key] += Q_tile^T[channel][query] dS[query][key]
    }
  }
  if (!active || j >= T) return;
  E* vrow = a.dv + ((long)b * T + j) * a.lddv + h * ATT_DK;
  E* krow =a.dk + ((long)b * T + j) * a.lddk + h * ATT_DK;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    st4(vrow + dt * 16 + fq * 4, f4(DV[dt]));
    st4(krow + dt * 16 + fq * 4, f4(DK[dt]));
  }
}

template <typename E, bool DROP>
__global__ __launch_bounds__(STR_NT, 2) void rel_bwd_dpos_kernel(const RelBwdArgs<E> a) {
  extern __shared__ __attribute__((aligned(16))) float dp_lds[];
  float* Kb = dp_lds;                                        // K, V rows of the band keys jbase .. jbase + 79
  float* Vb = Kb + DP_BR * STR_PLD;
  float* Qs = Vb + DP_BR * STR_PLD;                          // qu, dctx rows i0 .. i0 + 15
  float* Ds = Qs + DP_QT * STR_PLD;
  float* Vq = Ds + DP_QT * STR_PLD;                          // qv rows i0 .. i0 + 16
  float* GSs = Vq + (DP_QT + 1) * STR_PLD;                   // per wave: qu . k and dctx . v as [query][band key]
  float* GPs = GSs + STR_NW * 16 * DP_GLD;
  float* Ls = GPs + STR_NW * 16 * DP_GLD;
  float* Es = Ls + DP_QT;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int z = attn_xcd_pair(blockIdx.x, a.ndb);
  if (z >= a.B * a.H) return;                                // whole workgroup
  const int h = z / a.B, b = z % a.B;
  const int T = a.T;
  const int Ts = attn_shift_len(a.tshift, T);
  const int cb0 = attn_xcd_block(blockIdx.x, a.ndb) * STR_QB;   // the workgroup's first flat column
  if (cb0 > 2 * Ts - 1) return;                              // whole workgroup: beyond the last diagonal, its rows are never read
  const int cw = cb0 + 16 * wave;
  const int c = cw + fr, o = c - Ts;                         // this lane's flat column and its diagonal j - i
  const E* ks = a.k + (long)b * T * a.ldk + h * ATT_DK;
  const E* vs = a.v + (long)b * T * a.ldv + h * ATT_DK;
  const E* qs = a.qu + (long)b * T * a.ldq + h * ATT_DK;
  const E* ws = a.qv + (long)b * T * a.ldqv + h * ATT_DK;
  const E* ds = a.dctx + (long)b * T * a.ldd + h * ATT_DK;
  const float* ls = a.lse + (long)z * T;
  const float* es = a.delta + (long)z * T;
  const unsigned char* mp = a.mask ? a.mask + (long)b * a.mb : nullptr;

  float4 pf[4];                                              // the pos row behind column c (clamped where c is no column of bd)
  frag_global(a.pos + (long)band_pos_row(c, Ts) * a.ldpos + h * ATT_DK, fq, pf);

  // queries whose diagonal element lies in the Ts x Ts square for some column of the block: 0 <= i + c - Ts < Ts, i < Ts
  const int it0 = max(0, Ts - cb0 - (STR_QB - 1)) / DP_QT;
  const int it1 = (min(Ts, 2 * Ts - cb0) + DP_QT - 1) / DP_QT;

  float4 kr[DP_BQ], vr[DP_BQ], qr, dr, wr0, wr1 = make_float4(0.f, 0.f, 0.f, 0.f);
  float sr = 0.f;                                            // threads 0 .. 15: lse, 16 .. 31: delta of tile row t & 15
  unsigned mkn = 0x01010101u;
  auto request = [&](int it) {
    const int i0 = it * DP_QT, jbase = i0 + cb0 - Ts;
#pragma unroll
    for (int q = 0; q < DP_BQ; ++q) {
      const int e = t + STR_NT * q, row = e >> 4, c4 = e & 15;
      const long key = min(max(jbase + row, 0), T - 1);      // outside [0, T): a clamped re-read, selected away by index
      kr[q] = ld4(ks + key * a.ldk + 4 * c4);
      vr[q] = ld4(vs + key * a.ldv + 4 * c4);
    }
    {
      const int row = t >> 4, c4 = t & 15;
      const long qrow = min(i0 + row, T - 1);
      qr = ld4(qs + qrow * a.ldq + 4 * c4);
      dr = ld4(ds + qrow * a.ldd + 4 * c4);
      wr0 = ld4(ws + qrow * a.ldqv + 4 * c4);
      if (t < 16) wr1 = ld4(ws + (long)min(i0 + DP_QT, T - 1) * a.ldqv + 4 * c4);
    }
    if (t < 2 * DP_QT) sr = (t < DP_QT ? ls : es)[min(i0 + (t & (DP_QT - 1)), T - 1)];
    if (mp) {
      mkn = 0u;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = i0 + 4 * fq + r;
        mkn |= (unsigned)mp[(long)min(ii, T - 1) * a.mi + min(max(ii + o, 0), T - 1)] << (8 * r);
      }
    }
  };

  f32x4 DP[4];                                               // [dt][r]: channel 16 dt + 4 fq + r of column c
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) DP[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float* GS = GSs + wave * 16 * DP_GLD;
  float* GP = GPs + wave * 16 * DP_GLD;
  const AttnDrop drop = DROP ? attn_drop_setup(a.drop_p, a.drop_step, a.drop_salt) : AttnDrop{};

  if (it0 < it1) request(it0);
  for (int it = it0; it < it1; ++it) {
    const int i0 = it * DP_QT;
    __syncthreads();                                         // the previous tile's reads are done
#pragma unroll
    for (int q = 0; q < DP_BQ; ++q) {
      const int e = t + STR_NT * q, row = e >> 4, c4 = e & 15;
      *reinterpret_cast<float4*>(&Kb[row * STR_PLD + 4 * c4]) = kr[q];
      *reinterpret_cast<float4*>(&Vb[row * STR_PLD + 4 * c4]) = vr[q];
    }
    {
      const int row = t >> 4, c4 = t & 15;
      *reinterpret_cast<float4*>(&Qs[row * STR_PLD + 4 * c4]) = qr;
      *reinterpret_cast<float4*>(&Ds[row * STR_PLD + 4 * c4]) = dr;
      *reinterpret_cast<float4*>(&Vq[row * STR_PLD + 4 * c4]) = wr0;
      if (t < 16) *reinterpret_cast<float4*>(&Vq[DP_QT * STR_PLD + 4 * c4]) = wr1;
    }
    if (t < DP_QT) Ls[t] = sr;
    else if (t < 2 * DP_QT) Es[t - DP_QT] = sr;
    const unsigned mk = mkn;
    __syncthreads();
    if (it + 1 < it1) request(it + 1);                       // in flight under this tile's products
    if (cw > 2 * Ts - 1) continue;                           // wave-uniform: no diagonal of this wave exists

    // ---- qu . k and dctx . v on the wave's band keys 16 w .. 16 w + 30, as [query fr][band key] ----
    {
      float4 qf[4], df[4];
      frag_lds(&Qs[fr * STR_PLD], fq, qf);
      frag_lds(&Ds[fr * STR_PLD], fq, df);
#pragma unroll
      for (int bt = 0; bt < 2; ++bt) {
        float4 xf[4];
        frag_lds(&Kb[(16 * wave + 16 * bt + fr) * STR_PLD], fq, xf);
        *reinterpret_cast<float4*>(&GS[fr * DP_GLD + 16 * bt + 4 * fq]) = f4(dot64(xf, qf, (f32x4){0.f, 0.f, 0.f, 0.f}));
        frag_lds(&Vb[(16 * wave + 16 * bt + fr) * STR_PLD], fq, xf);
        *reinterpret_cast<float4*>(&GP[fr * DP_GLD + 16 * bt + 4 * fq]) = f4(dot64(xf, df, (f32x4){0.f, 0.f, 0.f, 0.f}));
      }
    }
    // ---- the position term in place: qv rows (i: lower columns, i + 1: upper) against this lane's pos row ----
    f32x4 bd;                                                // [r]: query i0 + 4 fq + r, column c
    {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      float4 xlo[4], xhi[4];
      if (cw + 15 <= Ts) {
        frag_lds(&Vq[fr * STR_PLD], fq, xlo);
        bd = dot64(xlo, pf, zero);
      } else if (cw > Ts) {
        frag_lds(&Vq[(fr + 1) * STR_PLD], fq, xhi);
        bd = dot64(xhi, pf, zero);
      } else {
        frag_lds(&Vq[fr * STR_PLD], fq, xlo);
        frag_lds(&Vq[(fr + 1) * STR_PLD], fq, xhi);
        const f32x4 lo = dot64(xlo, pf, zero), hi = dot64(xhi, pf, zero);
#pragma unroll
        for (int r = 0; r < 4; ++r) bd[r] = c <= Ts ? lo[r] : hi[r];
      }
    }
    wave_handover();
    const float4 l4 = *reinterpret_cast<const float4*>(&Ls[4 * fq]);
    const float4 e4 = *reinterpret_cast<const float4*>(&Es[4 * fq]);
    const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, eq[4] = {e4.x, e4.y, e4.z, e4.w};
    f32x4 g;
    float m[4];                                              // DROP: element (ii, ii + o) of the pair's P, a diagonal: stride ldp + 1
    if (DROP) stream_keep_col(drop, ((long)z * T + i0 + 4 * fq) * a.ldp + i0 + 4 * fq + o, a.ldp + 1, m);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int aq = 4 * fq + r, ii = i0 + aq, jj = ii + o;
      const float s = GS[aq * DP_GLD + aq + fr], dp = GP[aq * DP_GLD + aq + fr];          // band key (query + column) of the wave
      const bool on = ii < Ts && jj >= 0 && jj < Ts && jj != ii + 1 && ((mk >> (8 * r)) & 0xffu) != 0u;   // by index, then the mask byte
      const float p = __expf(a.scale * (s + bd[r]) - lq[r]);
      g[r] = on ? a.scale * p * ((DROP ? dp * m[r] : dp) - eq[r]) : 0.f;
    }
    wave_handover();                                         // the next tile's stores come after these reads
    // ---- dflat^T[channel][c] += QV_tile^T[channel][query] g[query][c] ----
    if (cw + 15 <= Ts) {
      baccum16(Vq, fr, fq, g, DP);
    } else if (cw > Ts) {
      baccum16(Vq + STR_PLD, fr, fq, g, DP);
    } else {
      f32x4 glo, ghi;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        glo[r] = c <= Ts ? g[r] : 0.f;
        ghi[r] = c <= Ts ? 0.f : g[r];
      }
      baccum16(Vq, fr, fq, glo, DP);
      baccum16(Vq + STR_PLD, fr, fq, ghi, DP);
    }
  }
  if (c >= 2 * T) return;                                    // the workspace has 2 T rows per batch
  float* drow = a.dflat + ((long)b * 2 * T + c) * ((long)a.H * ATT_DK) + h * ATT_DK;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) st4(drow + dt * 16 + fq * 4, f4(DP[dt]));
}

// dpos row n += sum over b, ascending, of (dflat[b][n + 1] + dflat[b][n + Ts + 2]): the lower and the upper diagonal of pos row n
template <typename E>
__global__ __launch_bounds__(256) void rel_bwd_dpos_sum_kernel(const RelBwdArgs<E> a) {
  const int D4 = a.H * ATT_DK / 4;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.T * D4) return;
  const int n = (int)(idx / D4), c4 = (int)(idx % D4);
  const int Ts = attn_shift_len(a.tshift, a.T);
  if (n >= Ts) return;                                       // rows from Ts on take no position gradient
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b = 0; b < a.B; ++b) {
    const float* base = a.dflat + (long)b * 2 * a.T * (4L * D4) + 4 * c4;
    const float4 lo = *reinterpret_cast<const float4*>(base + (long)(n + 1) * (4L * D4));
    s.x += lo.x; s.y += lo.y; s.z += lo.z; s.w += lo.w;
    if (n <= Ts - 3) {
      const float4 hi = *reinterpret_cast<const float4*>(base + (long)(n + Ts + 2) * (4L * D4));
      s.x += hi.x; s.y += hi.y; s.z += hi.z; s.w += hi.w;
    }
  }
  float4* d = reinterpret_cast<float4*>(a.dpos + (long)n * a.lddpos + 4 * c4);
  float4 y = *d;
  y.x += s.x; y.y += s.y; y.z += s.z; y.w += s.w;
  *d = y;
}

// the checks of stream_bwd_check (attn_stream_bwd.hip) and the forward's rules for qv / pos; they return before anything is launched
template <typename E>
int rel_bwd_check(const RelBwdArgs<E>& a, int T1, int T2, int dk) {
  const bool operands = a.dctx && a.ctx && a.qu && a.qv && a.k && a.v && a.pos && a.lse && a.delta && a.hi && a.dflat && a.dqu &&
                        a.dqv && a.dk && a.dv && a.dpos;
  if (const int rc = attn_check_common(operands, a.B, a.H, T1, T2, a.drop_p, a.drop_step)) return rc;
  if (dk != ATT_DK || T1 != T2 || T1 > (1 << 29)) return EAMD_EUNSUPPORTED;
  if (!stream_in_ok(a.dctx, a.ldd) || !stream_in_ok(a.ctx, a.ldc) || !stream_in_ok(a.qu, a.ldq) || !stream_in_ok(a.qv, a.ldqv) ||
      !stream_in_ok(a.k, a.ldk) || !stream_in_ok(a.v, a.ldv) || !stream_in_ok(a.pos, a.ldpos) || !stream_out_ok(a.dqu, a.lddqu) ||
      !stream_out_ok(a.dqv, a.lddqv) || !stream_out_ok(a.dk, a.lddk) || !stream_out_ok(a.dv, a.lddv) ||
      !stream_out_ok(a.dpos, a.lddpos) || !al16(a.hi) || !al16(a.dflat))
    return EAMD_EUNSUPPORTED;
  return attn_too_many<E>(a.B, a.H, 2 * T1) ? EAMD_EUNSUPPORTED : EAMD_OK;
}

template <typename E, bool DROP>
int rel_bwd_launch(const RelBwdArgs<E>& a, hipStream_t s) {
  const int B = a.B, H = a.H, T1 = a.T;
  const long D4 = (long)H * ATT_DK / 4;
  if constexpr (sizeof(E) == 2) {                            // bf16 storage: delta from its own sweep, not from the rounded ctx
    hipLaunchKernelGGL((rel_bwd_q_kernel<E, true, DROP>), dim3(attn_grid(a.nqb, B, H)), dim3(STR_NT), 0, s, a);
    EAMD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((rel_bwd_q_kernel<E, false, DROP>), dim3(attn_grid(a.nqb, B, H)), dim3(STR_NT), 0, s, a);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((rel_bwd_dqv_shift_kernel<E>), dim3((unsigned)(((long)B * T1 * D4 + 255) / 256)), dim3(256), 0, s, a);
  EAMD_LAUNCH_CHECK();
  hipLaunchKernelGGL((rel_bwd_kv_kernel<E, DROP>), dim3(attn_grid(a.nqb, B, H)), dim3(STR_NT), 0, s, a);       // reads the delta written above
  EAMD_LAUNCH_CHECK();
  if (const int rc = attn_launch<rel_bwd_dpos_kernel<E, DROP>>(DP_LDS, attn_grid(a.ndb, B, H), STR_NT, DP_LDS, s, a)) return rc;
  hipLaunchKernelGGL((rel_bwd_dpos_sum_kernel<E>), dim3((unsigned)(((long)T1 * D4 + 255) / 256)), dim3(256), 0, s, a);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

template <typename E>
int rel_bwd_entry(const void* dctx, int64_t ldd, const void* ctx, int64_t ldc, const void* qu, int64_t ldq, const void* qv, int64_t ldqv,
                  const void* k, int64_t ldk, const void* v, int64_t ldv, const void* pos, int64_t ldpos, const unsigned char* mask,
                  int64_t mb, int64_t mi, const float* lse, const int32_t* shift_len, float* delta_ws, float* dqv_ws, float* dpos_ws,
                  float* dqu, int64_t lddqu, float* dqv, int64_t lddqv, void* dk_out, int64_t lddk, void* dv, int64_t lddv, float* dpos,
                  int64_t lddpos, int B, int H, int T1, int T2, int dk, float scale, void* stream, float drop_p = 0.f,
                  const uint64_t* drop_step = nullptr, uint64_t drop_salt = 0) {
  RelBwdArgs<E> a;
  a.dctx = (const E*)dctx; a.ctx = (const E*)ctx; a.qu = (const E*)qu; a.qv = (const E*)qv; a.k = (const E*)k; a.v = (const E*)v;
  a.pos = (const E*)pos; a.mask = mask; a.lse = lse; a.tshift = shift_len;
  a.delta = delta_ws; a.hi = dqv_ws; a.dflat = dpos_ws;
  a.dqu = dqu; a.dqv = dqv; a.dk = (E*)dk_out; a.dv = (E*)dv; a.dpos = dpos;
  a.ldd = ldd; a.ldc = ldc; a.ldq = ldq; a.ldqv = ldqv; a.ldk = ldk; a.ldv = ldv; a.ldpos = ldpos; a.mb = mb; a.mi = mi;
  a.lddqu = lddqu; a.lddqv = lddqv; a.lddk = lddk; a.lddv = lddv; a.lddpos = lddpos;
  a.B = B; a.H = H; a.T = T1; a.scale = scale;
  a.drop_p = drop_p; a.drop_step = (const unsigned long long*)drop_step; a.drop_salt = drop_salt; a.ldp = stream_ldp(T2);
  if (const int rc = rel_bwd_check(a, T1, T2, dk)) return rc;
  a.nqb = (T1 + STR_QB - 1) / STR_QB;
  a.ndb = (2 * T1 + STR_QB - 1) / STR_QB;                    // flat columns 0 .. 2 T - 1
  hipStream_t s = (hipStream_t)stream;
  return drop_p > 0.f ? rel_bwd_launch<E, true>(a, s) : rel_bwd_launch<E, false>(a, s);
}

}  // namespace

extern "C" int eamd_attn_bwd_stream_rel_f32(const float* dctx, int64_t ldd, const float* ctx, int64_t ldc, const float* qu, int64_t ldq,
                                            const float* qv, int64_t ldqv, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                            const float* pos, int64_t ldpos, const unsigned char* mask, int64_t mask_bstride,
                                            int64_t mask_qstride, const float* lse, const int32_t* shift_len, float* delta_ws,
                                            float* dqv_ws, float* dpos_ws, float* dqu, int64_t lddqu, float* dqv, int64_t lddqv,
                                            float* dk_out, int64_t lddk, float* dv, int64_t lddv, float* dpos, int64_t lddpos, int B,
                                            int H, int T1, int T2, int dk, float scale, void* stream) {
  return rel_bwd_entry<float>(dctx, ldd, ctx, ldc, qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mask_bstride, mask_qstride, lse,
                              shift_len, delta_ws, dqv_ws, dpos_ws, dqu, lddqu, dqv, lddqv, dk_out, lddk, dv, lddv, dpos, lddpos, B, H,
                              T1, T2, dk, scale, stream);
}

extern "C" int eamd_attn_bwd_stream_rel(const void* dctx, int64_t ldd, const void* ctx, int64_t ldc, const void* qu, int64_t ldq,
                                        const void* qv, int64_t ldqv, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                        const void* pos, int64_t ldpos, const unsigned char* mask, int64_t mask_bstride,
                                        int64_t mask_qstride, const float* lse, const int32_t* shift_len, float* delta_ws,
                                        float* dqv_ws, float* dpos_ws, float* dqu, int64_t lddqu, float* dqv, int64_t lddqv,
                                        void* dk_bf16, int64_t lddk, void* dv_bf16, int64_t lddv, float* dpos, int64_t lddpos, int B,
                                        int H, int T1, int T2, int dk, float scale, void* stream) {
  return rel_bwd_entry<bf16_t>(dctx, ldd, ctx, ldc, qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mask_bstride, mask_qstride, lse,
                               shift_len, delta_ws, dqv_ws, dpos_ws, dqu, lddqu, dqv, lddqv, dk_bf16, lddk, dv_bf16, lddv, dpos, lddpos,
                               B, H, T1, T2, dk, scale, stream);
}

// the backward of eamd_attn_fwd_stream_drop[_f32] called with qv / pos, at the same (drop_p, drop_step, drop_salt): the keep bits are
// drawn again per tile in all three sweeps (and in bf16 storage's delta sweep).  drop_p == 0 launches the kernels of the entry
// points above: their bits
extern "C" int eamd_attn_bwd_stream_rel_drop_f32(const float* dctx, int64_t ldd, const float* ctx, int64_t ldc, const float* qu,
                                                 int64_t ldq, const float* qv, int64_t ldqv, const float* k, int64_t ldk, const float* v,
                                                 int64_t ldv, const float* pos, int64_t ldpos, const unsigned char* mask,
                                                 int64_t mask_bstride, int64_t mask_qstride, const float* lse, const int32_t* shift_len,
                                                 float* delta_ws, float* dqv_ws, float* dpos_ws, float* dqu, int64_t lddqu, float* dqv,
                                                 int64_t lddqv, float* dk_out, int64_t lddk, float* dv, int64_t lddv, float* dpos,
                                                 int64_t lddpos, int B, int H, int T1, int T2, int dk, float scale, float drop_p,
                                                 const uint64_t* drop_step, uint64_t drop_salt, void* stream) {
  return rel_bwd_entry<float>(dctx, ldd, ctx, ldc, qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mask_bstride, mask_qstride, lse,
                              shift_len, delta_ws, dqv_ws, dpos_ws, dqu, lddqu, dqv, lddqv, dk_out, lddk, dv, lddv, dpos, lddpos, B, H,
                              T1, T2, dk, scale, stream, drop_p, drop_step, drop_salt);
}

extern "C" int eamd_attn_bwd_stream_rel_drop(const void* dctx, int64_t ldd, const void* ctx, int64_t ldc, const void* qu, int64_t ldq,
                                             const void* qv, int64_t ldqv, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                             const void* pos, int64_t ldpos, const unsigned char* mask, int64_t mask_bstride,
                                             int64_t mask_qstride, const float* lse, const int32_t* shift_len, float* delta_ws,
                                             float* dqv_ws, float* dpos_ws, float* dqu, int64_t lddqu, float* dqv, int64_t lddqv,
                                             void* dk_bf16, int64_t lddk, void* dv_bf16, int64_t lddv, float* dpos, int64_t lddpos,
                                             int B, int H, int T1, int T2, int dk, float scale, float drop_p,
                                             const uint64_t* drop_step, uint64_t drop_salt, void* stream) {
  return rel_bwd_entry<bf16_t>(dctx, ldd, ctx, ldc, qu, ldq, qv, ldqv, k, ldk, v, ldv, pos, ldpos, mask, mask_bstride, mask_qstride, lse,
                               shift_len, delta_ws, dqv_ws, dpos_ws, dqu, lddqu, dqv, lddqv, dk_bf16, lddk, dv_bf16, lddv, dpos, lddpos,
                               B, H, T1, T2, dk, scale, stream, drop_p, drop_step, drop_salt);
}
