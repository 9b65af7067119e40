// Memory-linear attention backward for training without relative positions, d_k = 64, any number of keys, fp32 or bf16 storage,
// on the fp32 matrix cores (v_mfma_f32_16x16x4_f32).  The forward (attn_stream.hip, LSE flag) kept ctx and the row statistic
// lse_i = log sum_j exp(s_ij) of the scaled, masked scores; both kernels here rebuild P_ij = exp(s_ij - lse_i) tile by tile from
// qu and k, so no [T1, T2] matrix exists in either direction.  No atomics: every output element has one owner, which sums in a
// fixed order - the same bits on every launch.
//   dP = dctx v^T,  delta_i = sum_j P_ij dP_ij = sum_c dctx_ic ctx_ic,  dS = scale P (dP - delta),
//   dq = dS k,  dk = dS^T qu,  dv = P^T dctx.
// reference: autograd of transformer/attention.py:63-114 (forward_attention).
//
// Query side (stream_bwd_q_kernel).  One workgroup = one (batch, head) pair x 64 queries, four waves, pairs dealt to the XCDs by
// attn_xcd_pair / attn_xcd_block; wave w owns queries 16 w .. 16 w + 15 for the whole sweep over the keys, exactly as in the
// forward.  A lane keeps the qu and dctx fragments of query fr, lse_i and delta_i (its own 16 channels of dctx . ctx, summed over
// the four 16-lane groups; lane group 0 also writes it to the workspace the key side reads) and the transposed accumulator
// dq^T[channel][query].  K and V tiles of KT = 32 keys are staged once per workgroup as [row][68] floats; the global loads of
// tile t + 1 are issued behind tile t's LDS stores and land under its products.  S^T[key][query] = K_tile qu^T and
// dP^T[key][query] = V_tile dctx^T leave the matrix cores with four adjacent keys of query fr per lane - the B operand of
// dq^T += K_tile^T dS^T - so neither P nor dS touches LDS.
// Key side (stream_bwd_kv_kernel), launched behind it.  One workgroup = one pair x 64 keys; wave w owns keys 16 w .. 16 w + 15, its
// K and V fragments stay in registers, and the workgroup sweeps query tiles of 32: qu and dctx rows staged as above, lse and
// delta of the tile beside them.  S[query][key] = Q_tile k^T and dP[query][key] = dCtx_tile v^T give a lane four adjacent queries
// of key fr - the B operand of dv^T[channel][key] += dCtx_tile^T P and dk^T[channel][key] += Q_tile^T dS.  The mask byte of a
// (query, key) element is read per element: four clamped byte loads of stride mask_qstride per 16-query piece.
// Both kernels: 17.4 / 17.7 KB of LDS and launch bounds for TWO workgroups per CU (eight waves), the occupancy the forward was
// measured to need to hide its fragment-load latency.
// Hazards:
//   * keys >= T2: attn_score sets the score to -inf by index, so P = 0; their staged K rows are clamped re-reads (finite) and
//     their V rows zeros, so dP is finite and dS = 0 * finite = 0 exactly;
//   * queries >= T1 of a staged tile (key side): the probability is SELECTED to zero on the index - a clamped re-read would carry
//     the last row's lse and a non-zero delta - and their qu / dctx / lse / delta are staged as zeros, so the zero probability
//     never meets a stale value; on the query side such lanes compute on a clamped re-read and are not stored;
//   * a dead row (every key masked) has lse = 0 and every score -inf: exp(-inf - 0) = 0, so dq = 0 exactly and the row adds
//     nothing to dk / dv; its ctx is zero, so delta = 0;
//   * T1 != T2, T1 = 1 and operands / outputs that are column blocks of wider buffers: every tensor has its own row stride and
//     outputs are written in pieces of four elements inside their 64 columns only.
#include "attn_stream_common.h"

namespace {

template <typename T>
struct StreamBwdArgs {
  const T* dctx; const T* ctx; const T* qu; const T* k; const T* v;
  const unsigned char* mask;
  const float* lse; float* delta;
  T* dq; T* dk; T* dv;
  long ldd, ldc, ldq, ldk, ldv, mb, mi, lddq, lddk, lddv;
  int B, H, T1, T2, nqb, nkb;
  float scale;
  // the forward's attention dropout (DROP kernels): the keep bits of P's stored layout [H*B][T1][ldp], attn_stream_common.h
  float drop_p; const unsigned long long* drop_step; unsigned long long drop_salt; long ldp;
};

// acc^T[channel 16 dt + 4 fq + r][column fr] += sum over the tile's rows of X[row][channel] w[row][column fr]; w[t][r]: row 16 t + 4 fq + r
__device__ __forceinline__ void baccum(const float* X, int fr, int fq, const f32x4 (&w)[STR_NKT], f32x4 (&acc)[4]) {
#pragma unroll
  for (int t = 0; t < STR_NKT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* row = &X[(16 * t + 4 * fq + r) * STR_PLD + fr];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[dt * 16], w[t][r], acc[dt], 0, 0, 0);
    }
}

// DROP (both kernels): the forward built ctx from Pd = P o M / (1 - p).  delta = dctx . ctx is unchanged in form (sum_j P dP =
// sum_j Pd dPd), dP <- M / (1 - p) o (dctx v^T) in dS, and dv takes Pd; M is regenerated per tile (stream_drop_row / _keep_col)
template <typename T, bool DROP>
__global__ __launch_bounds__(STR_NT, 2) void stream_bwd_q_kernel(const StreamBwdArgs<T> a) {
  __shared__ __attribute__((aligned(16))) float Ks[STR_KT * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Vs[STR_KT * STR_PLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int z = attn_xcd_pair(blockIdx.x, a.nqb);            // z = h * B + b
  if (z >= a.B * a.H) return;                                // whole workgroup
  const int h = z / a.B, b = z % a.B;
  const int T1 = a.T1, T2 = a.T2;
  const int i0 = attn_xcd_block(blockIdx.x, a.nqb) * STR_QB + 16 * wave;
  const bool active = i0 < T1;                               // wave-uniform; idle waves still stage and keep the barriers
  const int i = i0 + fr;                                     // this lane's query (rows past T1: clamped re-reads, never stored)
  const int qi = min(i, T1 - 1);
  const int ntile = (T2 + STR_KT - 1) / STR_KT;
  const T* ks = a.k + (long)b * T2 * a.ldk + h * ATT_DK;
  const T* vs = a.v + (long)b * T2 * a.ldv + h * ATT_DK;
  const unsigned char* mr = a.mask ? a.mask + (long)b * a.mb + (long)qi * a.mi : nullptr;

  float4 qf[4], df[4];
  frag_global(a.qu + ((long)b * T1 + qi) * a.ldq + h * ATT_DK, fq, qf);
  frag_global(a.dctx + ((long)b * T1 + qi) * a.ldd + h * ATT_DK, fq, df);
  const float lse = a.lse[(long)z * T1 + qi];
  float delta = 0.f;
  {
    float4 cf[4];
    frag_global(a.ctx + ((long)b * T1 + qi) * a.ldc + h * ATT_DK, fq, cf);
#pragma unroll
    for (int j = 0; j < 4; ++j) delta += df[j].x * cf[j].x + df[j].y * cf[j].y + df[j].z * cf[j].z + df[j].w * cf[j].w;
    delta = attn_sum16_32(delta);
    if (active && fq == 0 && i < T1) a.delta[(long)z * T1 + i] = delta;
  }

  float4 kr[STR_KQ], vr[STR_KQ];                                   // register stage: one key tile on its way to LDS
  unsigned mkn[STR_NKT];
  auto request = [&](int jt) {
    const int j0 = jt * STR_KT;
#pragma unroll
    for (int q = 0; q < STR_KQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      const long key = min(j0 + row, T2 - 1);
      kr[q] = ld4(ks + key * a.ldk + 4 * c4);
      vr[q] = ld4(vs + key * a.ldv + 4 * c4);
      if (j0 + row >= T2) vr[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) mkn[kt] = mr ? attn_mask4(mr, j0 + 16 * kt + 4 * fq, T2) : 0x01010101u;
  };

  const AttnDrop drop = DROP ? attn_drop_setup(a.drop_p, a.drop_step, a.drop_salt) : AttnDrop{};
  const long pro = ((long)z * T1 + qi) * a.ldp;              // DROP: where this query's row of P would start
  f32x4 DQ[4];                                               // DQ[dt][r]: channel 16 dt + 4 fq + r of query fr
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) DQ[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

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
    unsigned mk[STR_NKT];
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) mk[kt] = mkn[kt];
    __syncthreads();
    if (jt + 1 < ntile) request(jt + 1);                     // in flight under this tile's products
    if (!active) continue;

    f32x4 S[STR_NKT], dP[STR_NKT];                                 // [kt][r]: key j0 + 16 kt + 4 fq + r, query fr
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt) {
      float4 xf[4];
      frag_lds(&Ks[(16 * kt + fr) * STR_PLD], fq, xf);
      S[kt] = dot64(xf, qf, (f32x4){0.f, 0.f, 0.f, 0.f});
      frag_lds(&Vs[(16 * kt + fr) * STR_PLD], fq, xf);
      dP[kt] = dot64(xf, df, (f32x4){0.f, 0.f, 0.f, 0.f});
    }
    if (DROP) stream_drop_row(drop, pro, j0, fq, a.ldp, dP);
#pragma unroll
    for (int kt = 0; kt < STR_NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(attn_score(S[kt][r], a.scale, j0 + 16 * kt + 4 * fq + r, T2, mk[kt], r) - lse);
        S[kt][r] = a.scale * p * (dP[kt][r] - delta);        // dS^T[key][query]
      }
    baccum(Ks, fr, fq, S, DQ);                               // dq^T[channel][query] += K_tile^T[channel][key] dS^T[key][query]
  }
  if (!active || i >= T1) return;
  T* drow = a.dq + ((long)b * T1 + i) * a.lddq + h * ATT_DK;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) st4(drow + dt * 16 + fq * 4, f4(DQ[dt]));
}

template <typename T, bool DROP>
__global__ __launch_bounds__(STR_NT, 2) void stream_bwd_kv_kernel(const StreamBwdArgs<T> a) {
  __shared__ __attribute__((aligned(16))) float Qs[STR_KT * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Ds[STR_KT * STR_PLD];
  __shared__ __attribute__((aligned(16))) float Ls[STR_KT], Es[STR_KT];                         // lse and delta of the staged queries
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int z = attn_xcd_pair(blockIdx.x, a.nkb);
  if (z >= a.B * a.H) return;                                // whole workgroup
  const int h = z / a.B, b = z % a.B;
  const int T1 = a.T1, T2 = a.T2;
  const int j0w = attn_xcd_block(blockIdx.x, a.nkb) * STR_QB + 16 * wave;
  const bool active = j0w < T2;                              // wave-uniform
  const int j = j0w + fr;                                    // this lane's key (past T2: a clamped re-read, masked by index, never stored)
  const int kj = min(j, T2 - 1);
  const int ntile = (T1 + STR_KT - 1) / STR_KT;
  const T* qs = a.qu + (long)b * T1 * a.ldq + h * ATT_DK;
  const T* ds = a.dctx + (long)b * T1 * a.ldd + h * ATT_DK;
  const float* ls = a.lse + (long)z * T1;
  const float* es = a.delta + (long)z * T1;
  const unsigned char* mc = a.mask ? a.mask + (long)b * a.mb + kj : nullptr;     // this key's column of the pair's mask rows

  float4 kf[4], vf[4];
  frag_global(a.k + ((long)b * T2 + kj) * a.ldk + h * ATT_DK, fq, kf);
  frag_global(a.v + ((long)b * T2 + kj) * a.ldv + h * ATT_DK, fq, vf);

  float4 qr[STR_KQ], dr[STR_KQ];                                   // register stage: one query tile on its way to LDS
  float sr = 0.f;                                            // threads 0 .. 31: lse, 32 .. 63: delta of tile row t & 31
  unsigned mkn[STR_NKT];
  auto request = [&](int it) {
    const int i0 = it * STR_KT;
#pragma unroll
    for (int q = 0; q < STR_KQ; ++q) {
      const int c = t + STR_NT * q, row = c >> 4, c4 = c & 15;
      const long qrow = min(i0 + row, T1 - 1);
      qr[q] = ld4(qs + qrow * a.ldq + 4 * c4);
      dr[q] = ld4(ds + qrow * a.ldd + 4 * c4);
      if (i0 + row >= T1) qr[q] = dr[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (t < 2 * STR_KT) {
      const int row = t & (STR_KT - 1);
      sr = (t < STR_KT ? ls : es)[min(i0 + row, T1 - 1)];
      if (i0 + row >= T1) sr = 0.f;
    }
#pragma unroll
    for (int qt = 0; qt < STR_NKT; ++qt) {
      unsigned w = 0x01010101u;
      if (mc) {
        w = 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) w |= (unsigned)mc[(long)min(i0 + 16 * qt + 4 * fq + r, T1 - 1) * a.mi] << (8 * r);
      }
      mkn[qt] = w;
    }
  };

  const AttnDrop drop = DROP ? attn_drop_setup(a.drop_p, a.drop_step, a.drop_salt) : AttnDrop{};
  const long pcol = (long)z * T1 * a.ldp + j;                // DROP: this key's column of the pair's P
  f32x4 DV[4], DK[4];                                        // [dt][r]: channel 16 dt + 4 fq + r of key fr
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) DV[dt] = DK[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

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
    if (t < STR_KT) Ls[t] = sr;
    else if (t < 2 * STR_KT) Es[t - STR_KT] = sr;
    unsigned mk[STR_NKT];
#pragma unroll
    for (int qt = 0; qt < STR_NKT; ++qt) mk[qt] = mkn[qt];
    __syncthreads();
    if (it + 1 < ntile) request(it + 1);                     // in flight under this tile's products
    if (!active) continue;

    f32x4 P[STR_NKT], dS[STR_NKT];                                 // [qt][r]: query i0 + 16 qt + 4 fq + r, key fr
#pragma unroll
    for (int qt = 0; qt < STR_NKT; ++qt) {
      float4 xf[4];
      frag_lds(&Qs[(16 * qt + fr) * STR_PLD], fq, xf);
      P[qt] = dot64(xf, kf, (f32x4){0.f, 0.f, 0.f, 0.f});
      frag_lds(&Ds[(16 * qt + fr) * STR_PLD], fq, xf);
      dS[qt] = dot64(xf, vf, (f32x4){0.f, 0.f, 0.f, 0.f});
    }
#pragma unroll
    for (int qt = 0; qt < STR_NKT; ++qt) {
      const float4 l4 = *reinterpret_cast<const float4*>(&Ls[16 * qt + 4 * fq]);
      const float4 e4 = *reinterpret_cast<const float4*>(&Es[16 * qt + 4 * fq]);
      const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, eq[4] = {e4.x, e4.y, e4.z, e4.w};
      float m[4];
      if (DROP) stream_keep_col(drop, pcol + (long)(i0 + 16 * qt + 4 * fq) * a.ldp, a.ldp, m);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = __expf(attn_score(P[qt][r], a.scale, j, T2, mk[qt], r) - lq[r]);
        if (i0 + 16 * qt + 4 * fq + r >= T1) p = 0.f;        // by index: a clamped row would carry a live lse and delta
        P[qt][r] = DROP ? p * m[r] : p;                      // Pd for dv
        dS[qt][r] = a.scale * p * ((DROP ? dS[qt][r] * m[r] : dS[qt][r]) - eq[r]);
      }
    }
    baccum(Ds, fr, fq, P, DV);                               // dv^T[channel][key] += dCtx_tile^T[channel][query] P[query][key]
    baccum(Qs, fr, fq, dS, DK);                              // dk^T[channel][key] += Q_tile^T[channel][query] dS[query][key]
  }
  if (!active || j >= T2) return;
  T* vrow = a.dv + ((long)b * T2 + j) * a.lddv + h * ATT_DK;
  T* krow = a.dk + ((long)b * T2 + j) * a.lddk + h * ATT_DK;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    st4(vrow + dt * 16 + fq * 4, f4(DV[dt]));
    st4(krow + dt * 16 + fq * 4, f4(DK[dt]));
  }
}

// the checks of stream_check (attn_stream.hip) for the backward's operands; they return before anything is launched
template <typename T>
int stream_bwd_check(const StreamBwdArgs<T>& a, int dk) {
  const bool operands = a.dctx && a.ctx && a.qu && a.k && a.v && a.lse && a.delta && a.dq && a.dk && a.dv;
  if (const int rc = attn_check_common(operands, a.B, a.H, a.T1, a.T2, a.drop_p, a.drop_step)) return rc;
  if (dk != ATT_DK) return EAMD_EUNSUPPORTED;
  if (!stream_in_ok(a.dctx, a.ldd) || !stream_in_ok(a.ctx, a.ldc) || !stream_in_ok(a.qu, a.ldq) || !stream_in_ok(a.k, a.ldk) ||
      !stream_in_ok(a.v, a.ldv) || !stream_out_ok(a.dq, a.lddq) || !stream_out_ok(a.dk, a.lddk) || !stream_out_ok(a.dv, a.lddv))
    return EAMD_EUNSUPPORTED;
  return attn_too_many<T>(a.B, a.H, a.T1 > a.T2 ? a.T1 : a.T2) ? EAMD_EUNSUPPORTED : EAMD_OK;
}

template <typename T>
int stream_bwd_entry(const void* dctx, int64_t ldd, const void* ctx, int64_t ldc, const void* qu, int64_t ldq, const void* k, int64_t ldk,
                     const void* v, int64_t ldv, const unsigned char* mask, int64_t mb, int64_t mi, const float* lse, float* delta_ws,
                     void* dq, int64_t lddq, void* dk_out, int64_t lddk, void* dv, int64_t lddv, int B, int H, int T1, int T2, int dk,
                     float scale, void* stream, float drop_p = 0.f, const uint64_t* drop_step = nullptr, uint64_t drop_salt = 0) {
  StreamBwdArgs<T> a;
  a.dctx = (const T*)dctx; a.ctx = (const T*)ctx; a.qu = (const T*)qu; a.k = (const T*)k; a.v = (const T*)v;
  a.mask = mask; a.lse = lse; a.delta = delta_ws;
  a.dq = (T*)dq; a.dk = (T*)dk_out; a.dv = (T*)dv;
  a.ldd = ldd; a.ldc = ldc; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.mb = mb; a.mi = mi; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
  a.B = B; a.H = H; a.T1 = T1; a.T2 = T2; a.scale = scale;
  a.drop_p = drop_p; a.drop_step = (const unsigned long long*)drop_step; a.drop_salt = drop_salt; a.ldp = stream_ldp(T2);
  if (const int rc = stream_bwd_check(a, dk)) return rc;
  a.nqb = (T1 + STR_QB - 1) / STR_QB;
  a.nkb = (T2 + STR_QB - 1) / STR_QB;
  hipStream_t s = (hipStream_t)stream;
  const dim3 gq(attn_grid(a.nqb, B, H)), gk(attn_grid(a.nkb, B, H));
  if (drop_p > 0.f) hipLaunchKernelGGL((stream_bwd_q_kernel<T, true>), gq, dim3(STR_NT), 0, s, a);
  else hipLaunchKernelGGL((stream_bwd_q_kernel<T, false>), gq, dim3(STR_NT), 0, s, a);
  EAMD_LAUNCH_CHECK();
  if (drop_p > 0.f) hipLaunchKernelGGL((stream_bwd_kv_kernel<T, true>), gk, dim3(STR_NT), 0, s, a);   // reads the delta written above
  else hipLaunchKernelGGL((stream_bwd_kv_kernel<T, false>), gk, dim3(STR_NT), 0, s, a);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // namespace

extern "C" int eamd_attn_bwd_stream_f32(const float* dctx, int64_t ldd, const float* ctx, int64_t ldc, const float* qu, int64_t ldq,
                                        const float* k, int64_t ldk, const float* v, int64_t ldv, const unsigned char* mask,
                                        int64_t mask_bstride, int64_t mask_qstride, const float* lse, float* delta_ws, float* dq,
                                        int64_t lddq, float* dk_out, int64_t lddk, float* dv, int64_t lddv, int B, int H, int T1, int T2,
                                        int dk, float scale, void* stream) {
  return stream_bwd_entry<float>(dctx, ldd, ctx, ldc, qu, ldq, k, ldk, v, ldv, mask, mask_bstride, mask_qstride, lse, delta_ws, dq, lddq,
                                 dk_out, lddk, dv, lddv, B, H, T1, T2, dk, scale, stream);
}

extern "C" int eamd_attn_bwd_stream(const void* dctx, int64_t ldd, const void* ctx, int64_t ldc, const void* qu, int64_t ldq,
                                    const void* k, int64_t ldk, const void* v, int64_t ldv, const unsigned char* mask,
                                    int64_t mask_bstride, int64_t mask_qstride, const float* lse, float* delta_ws, void* dq_bf16,
                                    int64_t lddq, void* dk_bf16, int64_t lddk, void* dv_bf16, int64_t lddv, int B, int H, int T1, int T2,
                                    int dk, float scale, void* stream) {
  return stream_bwd_entry<bf16_t>(dctx, ldd, ctx, ldc, qu, ldq, k, ldk, v, ldv, mask, mask_bstride, mask_qstride, lse, delta_ws, dq_bf16,
                                  lddq, dk_bf16, lddk, dv_bf16, lddv, B, H, T1, T2, dk, scale, stream);
}

// the backward of eamd_attn_fwd_stream_drop[_f32] at the same (drop_p, drop_step, drop_salt): the keep bits are drawn again per
// tile, nothing is stored.  drop_p == 0 launches the kernels of the entry points above: their bits
extern "C" int eamd_attn_bwd_stream_drop_f32(const float* dctx, int64_t ldd, const float* ctx, int64_t ldc, const float* qu, int64_t ldq,
                                             const float* k, int64_t ldk, const float* v, int64_t ldv, const unsigned char* mask,
                                             int64_t mask_bstride, int64_t mask_qstride, const float* lse, float* delta_ws, float* dq,
                                             int64_t lddq, float* dk_out, int64_t lddk, float* dv, int64_t lddv, int B, int H, int T1,
                                             int T2, int dk, float scale, float drop_p, const uint64_t* drop_step, uint64_t drop_salt,
                                             void* stream) {
  return stream_bwd_entry<float>(dctx, ldd, ctx, ldc, qu, ldq, k, ldk, v, ldv, mask, mask_bstride, mask_qstride, lse, delta_ws, dq, lddq,
                                 dk_out, lddk, dv, lddv, B, H, T1, T2, dk, scale, stream, drop_p, drop_step, drop_salt);
}

extern "C" int eamd_attn_bwd_stream_drop(const void* dctx, int64_t ldd, const void* ctx, int64_t ldc, const void* qu, int64_t ldq,
                                         const void* k, int64_t ldk, const void* v, int64_t ldv, const unsigned char* mask,
                                         int64_t mask_bstride, int64_t mask_qstride, const float* lse, float* delta_ws, void* dq_bf16,
                                         int64_t lddq, void* dk_bf16, int64_t lddk, void* dv_bf16, int64_t lddv, int B, int H, int T1,
                                         int T2, int dk, float scale, float drop_p, const uint64_t* drop_step, uint64_t drop_salt,
                                         void* stream) {
  return stream_bwd_entry<bf16_t>(dctx, ldd, ctx, ldc, qu, ldq, k, ldk, v, ldv, mask, mask_bstride, mask_qstride, lse, delta_ws, dq_bf16,
                                  lddq, dk_bf16, lddk, dv_bf16, lddv, B, H, T1, T2, dk, scale, stream, drop_p, drop_step, drop_salt);
}
