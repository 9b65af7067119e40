// Batched greedy transducer decoding: frame t of up to 64 utterances in two launches.
// reference: espnet/nets/beam_search_transducer.py:130-161 (greedy_search: at most one symbol per frame, so all utterances of a
// batch walk the frames in lock-step), transducer/joint_network.py:45-46 (lin_out(act(lin_enc(h_enc) + lin_dec(h_dec)))).
//
//   eamd_rnnt_greedy_joint   logits[b, v] = sum_k act(enc_proj[b, t, k] + d[b, k]) W_out[v, k] + b_out[v] on 16-row x 16-column
//                            tiles; the [B, V] logits are never written: a tile leaves (maximum, its lowest token id,
//                            sum exp(logit - maximum)) per row - the three numbers an argmax and its log-probability need.
//                            A workgroup owns 16 columns of W_out and serves every row block, so W_out is read once per frame
//                            (its four waves split the reduction over J and meet in LDS); operands go straight from global memory / L2 into v_mfma_f32_16x16x4_f32 (decode.hip:
//                            linear_mfma16_ln_f32_kernel, rnn.hip: lstm_step_fwd_kernel), the joint activation is applied to the
//                            A fragment on its way in.  J % 4 != 0 (or operands that are not 16-byte aligned): the same tiles
//                            from scalar loads and FMAs.
//   eamd_rnnt_greedy_pick    one workgroup, one wave per row: merges the row's tile records (first maximum = lowest id among equal
//                            logits, torch.max / eamd_argmax_rows), logp = -log(sum exp(logit - max)), and does the search's
//                            bookkeeping for the frame with plain stores - the `live` mask it leaves is the one the LSTM / GRU cell
//                            kernels take (0 = state carried through unchanged).
// Both read the frame index as t, or *t_dev + t (eamd_decode_self_attn_dyn's pos_dev convention): one captured graph serves every
// frame; pick advances *t_dev after every row has read it.
#include "common.h"
#include "select.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int RG_TILE = 16;            // columns per tile record (one workgroup)
constexpr int RG_WAVES = 4;            // waves per workgroup: each takes every fourth 16-k round of the reduction
constexpr int RG_REC = 4;              // floats per record: maximum, token id (bits), sum of exp, unused

template <int MT, bool VEC>
__global__ __launch_bounds__(64 * RG_WAVES) void rnnt_greedy_joint_kernel(const float* __restrict__ enc, const float* __restrict__ d,
                                                                          const float* __restrict__ W, const float* __restrict__ bias,
                                                                          float* __restrict__ part, int B, int T, int J, int V,
                                                                          int act, int t, const int* __restrict__ t_dev) {
  // a workgroup owns one tile of 16 columns; its waves split the reduction over J (the step is latency-bound: a wave alone walks
  // J / 16 dependent load + activation + MFMA rounds) and meet in LDS, in a fixed order
  __shared__ float red[RG_WAVES][MT * 4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int tile = blockIdx.x;
  const int ntile = (V + RG_TILE - 1) / RG_TILE;
  const int n0 = tile * RG_TILE;
  int tt = t + (t_dev ? *t_dev : 0);
  tt = min(max(tt, 0), T - 1);                                 // a frame beyond the buffer is never live (pick); read a valid one
  f32x4 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* wr = W + (long)min(n0 + fr, V - 1) * J;         // clamped rows / columns are computed and never stored
  if (VEC) {
    // lane (fr, fq): A row = batch row i * 16 + fr, B row = column n0 + fr, four consecutive k at k0 + 4 fq
    const float* er[MT];
    const float* dr[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = min(i * 16 + fr, B - 1);
      er[i] = enc + ((long)m * T + tt) * J;
      dr[i] = d + (long)m * J;
    }
    for (int k0 = 16 * wave; k0 < J; k0 += 16 * RG_WAVES) {
      const int k = k0 + fq * 4;
      const bool in = k < J;                                   // J % 4 == 0: a float4 is inside the row or outside it
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 b4 = in ? *reinterpret_cast<const float4*>(wr + k) : z4;
      float4 a4[MT];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const float4 e = in ? *reinterpret_cast<const float4*>(er[i] + k) : z4;
        const float4 p = in ? *reinterpret_cast<const float4*>(dr[i] + k) : z4;
        a4[i] = in ? make_float4(eamd_act(e.x + p.x, act), eamd_act(e.y + p.y, act), eamd_act(e.z + p.z, act),
                                 eamd_act(e.w + p.w, act)) : z4;
      }
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i].x, b4.x, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i].y, b4.y, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i].z, b4.z, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i].w, b4.w, acc[i], 0, 0, 0);
      }
    }
  } else {
    // scalar tail form, same accumulator layout: lane (fr, fq) owns column n0 + fr of rows i * 16 + 4 fq + r
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = min(i * 16 + fq * 4 + r, B - 1);
        const float* e = enc + ((long)m * T + tt) * J;
        const float* p = d + (long)m * J;
        float s = 0.f;
        for (int k = wave; k < J; k += RG_WAVES) s = fmaf(eamd_act(e[k] + p[k], act), wr[k], s);
        acc[i][r] = s;
      }
    }
  }
  // accumulator layout: lane (fr = column, fq) holds rows 4 fq + r of the tile
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][i * 4 + r][lane] = acc[i][r];
  __syncthreads();
  if (wave != 0) return;
  const int n = n0 + fr;
  const float bv = (n < V && bias) ? bias[n] : 0.f;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float a = red[0][i * 4 + r][lane];
#pragma unroll
      for (int w = 1; w < RG_WAVES; ++w) a += red[w][i * 4 + r][lane];
      const float v = n < V ? a + bv : -INFINITY;              // columns past V never win and add exp(-inf) = 0
      float mx = v;
      int id = n;
      wave_first_max<16>(mx, id);                              // the 16 lanes that share fq (one accumulator row)
      float s = n < V ? __expf(v - mx) : 0.f;
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
      const int m = i * 16 + fq * 4 + r;
      if (fr == 0 && m < B)
        *reinterpret_cast<float4*>(part + ((long)m * ntile + tile) * RG_REC) = make_float4(mx, __int_as_float(id), s, 0.f);
    }
  }
}

__global__ __launch_bounds__(1024) void rnnt_greedy_pick_kernel(const float* __restrict__ part, const int* __restrict__ hlens,
                                                                int* __restrict__ yseq, int* __restrict__ ylen,
                                                                float* __restrict__ score, long long* __restrict__ tok,
                                                                unsigned char* __restrict__ live, int B, int T, int V, int ycap,
                                                                int blank, int t, int* __restrict__ t_dev) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int ntile = (V + RG_TILE - 1) / RG_TILE;
  const int tt = t + (t_dev ? *t_dev : 0);
  for (int b = wave; b < B; b += nw) {
    const float* pr = part + (long)b * ntile * RG_REC;
    float mx = -INFINITY;
    int id = 0x7fffffff;
    for (int j = lane; j < ntile; j += 64) {                   // tiles in ascending order: a later equal maximum does not replace
      const float4 rec = *reinterpret_cast<const float4*>(pr + (long)j * RG_REC);
      first_max(mx, id, rec.x, __float_as_int(rec.y));
    }
    wave_first_max<64>(mx, id);
    float s = 0.f;
    for (int j = lane; j < ntile; j += 64) {
      const float4 rec = *reinterpret_cast<const float4*>(pr + (long)j * RG_REC);
      s += rec.z * __expf(rec.x - mx);
    }
    s = wave_sum(s);
    if (lane == 0) {
      const int lim = hlens ? min(hlens[b], T) : T;
      const int len = ylen[b];
      const bool on = tt >= 0 && tt < lim && id != blank && id >= 0 && id < V && len < ycap;
      if (on) {
        yseq[(long)b * ycap + len] = id;
        ylen[b] = len + 1;
        score[b] -= logf(s);
      }
      tok[b] = on ? id : blank;
      live[b] = on ? 1 : 0;
    }
  }
  if (t_dev) {
    __syncthreads();                                           // every wave has read the counter
    if (threadIdx.x == 0) *t_dev = tt - t + 1;
  }
}

}  // namespace

extern "C" {

int eamd_rnnt_greedy_part_floats(int B, int V) {
  if (B <= 0 || V <= 0 || (int64_t)B * ((V + RG_TILE - 1) / RG_TILE) * RG_REC > 0x7fffffff) return 0;
  return B * ((V + RG_TILE - 1) / RG_TILE) * RG_REC;
}

int eamd_rnnt_greedy_joint(const float* enc_proj, const float* d, const float* w_out, const float* b_out, float* part, int B, int T,
                           int J, int V, int act, int t, const int32_t* t_dev, void* stream) {
  if (!enc_proj || !d || !w_out || !part || B < 1 || B > 64 || T < 1 || J < 1 || V < 2 || t < 0) return EAMD_EINVAL;
  if (act != EAMD_ACT_TANH && act != EAMD_ACT_RELU && act != EAMD_ACT_SWISH && act != EAMD_ACT_NONE) return EAMD_EINVAL;
  if (((uintptr_t)part) & 15) return EAMD_EINVAL;
  const int ntile = (V + RG_TILE - 1) / RG_TILE;
  const dim3 grid(ntile), block(64 * RG_WAVES);
  const bool vec = J % 4 == 0 && !(((uintptr_t)enc_proj | (uintptr_t)d | (uintptr_t)w_out) & 15);
  const int mt = (B + 15) / 16;
  hipStream_t s = (hipStream_t)stream;
#define EAMD_RGJ(MT_, VEC_) hipLaunchKernelGGL((rnnt_greedy_joint_kernel<MT_, VEC_>), grid, block, 0, s, enc_proj, d, w_out, b_out, part, B, T, J, V, act, t, t_dev)
  if (vec) {
    if (mt == 1) EAMD_RGJ(1, true); else if (mt == 2) EAMD_RGJ(2, true); else if (mt == 3) EAMD_RGJ(3, true); else EAMD_RGJ(4, true);
  } else {
    if (mt == 1) EAMD_RGJ(1, false); else if (mt == 2) EAMD_RGJ(2, false); else if (mt == 3) EAMD_RGJ(3, false); else EAMD_RGJ(4, false);
  }
#undef EAMD_RGJ
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_rnnt_greedy_pick(const float* part, const int32_t* hlens, int32_t* yseq, int32_t* ylen, float* score, int64_t* tok,
                          uint8_t* live, int B, int T, int V, int ycap, int blank, int t, int32_t* t_dev, void* stream) {
  if (!part || !yseq || !ylen || !score || !tok || !live || B < 1 || B > 64 || T < 1 || V < 2 || ycap < 1 || blank < 0 ||
      blank >= V || t < 0)
    return EAMD_EINVAL;
  if (((uintptr_t)part) & 15) return EAMD_EINVAL;
  hipLaunchKernelGGL(rnnt_greedy_pick_kernel, dim3(1), dim3(64 * (B < 16 ? B : 16)), 0, (hipStream_t)stream, part, hlens, yseq, ylen,
                     score, reinterpret_cast<long long*>(tok), live, B, T, V, ycap, blank, t, t_dev);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
