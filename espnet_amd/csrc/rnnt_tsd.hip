// Batched time-synchronous transducer beam search: the bookkeeping of one pass (frame t, symbol expansion v) for n utterances in
// one launch.
// reference: espnet/nets/beam_search_transducer.py:239-347 (time_sync_decoding without an LM).  Every frame takes max_sym_exp = M
// passes whatever the hypotheses are, so the utterances of a batch advance in lock-step; what the reference does with Python lists
// per utterance - add the blank continuations of C to A (merging equal label sequences), build D from C's extensions, keep the
// `beam` best of D as the next C and, after the last pass, the `beam` best of A as the next B - is done here by one workgroup per
// utterance on W <= 16 slots, at most 16 * 16 = 256 candidates in D and W * M <= 64 entries in A.
//
//   eamd_rnnt_tsd_step   reads eamd_transducer_expand_rows' record of the pass's n * W rows, the block that holds C and the A of the
//                        frame; updates A; on a pass v < M - 1 writes the block of pass v + 1, at v == M - 1 the other parity of B;
//                        and leaves per row what the rest of the pass needs: the block row whose prediction-network state it
//                        continues (par), the appended token (tok) and the cell kernels' mask (live).  Selection is a
//                        rank-by-counting sort in LDS (rs_rank: stable, equal scores keep the list's order); equal label sequences
//                        are found by comparing lengths and tokens, one wave per pair (rs_same_labels); the only traffic that grows
//                        with T is the copy of W hypotheses' labels (rs_copy_labels).
//   eamd_rnnt_tsd_step_lm  the same pass with RNNLM shallow fusion: the record of width 1 + 3k that eamd_transducer_expand_rows
//                        writes with an LM (the raw LM log-probability of each chosen token behind the token ids) and lm_weight;
//                        the score sums follow the reference's float32 arithmetic (rnnt_search.h: rs_add / rs_ext / rs_merge).
//                        One kernel text, templated on LM.
// Hypotheses live in M + 1 blocks of n * W rows: block 0 and block M are the two parities of B, block v (1 <= v < M) is the C of pass
// v.  Block row = block * n * W + b * W + w.  Plain stores, no atomics, no scratch buffers: a workgroup owns its utterance's rows.
#include "common.h"
#include "rnnt_search.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int TS_W = 16;                       // slots per utterance at most
constexpr int TS_M = 4;                        // passes per frame at most
constexpr int TS_D = TS_W * TS_W;              // candidates of D at most: W slots x k <= W tokens
constexpr int TS_A = TS_W * TS_M;              // entries of A at most
constexpr int TS_THREADS = 256;

// LM: the record carries the k raw LM log-probabilities of the chosen tokens behind the token ids, and the score sums follow the
// float32 rule of rnnt_search.h (rs_add / rs_ext / rs_merge) with wf = (float)lm_weight; LM = false ignores wf
template <bool LM>
__global__ __launch_bounds__(TS_THREADS) void rnnt_tsd_step_kernel(
    const float* __restrict__ rec, const int* __restrict__ hlens, double* __restrict__ score, int* __restrict__ ulen,
    int* __restrict__ count, int* __restrict__ yseq, double* __restrict__ a_score, int* __restrict__ a_src, int* __restrict__ nA,
    int* __restrict__ par, long long* __restrict__ tok, unsigned char* __restrict__ live, int n, int W, int V, int T, int M, int t,
    int v, int p, float wf) {
  __shared__ double d_score[TS_D];             // candidates of D
  __shared__ double sa_score[TS_A];            // A: scores, block rows, lengths
  __shared__ double c_score[TS_W];             // C: scores, lengths
  __shared__ float s_rec[TS_W * (1 + (LM ? 3 : 2) * TS_W)];
  __shared__ int sa_src[TS_A], sa_ulen[TS_A];
  __shared__ int c_ulen[TS_W];
  __shared__ int c_new[TS_W];                  // C slot -> 1 when no entry of A holds its labels
  __shared__ int s_sel[TS_W];                  // new slot -> its candidate of D, or its entry of A
  __shared__ unsigned char s_eq[TS_W][TS_A];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = min(W, V - 1), RW = 1 + (LM ? 3 : 2) * k;
  const int ycap = 1 + T * (M - 1), AM = W * M;
  const int R = n * W, rows = (M + 1) * R;
  const int cin = v == 0 ? (p ? M : 0) : v;    // the block that holds C, the block this pass writes
  const int cout = v < M - 1 ? v + 1 : (p ? 0 : M);
  const int Tb = max(0, hlens ? min(hlens[b], T) : T);
  const int row0 = b * W;
  const int in0 = cin * R + row0, out0 = cout * R + row0;
  if (t >= Tb) {                               // the utterance is over: B waits in parity p
    const int b0 = (p ? M : 0) * R + row0;
    if (tid < W) {
      par[row0 + tid] = b0 + tid;
      tok[row0 + tid] = 0;
      live[row0 + tid] = 0;
    }
    if (v == M - 1) rs_carry_block<TS_THREADS>(score, ulen, count, yseq, ycap, W, (p ? M : 0) * n + b, cout * n + b, b0, out0, tid);
    return;
  }
  // everything the decisions need is fetched here, side by side: the stages below depend on each other, and a global load in each
  // of them would put its latency on the path once per stage (the lengths of A's entries are the one dependent load)
  const int nc = min(max(count[cin * n + b], 0), W);
  const int na0 = v == 0 ? 0 : min(max(nA[b], 0), AM - W);
  for (int x = tid; x < W * RW; x += TS_THREADS) s_rec[x] = rec[(long)row0 * RW + x];
  if (tid < W) {
    const int u = ulen[in0 + tid];
    const double sc = score[in0 + tid];
    c_ulen[tid] = tid < nc ? min(max(u, 0), ycap - 1) : 0;
    c_score[tid] = tid < nc ? sc : 0.0;
  }
  if (tid >= 64 && tid < 64 + na0) {
    const int e = tid - 64;
    const int src = min(max(a_src[(long)b * AM + e], 0), rows - 1);
    sa_src[e] = src;
    sa_score[e] = a_score[(long)b * AM + e];
    sa_ulen[e] = min(max(ulen[src], 0), ycap - 1);
  }
  __syncthreads();
  // which C slot holds the labels of which entry of A: lengths, then tokens
  for (int q = wave; q < nc * na0; q += TS_THREADS / 64) {
    const int c = q / na0, e = q - c * na0, L = c_ulen[c];
    const bool eq = L == sa_ulen[e] &&
                    rs_same_labels(yseq + (long)(in0 + c) * ycap, L, 0, yseq + (long)sa_src[e] * ycap, L, 0, L, lane);
    if (lane == 0) s_eq[c][e] = eq ? 1 : 0;
  }
  __syncthreads();
  // A: a slot of C joins the first entry that holds its labels (logaddexp, in C's order), else it is appended in C's order
  if (tid < nc) {
    int f = -1;
    for (int e = 0; e < na0 && f < 0; ++e)
      if (s_eq[tid][e]) f = e;
    c_new[tid] = f < 0;
  }
  __syncthreads();
  if (tid < na0) {
    double s = sa_score[tid];
    for (int c = 0; c < nc; ++c) {
      bool mine = s_eq[c][tid] != 0;
      for (int e = 0; e < tid && mine; ++e) mine = !s_eq[c][e];
      if (mine) s = rs_merge<LM>(s, rs_add<LM>(c_score[c], c_ulen[c], s_rec[c * RW]), c_ulen[c]);
    }
    sa_score[tid] = s;
  } else if (tid >= 64 && tid < 64 + nc) {
    const int c = tid - 64;
    if (c_new[c]) {
      int pos = na0;
      for (int o = 0; o < c; ++o) pos += c_new[o];
      sa_score[pos] = rs_add<LM>(c_score[c], c_ulen[c], s_rec[c * RW]);
      sa_src[pos] = in0 + c;
      sa_ulen[pos] = c_ulen[c];
    }
  }
  __syncthreads();
  int na = na0;
  for (int c = 0; c < nc; ++c) na += c_new[c];
  if (tid < na) {
    a_score[(long)b * AM + tid] = sa_score[tid];
    a_src[(long)b * AM + tid] = sa_src[tid];
  }
  if (tid == 0) nA[b] = na;
  if (v < M - 1) {
    // D: per slot of C its k extensions in the record's order; the first W of sorted(D, reverse=True) are the next C
    const int nd = nc * k;
    for (int c = tid; c < nd; c += TS_THREADS) {
      const int w = c / k, j = c - w * k;
      d_score[c] = rs_ext<LM>(c_score[w], c_ulen[w], s_rec[w * RW + 1 + j], LM ? s_rec[w * RW + 1 + 2 * k + j] : 0.f, wf);
    }
    __syncthreads();
    for (int c = tid; c < nd; c += TS_THREADS) {
      const int cnt = rs_rank(d_score, nd, c);
      if (cnt < W) s_sel[cnt] = c;
    }
    __syncthreads();
    const int nn = min(W, nd);
    if (tid == 0) count[cout * n + b] = nn;
    if (tid < W) {
      const int r = row0 + tid;
      if (tid < nn) {
        const int c = s_sel[tid], w = c / k, j = c - w * k;
        score[out0 + tid] = d_score[c];
        ulen[out0 + tid] = min(c_ulen[w] + 1, ycap - 1);
        par[r] = in0 + w;
        tok[r] = min(max((int)s_rec[w * RW + 1 + k + j], 0), V - 1);
        live[r] = 1;
      } else {
        par[r] = in0 + tid;
        tok[r] = 0;
        live[r] = 0;
      }
    }
    rs_copy_labels<TS_THREADS>(nn, ycap, tid, [&](int m) {
      const int c = s_sel[m], w = c / k, j = c - w * k;
      return RsLabels{yseq + (long)(out0 + m) * ycap, yseq + (long)(in0 + w) * ycap, c_ulen[w], min(c_ulen[w] + 1, ycap - 1),
                      min(max((int)s_rec[w * RW + 1 + k + j], 0), V - 1)};
    });
    return;
  }
  // the frame's end: the first W of sorted(A, reverse=True) are the next B
  if (tid < na) {
    const int cnt = rs_rank(sa_score, na, tid);
    if (cnt < W) s_sel[cnt] = tid;
  }
  __syncthreads();
  const int nn = min(W, na);
  if (tid == 0) count[cout * n + b] = nn;
  if (tid < W) {
    const int r = row0 + tid;
    if (tid < nn) {
      const int e = s_sel[tid];
      score[out0 + tid] = sa_score[e];
      ulen[out0 + tid] = sa_ulen[e];
      par[r] = sa_src[e];
    } else {
      par[r] = in0 + tid;
    }
    tok[r] = 0;
    live[r] = 0;
  }
  rs_copy_labels<TS_THREADS>(nn, ycap, tid, [&](int m) {
    const int a = s_sel[m];
    return RsLabels{yseq + (long)(out0 + m) * ycap, yseq + (long)sa_src[a] * ycap, sa_ulen[a], sa_ulen[a], 0};
  });
}

int tsd_launch(bool lm, float lm_weight, const float* rec, const int32_t* hlens, double* score, int32_t* ulen, int32_t* count,
               int32_t* yseq, double* a_score, int32_t* a_src, int32_t* nA, int32_t* par, int64_t* tok, uint8_t* live, int n, int W,
               int V, int T, int M, int t, int v, int p, void* stream) {
  if (!rec || !score || !ulen || !count || !yseq || !a_score || !a_src || !nA || !par || !tok || !live) return EAMD_EINVAL;
  if (n < 1 || W < 1 || V < 2 || T < 1 || t < 0 || v < 0 || (M >= 1 && v >= M) || (p != 0 && p != 1)) return EAMD_EINVAL;
  if (lm_weight != lm_weight || lm_weight - lm_weight != 0.f) return EAMD_EINVAL;            // NaN or infinite
  // one array handed in for two operands: a workgroup's stores would meet its own loads.  (The block a pass reads and the block it
  // writes are told apart by (v, p) inside one allocation, so they cannot be the same.)
  const void* const ints[] = {ulen, count, yseq, a_src, nA, par};
  if (!rs_distinct(ints) || score == a_score) return EAMD_EINVAL;
  if (W > TS_W || W > V || M < 1 || M > TS_M) return EAMD_EUNSUPPORTED;
  if ((int64_t)(M + 1) * n * W > 0x7fffffff || (int64_t)n * T > 0x7fffffff || 1 + (int64_t)T * (M - 1) > 0x7fffffff / TS_W)
    return EAMD_EUNSUPPORTED;
  const auto kernel = lm ? rnnt_tsd_step_kernel<true> : rnnt_tsd_step_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(n), dim3(TS_THREADS), 0, (hipStream_t)stream, rec, hlens, score, ulen, count, yseq, a_score, a_src,
                     nA, par, reinterpret_cast<long long*>(tok), live, n, W, V, T, M, t, v, p, lm_weight);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // namespace

extern "C" {

int eamd_rnnt_tsd_step(const float* rec, const int32_t* hlens, double* score, int32_t* ulen, int32_t* count, int32_t* yseq,
                       double* a_score, int32_t* a_src, int32_t* nA, int32_t* par, int64_t* tok, uint8_t* live, int n, int W, int V,
                       int T, int M, int t, int v, int p, void* stream) {
  return tsd_launch(false, 0.f, rec, hlens, score, ulen, count, yseq, a_score, a_src, nA, par, tok, live, n, W, V, T, M, t, v, p,
                    stream);
}

int eamd_rnnt_tsd_step_lm(const float* rec, const int32_t* hlens, double* score, int32_t* ulen, int32_t* count, int32_t* yseq,
                          double* a_score, int32_t* a_src, int32_t* nA, int32_t* par, int64_t* tok, uint8_t* live, int n, int W, int V,
                          int T, int M, int t, int v, int p, float lm_weight, void* stream) {
  return tsd_launch(true, lm_weight, rec, hlens, score, ulen, count, yseq, a_score, a_src, nA, par, tok, live, n, W, V, T, M, t, v, p,
                    stream);
}

}  // extern "C"
