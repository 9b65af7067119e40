// Batched alignment-length-synchronous transducer beam search: the beam bookkeeping of one step for n utterances in one launch.
// reference: espnet/nets/beam_search_transducer.py:349-464 (align_length_sync_decoding without an LM), transducer/utils.py:181-203
// (recombine_hyps).  Every hypothesis consumes one (frame, label prefix) pair per step, so the utterances of a batch advance in
// lock-step; what the reference does with Python lists per utterance - build A from the active hypotheses, sort it, keep `beam`,
// recombine equal label sequences, collect the hypotheses that reached the last frame - is done here by one workgroup per
// utterance on W <= 16 slots and at most 16 * 17 = 272 candidates.
//
//   eamd_rnnt_alsd_step   reads eamd_transducer_expand_rows' record of the step's n * W rows and the state of one parity, writes
//                         the state of the other parity, appends the finals, and leaves per row what the rest of the step needs:
//                         the row whose prediction-network state it continues (par), the appended token (tok), the cell kernels'
//                         mask (live) and the encoder row of the next step (frame).  Selection is a rank-by-counting sort in LDS
//                         (rs_rank: stable, equal scores keep A's order); equal label sequences are found by comparing lengths
//                         and tokens, one wave per pair (rs_same_labels); the only traffic that grows with T is the copy of W
//                         parents' labels (rs_copy_labels).
//   eamd_rnnt_alsd_step_lm  the same step with RNNLM shallow fusion: the record of width 1 + 3k that eamd_transducer_expand_rows
//                         writes with an LM (the raw LM log-probability of each chosen token behind the token ids) and lm_weight;
//                         the score sums follow the reference's float32 arithmetic (rnnt_search.h: rs_add / rs_ext / rs_merge).
//                         One kernel text, templated on LM.
// The rows the rest of the step needs are moved by eamd_gather_rows (row_moves.hip).  Plain stores, no atomics, no scratch
// buffers: a workgroup owns its utterance's rows of every output.
#include "common.h"
#include "rnnt_search.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int AL_W = 16;                       // slots per utterance at most
constexpr int AL_C = AL_W * (AL_W + 1);        // candidates per utterance at most: W active slots x (blank + k <= W tokens)
constexpr int AL_THREADS = 256;

// LM: the record carries the k raw LM log-probabilities of the chosen tokens behind the token ids, and the score sums follow the
// float32 rule of rnnt_search.h (rs_add / rs_ext / rs_merge) with wf = (float)lm_weight; LM = false ignores wf
template <bool LM>
__global__ __launch_bounds__(AL_THREADS) void rnnt_alsd_step_kernel(
    const float* __restrict__ rec, const int* __restrict__ hlens, const double* __restrict__ score_in, const int* __restrict__ ulen_in,
    const int* __restrict__ nhyp_in, const int* __restrict__ yseq_in, double* __restrict__ score_out, int* __restrict__ ulen_out,
    int* __restrict__ nhyp_out, int* __restrict__ yseq_out, double* __restrict__ fin_score, int* __restrict__ fin_len,
    int* __restrict__ fin_yseq, int* __restrict__ nfin, int* __restrict__ par, long long* __restrict__ tok,
    unsigned char* __restrict__ live, int* __restrict__ frame, int W, int V, int T, int u_max, int i, float wf) {
  __shared__ double c_score[AL_C];             // candidates of A, raw scores
  __shared__ double s_score[AL_W];             // the new B: scores (first occurrences grow in the recombination)
  __shared__ int c_rank[AL_C];
  __shared__ int s_cand[AL_W], s_first[AL_W];  // new slot -> its candidate, -> the slot of its sequence's first occurrence
  __shared__ int a_slot[AL_W];                 // active slots in slot order
  __shared__ int o_ulen[AL_W];                 // labels of the old slots
  __shared__ int n_ulen[AL_W], n_src[AL_W], n_tok[AL_W], n_live[AL_W];
  __shared__ int f_slot[AL_W], f_pos[AL_W];    // finals of this step: old slot, position in the final list
  __shared__ unsigned char s_eq[AL_W][AL_W];
  __shared__ float s_rec[AL_W * (1 + (LM ? 3 : 2) * AL_W)];             // the utterance's rows of the record
  __shared__ double o_score[AL_W];
  __shared__ int s_nact, s_nf, s_nfin0;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = min(W, V - 1), RW = 1 + (LM ? 3 : 2) * k, K1 = k + 1;
  const int ycap = T + u_max + 1, fw = u_max + 2, fcap = W * fw;
  const int Tb = max(0, hlens ? min(hlens[b], T) : T);
  const int umb = min(u_max, Tb - 1);
  const int tmax = max(Tb - 1, 0);
  const int nh = min(max(nhyp_in[b], 0), W);
  const bool over = i >= Tb + umb;
  const long row0 = (long)b * W;
  // everything the decisions need is fetched here, side by side: the stages below depend on each other, and a global load in
  // each of them would put its latency on the path once per stage
  for (int x = tid; x < W * RW; x += AL_THREADS) s_rec[x] = rec[row0 * RW + x];
  if (tid < W) {
    const int u = ulen_in[row0 + tid];
    const double sc = score_in[row0 + tid];
    o_ulen[tid] = tid < nh ? min(max(u, 0), ycap - 1) : 0;
    o_score[tid] = tid < nh ? sc : 0.0;
  }
  if (tid == 0) s_nfin0 = nfin[b];
  __syncthreads();
  if (tid == 0) {
    int na = 0;
    if (!over)
      for (int w = 0; w < nh; ++w)
        if (i - o_ulen[w] + 1 <= Tb - 1) a_slot[na++] = w;      // t = i - u + 1 >= 1: frame 0 is never scored
    s_nact = na;
  }
  __syncthreads();
  const int nact = s_nact;
  if (nact == 0) {                             // utterance over, or the reference's `if B_:` - B is carried unchanged
    if (tid < W) {
      const long r = row0 + tid;
      score_out[r] = o_score[tid];
      ulen_out[r] = o_ulen[tid];
      par[r] = (int)r;
      tok[r] = 0;
      live[r] = 0;
      frame[r] = b * T + min(max(i + 2 - o_ulen[tid], 0), tmax);
    }
    if (tid == 0) nhyp_out[b] = nh;
    rs_copy_labels<AL_THREADS>(nh, ycap, tid, [&](int w) {
      return RsLabels{yseq_out + (row0 + w) * ycap, yseq_in + (row0 + w) * ycap, o_ulen[w], o_ulen[w], 0};
    });
    return;
  }
  // A: per active slot its blank continuation, then its k extensions in the record's order
  const int C = nact * K1;
  for (int c = tid; c < C; c += AL_THREADS) {
    const int a = c / K1, j = c - a * K1;
    const int w = a_slot[a];
    c_score[c] = j == 0 ? rs_add<LM>(o_score[w], o_ulen[w], s_rec[w * RW])
                        : rs_ext<LM>(o_score[w], o_ulen[w], s_rec[w * RW + j], LM ? s_rec[w * RW + 2 * k + j] : 0.f, wf);
  }
  __syncthreads();
  // sorted(A, reverse=True)[:W]: position = candidates ahead (larger score, or equal score and earlier in A)
  for (int c = tid; c < C; c += AL_THREADS) {
    const int cnt = rs_rank(c_score, C, c);
    c_rank[c] = cnt;
    if (cnt < W) s_cand[cnt] = c;
  }
  __syncthreads();
  const int nn = min(W, C);
  if (tid < nn) {
    const int c = s_cand[tid], a = c / K1, j = c - a * K1, w = a_slot[a];
    n_src[tid] = w;
    n_live[tid] = j > 0;
    n_tok[tid] = j > 0 ? min(max((int)s_rec[w * RW + k + j], 0), V - 1) : 0;
    n_ulen[tid] = o_ulen[w] + (j > 0 ? 1 : 0);
    s_score[tid] = c_score[c];
  }
  __syncthreads();
  // equal label sequences among the new slots: lengths, then tokens (element e of new slot m: the parent's label, or the new token)
  for (int p = wave; p < nn * nn; p += AL_THREADS / 64) {
    const int m2 = p / nn, m1 = p - m2 * nn;
    if (m1 >= m2) continue;
    const int w1 = n_src[m1], w2 = n_src[m2];
    const bool eq = n_ulen[m1] == n_ulen[m2] &&
                    rs_same_labels(yseq_in + (row0 + w1) * ycap, o_ulen[w1], n_tok[m1], yseq_in + (row0 + w2) * ycap, o_ulen[w2],
                                   n_tok[m2], min(n_ulen[m1], ycap - 1), lane);
    if (lane == 0) s_eq[m2][m1] = eq ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0) {
    // recombine_hyps as it behaves: a later equal sequence adds its score to the first occurrence and stays as it is
    for (int m = 0; m < nn; ++m) {
      int f = m;
      for (int m1 = 0; m1 < m; ++m1)
        if (s_eq[m][m1]) { f = m1; break; }
      s_first[m] = f;
      if (f != m) s_score[f] = rs_merge<LM>(s_score[f], s_score[m], n_ulen[m]);
    }
    // finals: the blank continuations of the slots on the last frame, in slot order
    int nf = min(max(s_nfin0, 0), fcap), q = 0;
    for (int a = 0; a < nact; ++a) {
      const int w = a_slot[a];
      if (i - o_ulen[w] + 1 != Tb - 1) continue;
      const int c = a * K1, rk = c_rank[c];
      if (nf < fcap) {
        fin_score[(long)b * fcap + nf] = (rk < nn && s_first[rk] == rk) ? s_score[rk] : c_score[c];
        fin_len[(long)b * fcap + nf] = min(o_ulen[w] + 1, fw);
        f_slot[q] = w;
        f_pos[q] = nf;
        ++q;
        ++nf;
      }
    }
    nfin[b] = nf;
    s_nf = q;
  }
  __syncthreads();
  if (tid < W) {
    const long r = row0 + tid;
    if (tid < nn) {
      const int u = min(n_ulen[tid], ycap - 1);
      score_out[r] = s_score[tid];
      ulen_out[r] = u;
      par[r] = (int)(row0 + n_src[tid]);
      tok[r] = n_tok[tid];
      live[r] = n_live[tid] ? 1 : 0;
      frame[r] = b * T + min(max(i + 2 - u, 0), tmax);
    } else {
      score_out[r] = 0.0;
      ulen_out[r] = 0;
      par[r] = (int)r;
      tok[r] = 0;
      live[r] = 0;
      frame[r] = b * T + min(max(i + 2, 0), tmax);
    }
  }
  if (tid == 0) nhyp_out[b] = nn;
  rs_copy_labels<AL_THREADS>(nn, ycap, tid, [&](int m) {
    const int w = n_src[m];
    return RsLabels{yseq_out + (row0 + m) * ycap, yseq_in + (row0 + w) * ycap, o_ulen[w], n_ulen[m], n_tok[m]};
  });
  rs_copy_labels<AL_THREADS>(s_nf, fw, tid, [&](int q) {
    const int w = f_slot[q];
    return RsLabels{fin_yseq + ((long)b * fcap + f_pos[q]) * fw, yseq_in + (row0 + w) * ycap, o_ulen[w], o_ulen[w], 0};
  });
}

int alsd_launch(bool lm, float lm_weight, const float* rec, const int32_t* hlens, const double* score_in, const int32_t* ulen_in,
                const int32_t* nhyp_in, const int32_t* yseq_in, double* score_out, int32_t* ulen_out, int32_t* nhyp_out,
                int32_t* yseq_out, double* fin_score, int32_t* fin_len, int32_t* fin_yseq, int32_t* nfin, int32_t* par, int64_t* tok,
                uint8_t* live, int32_t* frame, int n, int W, int V, int T, int u_max, int i, void* stream) {
  if (!rec || !score_in || !ulen_in || !nhyp_in || !yseq_in || !score_out || !ulen_out || !nhyp_out || !yseq_out || !fin_score ||
      !fin_len || !fin_yseq || !nfin || !par || !tok || !live || !frame)
    return EAMD_EINVAL;
  if (n < 1 || W < 1 || V < 2 || T < 1 || u_max < 0 || i < 0) return EAMD_EINVAL;
  if (lm_weight != lm_weight || lm_weight - lm_weight != 0.f) return EAMD_EINVAL;            // NaN or infinite
  if (score_in == score_out || ulen_in == ulen_out || nhyp_in == nhyp_out || yseq_in == yseq_out) return EAMD_EINVAL;
  if (W > AL_W || W > V) return EAMD_EUNSUPPORTED;
  if ((int64_t)n * T > 0x7fffffff || (int64_t)T + u_max + 1 > 0x7fffffff / AL_W || (int64_t)n * W > 0x7fffffff) return EAMD_EUNSUPPORTED;
  const auto kernel = lm ? rnnt_alsd_step_kernel<true> : rnnt_alsd_step_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(n), dim3(AL_THREADS), 0, (hipStream_t)stream, rec, hlens, score_in, ulen_in, nhyp_in, yseq_in,
                     score_out, ulen_out, nhyp_out, yseq_out, fin_score, fin_len, fin_yseq, nfin, par,
                     reinterpret_cast<long long*>(tok), live, frame, W, V, T, u_max, i, lm_weight);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // namespace

extern "C" {

int eamd_rnnt_alsd_step(const float* rec, const int32_t* hlens, const double* score_in, const int32_t* ulen_in, const int32_t* nhyp_in,
                        const int32_t* yseq_in, double* score_out, int32_t* ulen_out, int32_t* nhyp_out, int32_t* yseq_out,
                        double* fin_score, int32_t* fin_len, int32_t* fin_yseq, int32_t* nfin, int32_t* par, int64_t* tok,
                        uint8_t* live, int32_t* frame, int n, int W, int V, int T, int u_max, int i, void* stream) {
  return alsd_launch(false, 0.f, rec, hlens, score_in, ulen_in, nhyp_in, yseq_in, score_out, ulen_out, nhyp_out, yseq_out, fin_score,
                     fin_len, fin_yseq, nfin, par, tok, live, frame, n, W, V, T, u_max, i, stream);
}

int eamd_rnnt_alsd_step_lm(const float* rec, const int32_t* hlens, const double* score_in, const int32_t* ulen_in,
                           const int32_t* nhyp_in, const int32_t* yseq_in, double* score_out, int32_t* ulen_out, int32_t* nhyp_out,
                           int32_t* yseq_out, double* fin_score, int32_t* fin_len, int32_t* fin_yseq, int32_t* nfin, int32_t* par,
                           int64_t* tok, uint8_t* live, int32_t* frame, int n, int W, int V, int T, int u_max, int i, float lm_weight,
                           void* stream) {
  return alsd_launch(true, lm_weight, rec, hlens, score_in, ulen_in, nhyp_in, yseq_in, score_out, ulen_out, nhyp_out, yseq_out,
                     fin_score, fin_len, fin_yseq, nfin, par, tok, live, frame, n, W, V, T, u_max, i, stream);
}

}  // extern "C"
