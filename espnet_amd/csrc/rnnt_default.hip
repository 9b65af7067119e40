// Batched default (Graves A / B) transducer beam search: the bookkeeping of one POP for n utterances in one launch.
// reference: espnet/nets/beam_search_transducer.py:163-237 (default_beam_search without an LM).  The search pops the best entry of
// A until W entries of B beat everything left in A, so the pops of a frame depend on the data; the utterances of a batch advance
// in lock-step in pops, and every utterance keeps its own frame counter on the device.
//
//   eamd_rnnt_default_step   one workgroup per utterance.  It FINISHES the pending pop from eamd_transducer_expand_rows' record of
//                            the popped entry's joint row - k children into A, the blank continuation into B, A cut to its P best,
//                            bound = max(A), the entries of B ahead of it counted and, when there are W of them, ranked and moved
//                            into the next frame's A - and SELECTS the next pop, for which it leaves the pool row to read (par), the
//                            token (tok), the pool row to write (dst), the cell kernels' mask (live), the encoder row (frame) and
//                            the scatter's mask (alive).  A is kept sorted by (score descending, insertion order ascending): the
//                            reference's first maximum in list order is entry 0, and cutting A is a cut of the ranks.  Ranks come
//                            from counting in LDS with rs_key's order (A's tie is the insertion order, and B's two orders come
//                            from one pass, so the loops stay here).  Labels are not kept: every pop appends one (parent record,
//                            token) pair to the utterance's log, from which the host rebuilds the sequences.
// The new prediction-network state of every layer goes into the pool rows the step kernel named by eamd_scatter_rows
// (row_moves.hip).  Plain stores, no atomics: a workgroup owns its utterance's rows of every array.
#include "common.h"
#include "rnnt_search.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int DF_W = 16;                       // beam at most
constexpr int DF_P = 256;                      // pops per frame, entries of A and of B at most
constexpr int DF_A = DF_P + DF_W;              // A before the cut: P kept entries (one of them popped) + k <= W children
constexpr int DF_THREADS = 256;
// columns of ctr [n][8]
constexpr int DC_T = 0, DC_POPS = 1, DC_NA = 2, DC_NB = 3, DC_NLOG = 4, DC_SEQ = 5, DC_CUR = 6, DC_MAXPOPS = 7;

__global__ __launch_bounds__(DF_THREADS) void rnnt_default_step_kernel(
    const float* __restrict__ rec, const int* __restrict__ hlens, double* __restrict__ a_score, int* __restrict__ a_seq,
    int* __restrict__ a_row, int* __restrict__ a_log, int* __restrict__ a_tok, double* __restrict__ b_score, int* __restrict__ b_row,
    int* __restrict__ b_log, double* __restrict__ cur_score, int* __restrict__ ctr, int* __restrict__ log, int* __restrict__ flags,
    int* __restrict__ par, long long* __restrict__ tok, int* __restrict__ dst, unsigned char* __restrict__ live,
    int* __restrict__ frame, unsigned char* __restrict__ alive, int n, int W, int V, int T, int P, int k, int log_cap) {
  __shared__ double sa_score[DF_A], sb_score[DF_P];
  __shared__ int sa_seq[DF_A], sa_row[DF_A], sa_log[DF_A], sa_tok[DF_A], sa_pos[DF_A];
  __shared__ int sb_row[DF_P], sb_log[DF_P];
  __shared__ unsigned char sb_ahead[DF_P];
  __shared__ float s_rec[1 + 2 * DF_W];
  __shared__ double s_bound, s_pop_score;
  __shared__ int s_pop_row, s_pop_log, s_pop_tok;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = min(max(hlens ? hlens[b] : T, 0), T);
  int* c = ctr + (long)b * 8;
  const int base = b * 2 * P;
  const int t = c[DC_T];
  if (flags[b] != 0 || flags[n + b] != 0 || t < 0 || t >= Tb) {      // finished or overflowed: the state stays as it is
    if (tid == 0) {
      par[b] = base;
      tok[b] = 0;
      dst[b] = base;
      live[b] = 0;
      frame[b] = b * T;
      alive[b] = 0;
    }
    return;
  }
  const int pops = min(max(c[DC_POPS], 1), P);
  int nA = min(max(c[DC_NA], 0), P);
  int nB = min(max(c[DC_NB], 0), P - 1);
  const int nlog = min(max(c[DC_NLOG], 1), log_cap);
  const int seqc = c[DC_SEQ];
  const int cur = min(max(c[DC_CUR], 0), nlog - 1);
  const int cur_row = (t & 1) * P + pops - 1;              // the pool row the pending pop's state was written to
  const double s = cur_score[b];
  const long a0 = (long)b * P;
  for (int x = tid; x < nA; x += DF_THREADS) {
    sa_score[x] = a_score[a0 + x];
    sa_seq[x] = a_seq[a0 + x];
    sa_row[x] = a_row[a0 + x];
    sa_log[x] = a_log[a0 + x];
    sa_tok[x] = a_tok[a0 + x];
  }
  for (int x = tid; x < nB; x += DF_THREADS) {
    sb_score[x] = b_score[a0 + x];
    sb_row[x] = b_row[a0 + x];
    sb_log[x] = b_log[a0 + x];
  }
  if (tid < 1 + 2 * k) s_rec[tid] = rec[(long)b * (1 + 2 * k) + tid];
  __syncthreads();
  // finish the pop: the k children in the record's order, the blank continuation
  if (tid < k) {
    sa_score[nA + tid] = s + (double)s_rec[1 + tid];
    sa_seq[nA + tid] = seqc + tid;
    sa_row[nA + tid] = cur_row;
    sa_log[nA + tid] = cur;
    sa_tok[nA + tid] = min(max((int)s_rec[1 + k + tid], 1), V - 1);
  }
  if (tid == DF_THREADS - 1) {
    sb_score[nB] = s + (double)s_rec[0];
    sb_row[nB] = cur_row;
    sb_log[nB] = cur;
    b_score[a0 + nB] = sb_score[nB];
    b_row[a0 + nB] = cur_row;
    b_log[a0 + nB] = cur;
  }
  nA += k;
  nB += 1;
  __syncthreads();
  // position in A: entries ahead (larger score, or equal score and earlier insertion); entry 0 is max(A), the first one in list order
  for (int x = tid; x < nA; x += DF_THREADS) {
    const double key = rs_key(sa_score[x]);
    const int sq = sa_seq[x];
    int cnt = 0;
    for (int o = 0; o < nA; ++o) {
      const double ok = rs_key(sa_score[o]);
      cnt += (ok > key || (ok == key && sa_seq[o] < sq)) ? 1 : 0;
    }
    sa_pos[x] = cnt;
    if (cnt == 0) s_bound = key;
  }
  __syncthreads();
  const double bound = s_bound;
  const bool mine = tid < nB && rs_key(sb_score[tid]) > bound;          // nB <= P <= DF_THREADS: one entry of B per thread
  if (tid < nB) sb_ahead[tid] = mine ? 1 : 0;
  const int nahead = __syncthreads_count(mine ? 1 : 0);
  const bool turn = nahead >= W;                                        // the frame ends
  const int t1 = turn ? t + 1 : t;
  if (turn && t1 >= Tb) {
    // the last frame: B = ahead in its stable ascending order, the list the reference sorts into the n-best
    if (mine) {
      const double key = rs_key(sb_score[tid]);
      int rank = 0;
      for (int o = 0; o < nB; ++o) {
        const double ok = rs_key(sb_score[o]);
        rank += (sb_ahead[o] && (ok < key || (ok == key && o < tid))) ? 1 : 0;
      }
      b_score[a0 + rank] = sb_score[tid];
      b_row[a0 + rank] = sb_row[tid];
      b_log[a0 + rank] = sb_log[tid];
    }
    if (tid == 0) {
      c[DC_T] = t1;
      c[DC_POPS] = 0;
      c[DC_NA] = 0;
      c[DC_NB] = nahead;
      c[DC_SEQ] = nahead;
      c[DC_MAXPOPS] = max(c[DC_MAXPOPS], pops);
      flags[b] = 1;
      par[b] = base;
      tok[b] = 0;
      dst[b] = base;
      live[b] = 0;
      frame[b] = b * T;
      alive[b] = 0;
    }
    return;
  }
  // select the next pop: entry 0 of the new A, unless the frame has had its P pops or the log is full
  const int pops0 = turn ? 0 : pops;
  const bool pop = pops0 < P && nlog < log_cap;
  const int shift = pop ? 1 : 0;
  if (turn) {
    if (mine) {
      const double key = rs_key(sb_score[tid]);
      int rank = 0, pos = 0;                                            // both orders from one pass over B
      for (int o = 0; o < nB; ++o) {
        if (!sb_ahead[o]) continue;
        const double ok = rs_key(sb_score[o]);
        rank += (ok < key || (ok == key && o < tid)) ? 1 : 0;
        pos += (ok > key || (ok == key && o < tid)) ? 1 : 0;
      }
      if (pos == 0 && pop) {
        s_pop_score = sb_score[tid];
        s_pop_row = sb_row[tid];
        s_pop_log = sb_log[tid];
        s_pop_tok = 0;
      } else {
        const long q = a0 + pos - shift;
        a_score[q] = sb_score[tid];
        a_seq[q] = rank;
        a_row[q] = sb_row[tid];
        a_log[q] = sb_log[tid];
        a_tok[q] = 0;
      }
    }
  } else {
    for (int x = tid; x < nA; x += DF_THREADS) {
      const int pos = sa_pos[x];
      if (pos >= P) continue;                                          // the cut: it cannot be popped within this frame's P pops
      if (pos == 0 && pop) {
        s_pop_score = sa_score[x];
        s_pop_row = sa_row[x];
        s_pop_log = sa_log[x];
        s_pop_tok = sa_tok[x];
      } else {
        const long q = a0 + pos - shift;
        a_score[q] = sa_score[x];
        a_seq[q] = sa_seq[x];
        a_row[q] = sa_row[x];
        a_log[q] = sa_log[x];
        a_tok[q] = sa_tok[x];
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int kept = turn ? nahead : min(nA, P);
    c[DC_T] = t1;
    c[DC_NA] = kept - shift;
    c[DC_NB] = turn ? 0 : nB;
    c[DC_SEQ] = turn ? nahead : seqc + k;
    if (turn) c[DC_MAXPOPS] = max(c[DC_MAXPOPS], pops);
    if (pop) {
      c[DC_POPS] = pops0 + 1;
      c[DC_NLOG] = nlog + 1;
      c[DC_CUR] = nlog;
      log[((long)b * log_cap + nlog) * 2] = s_pop_log;
      log[((long)b * log_cap + nlog) * 2 + 1] = s_pop_tok;
      cur_score[b] = s_pop_score;
      par[b] = base + min(max(s_pop_row, 0), 2 * P - 1);
      tok[b] = min(max(s_pop_tok, 0), V - 1);
      dst[b] = base + (t1 & 1) * P + pops0;
      live[b] = s_pop_tok > 0 ? 1 : 0;
      frame[b] = b * T + t1;
      alive[b] = 1;
    } else {
      c[DC_POPS] = pops0;
      flags[n + b] = 1;
      par[b] = base;
      tok[b] = 0;
      dst[b] = base;
      live[b] = 0;
      frame[b] = b * T;
      alive[b] = 0;
    }
  }
}

}  // namespace

extern "C" {

int eamd_rnnt_default_step(const float* rec, const int32_t* hlens, double* a_score, int32_t* a_seq, int32_t* a_row, int32_t* a_log,
                           int32_t* a_tok, double* b_score, int32_t* b_row, int32_t* b_log, double* cur_score, int32_t* ctr,
                           int32_t* log, int32_t* flags, int32_t* par, int64_t* tok, int32_t* dst, uint8_t* live, int32_t* frame,
                           uint8_t* alive, int n, int W, int V, int T, int P, int k, int log_cap, void* stream) {
  if (!rec || !a_score || !a_seq || !a_row || !a_log || !a_tok || !b_score || !b_row || !b_log || !cur_score || !ctr || !log ||
      !flags || !par || !tok || !dst || !live || !frame || !alive)
    return EAMD_EINVAL;
  if (n < 1 || W < 1 || V < 2 || T < 1 || P < 1 || log_cap < 1) return EAMD_EINVAL;
  if (W > DF_W || W > V || P > DF_P || P < W) return EAMD_EUNSUPPORTED;
  if (k != (W < V - 1 ? W : V - 1)) return EAMD_EINVAL;
  if ((int64_t)n * T > 0x7fffffff || (int64_t)n * 2 * P > 0x7fffffff) return EAMD_EUNSUPPORTED;
  hipLaunchKernelGGL(rnnt_default_step_kernel, dim3(n), dim3(DF_THREADS), 0, (hipStream_t)stream, rec, hlens, a_score, a_seq, a_row,
                     a_log, a_tok, b_score, b_row, b_log, cur_score, ctr, log, flags, par, reinterpret_cast<long long*>(tok), dst, live,
                     frame, alive, n, W, V, T, P, k, log_cap);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
