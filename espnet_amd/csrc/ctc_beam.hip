// Time-synchronous CTC prefix beam search (Hannun et al. 2014) with n-gram shallow fusion: the whole search of a padded batch
// in ONE launch, one workgroup per utterance, the frame loop inside the kernel (the frames are a serial chain; the utterances
// are the parallelism, as in the Viterbi alignment kernel of ctc.hip).  The reference has no such search.
//
// Beam state (LDS, two buffers that swap per frame): up to W distinct prefixes, each with a node id, its parent's node id,
// its last two tokens, its length, (pb, pnb), the raw LM sum, the LM context and that context's walk of the trie
// (ngram_query.h: computed once, when the prefix enters the beam).  A node is one (parent, token) pair of a per-utterance arena
// in the workspace; frame t hands out the ids 1 + t W + rank, so no counter and no atomics; the token strings are written by a
// backtrace at the end.
//
// Frame t, N = beam (K + 1) table entries: per prefix l one "stay" entry (l itself) and K extensions l + c, c in the frame's
// candidate list C_t (the K largest of columns 1 .. V-2, made beforehand by eamd_topk_rows_i32 for all frames at once):
//   A  per prefix j: the position of last(j) in C_t, and the beam prefix i that spells parent(j) - then the extension
//      (i, last(j)) IS j: its mass is gathered by j's stay entry and the extension's own entry is struck (at most one i per j,
//      so the merge is a gather by the receiver).  Identity is exact: len(i) + 1 == len(j), last2(j) == last(i), and
//      parent(j) == id(i) or - a prefix that left the beam and was spelled again has a second node id - the two parent chains
//      compared token by token up to their common node.  The walk (dependent global loads) is entered only when a 32-bit
//      rolling hash of parent(j)'s tokens, kept in the beam entry, equals that of i: equal strings have equal hashes, so the
//      filter drops nothing that the walk would accept, and hypotheses that differ in an early token and agree ever after
//      (the usual n-best of speech) cost a compare, not a walk back to the point where they part.
//   B  (pb', pnb') and the rank score s of every entry; a live extension asks the LM for log10 p(c | context(l)).
//   C  rank of every finite entry by counting the entries ahead of it (s larger, or equal and a lower index); rank < W moves
//      to slot `rank` of the other buffer.  Counting needs no barrier between rounds and reads the scores as LDS broadcasts
//      (16 bytes per read); N <= 1056.
// Four barriers per frame.  The candidates of frame t + 1 are loaded while frame t is worked on.
#include <math.h>

#include "common.h"
#include "ngram_query.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int kMaxW = 32, kMaxK = 32, kMaxT = 2048;
constexpr int kMaxCand = kMaxW * (kMaxK + 1);
constexpr int kCandPad = (kMaxCand + 3) & ~3;
constexpr int kMaxThreads = 1024;

struct Beam {
  int id[kMaxW], par[kMaxW], last[kMaxW], last2[kMaxW], len[kMaxW], depth[kMaxW];
  unsigned hash[kMaxW], phash[kMaxW];         // a rolling hash of the prefix's tokens and of its parent's: equal strings, equal hashes
  float pb[kMaxW], pnb[kMaxW], lm[kMaxW];
  int ctx[kMaxW][kNgramMaxCtx];
  int node[kMaxW][kNgramMaxCtx + 1];
  float acc[kMaxW][kNgramMaxCtx + 1];
};

struct BeamArgs {
  const float* logp; long ld;                 // the blank column: logp[(b T + t) ld]
  const float* cval; const int32_t* cid;      // [B, T, K]; cid counts from column 1
  const int32_t* hlens;
  int2* arena;                                // [B][T W + 1] (parent, token)
  int32_t* out;                               // [B, nbest, 2 + T]: score bits, length, tokens
  NgramQueryTables lm; int has_lm, bos;
  float lm_w, penalty;
  int T, V, W, K, nbest;
};

__device__ __forceinline__ float lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (!(m > -INFINITY)) return -INFINITY;
  return m + log1pf(expf(-fabsf(a - b)));
}

// do the nodes a and b (of equal depth) spell the same string?  Walks both parent chains until they meet.
__device__ __forceinline__ bool same_string(const int2* __restrict__ arena, int a, int b) {
  while (a != b) {
    if (a <= 0 || b <= 0) return false;
    const int2 ea = arena[a], eb = arena[b];
    if (ea.y != eb.y) return false;
    a = ea.x;
    b = eb.x;
  }
  return true;
}

// entries ahead of (s, e) among score[0 .. n4) (n4 % 4 == 0, padded with -inf)
__device__ __forceinline__ int rank_of(const float* score, int n4, float s, int e) {
  int r = 0;
  for (int f = 0; f < n4; f += 4) {
    const f32x4 v = *(const f32x4*)(score + f);
    r += (v.x > s || (v.x == s && f < e)) + (v.y > s || (v.y == s && f + 1 < e)) + (v.z > s || (v.z == s && f + 2 < e)) +
         (v.w > s || (v.w == s && f + 3 < e));
  }
  return r;
}

__global__ __launch_bounds__(kMaxThreads) void ctc_prefix_beam_kernel(BeamArgs a) {
  __shared__ Beam s_beam[2];
  __shared__ __attribute__((aligned(16))) float s_score[kCandPad];
  __shared__ float s_cpb[kMaxCand], s_cpnb[kMaxCand], s_clm[kMaxCand];
  __shared__ float s_cv[2][kMaxK];
  __shared__ int s_ci[2][kMaxK];
  __shared__ float s_blank[2];
  __shared__ int s_kpos[kMaxW], s_src[kMaxW];
  __shared__ unsigned char s_merged[kMaxW * kMaxK];
  __shared__ int s_nb[2];

  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int T = a.T, W = a.W, K = a.K, K1 = a.K + 1, C = a.lm.C;
  int Tb = a.hlens[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  int2* __restrict__ arena = a.arena + (long)b * ((long)T * W + 1);
  const float* __restrict__ cval = a.cval + (long)b * T * K;
  const int32_t* __restrict__ cid = a.cid + (long)b * T * K;
  const float* __restrict__ blank = a.logp + (long)b * T * a.ld;

  if (tid == 0) {
    Beam& B0 = s_beam[0];
    B0.id[0] = 0; B0.par[0] = -1; B0.last[0] = -1; B0.last2[0] = -1; B0.len[0] = 0;
    B0.hash[0] = 0x9E3779B9u; B0.phash[0] = 0u;
    B0.pb[0] = 0.f; B0.pnb[0] = -INFINITY; B0.lm[0] = 0.f; B0.depth[0] = 0;
    for (int i = 0; i < kNgramMaxCtx; ++i) B0.ctx[0][i] = (i == 0 && a.has_lm) ? a.bos : -1;
    for (int i = 0; i <= kNgramMaxCtx; ++i) { B0.node[0][i] = 0; B0.acc[0][i] = 0.f; }
    if (a.has_lm) B0.depth[0] = ngram_walk(a.lm, B0.ctx[0], B0.node[0], B0.acc[0]);
    arena[0] = make_int2(-1, -1);
    s_nb[0] = 1;
    s_nb[1] = 0;
  }
  // this lane's share of the next frame's candidates: lanes 0 .. K-1 one (value, id) each, lane K the blank
  float pv = 0.f;
  int pi = 0;
  if (Tb > 0) {
    if (tid < K) { pv = cval[tid]; pi = cid[tid] + 1; }
    else if (tid == K) pv = blank[0];
    if (tid < K) { s_cv[0][tid] = pv; s_ci[0][tid] = pi; }
    else if (tid == K) s_blank[0] = pv;
  }
  __syncthreads();

  for (int t = 0; t < Tb; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    const Beam& P = s_beam[cur];
    Beam& Q = s_beam[nxt];
    const int nb = s_nb[cur];
    const int N = nb * K1, N4 = (N + 3) & ~3;
    const float* cv = s_cv[cur];
    const int* ci = s_ci[cur];
    const float lpb = s_blank[cur];
    if (t + 1 < Tb) {                                   // in flight until the end of this frame
      if (tid < K) { pv = cval[(long)(t + 1) * K + tid]; pi = cid[(long)(t + 1) * K + tid] + 1; }
      else if (tid == K) pv = blank[(long)(t + 1) * a.ld];
    }

    // ---- A1: where last(j) stands in C_t; clear the merge tables
    if (tid < nb) {
      int kp = -1;
      const int lt = P.last[tid];
      for (int k = 0; k < K; ++k)
        if (ci[k] == lt) kp = k;
      s_kpos[tid] = kp;
      s_src[tid] = -1;
    }
    for (int e = tid; e < nb * K; e += nthr) s_merged[e] = 0;
    __syncthreads();

    // ---- A2: the beam prefix i that spells parent(j)
    for (int p = tid; p < nb * nb; p += nthr) {
      const int j = p / nb, i = p - j * nb;
      if (s_kpos[j] >= 0 && P.len[i] + 1 == P.len[j] && P.last2[j] == P.last[i] && P.phash[j] == P.hash[i]) {
        const int pj = P.par[j];
        if (pj == P.id[i] || (P.len[i] > 0 && pj > 0 && same_string(arena, arena[pj].x, P.par[i]))) {
          s_src[j] = i;
          s_merged[i * K + s_kpos[j]] = 1;
        }
      }
    }
    __syncthreads();

    // ---- B: the table of the new frame
    for (int e = tid; e < N4; e += nthr) {
      if (e >= N) { s_score[e] = -INFINITY; continue; }
      const int i = e / K1, k = e - i * K1;
      const float pb = P.pb[i], pnb = P.pnb[i], tot = lae(pb, pnb);
      float npb = -INFINITY, npnb = -INFINITY, lmv = P.lm[i];
      int len = P.len[i];
      if (k == 0) {
        npb = tot + lpb;
        const int kp = s_kpos[i];
        if (kp >= 0) {
          const float lpc = cv[kp];
          npnb = pnb + lpc;
          const int q = s_src[i];
          if (q >= 0) {
            const float qpb = P.pb[q];
            npnb = lae(npnb, (P.last[q] == P.last[i] ? qpb : lae(qpb, P.pnb[q])) + lpc);
          }
        }
      } else {
        const int c = ci[k - 1];
        len += 1;
        if (!s_merged[i * K + k - 1]) npnb = (c == P.last[i] ? pb : tot) + cv[k - 1];
        if (a.has_lm && npnb > -INFINITY) lmv += ngram_point(a.lm, P.depth[i], P.node[i], P.acc[i], c);
      }
      const float ntot = lae(npb, npnb);
      float s = ntot + a.lm_w * lmv + a.penalty * (float)len;
      if (!(ntot > -INFINITY) || !(s > -INFINITY)) s = -INFINITY;
      s_score[e] = s;
      s_cpb[e] = npb; s_cpnb[e] = npnb; s_clm[e] = lmv;
    }
    if (tid == 0) s_nb[nxt] = 0;
    __syncthreads();

    // ---- C: rank by counting; the W best move to the other buffer
    for (int e = tid; e < N; e += nthr) {
      const float s = s_score[e];
      if (!(s > -INFINITY)) continue;
      const int r = rank_of(s_score, N4, s, e);
      if (r >= W) continue;
      atomicMax(&s_nb[nxt], r + 1);
      const int i = e / K1, k = e - i * K1;
      Q.pb[r] = s_cpb[e]; Q.pnb[r] = s_cpnb[e]; Q.lm[r] = s_clm[e];
      if (k == 0) {
        Q.id[r] = P.id[i]; Q.par[r] = P.par[i]; Q.last[r] = P.last[i]; Q.last2[r] = P.last2[i]; Q.len[r] = P.len[i];
        Q.depth[r] = P.depth[i]; Q.hash[r] = P.hash[i]; Q.phash[r] = P.phash[i];
        if (a.has_lm) {
#pragma unroll
          for (int x = 0; x < kNgramMaxCtx; ++x) Q.ctx[r][x] = P.ctx[i][x];
#pragma unroll
          for (int x = 0; x <= kNgramMaxCtx; ++x) { Q.node[r][x] = P.node[i][x]; Q.acc[r][x] = P.acc[i][x]; }
        }
      } else {
        const int c = ci[k - 1];
        const int id = 1 + t * W + r;
        Q.id[r] = id; Q.par[r] = P.id[i]; Q.last[r] = c; Q.last2[r] = P.last[i]; Q.len[r] = P.len[i] + 1;
        Q.hash[r] = P.hash[i] * 0x01000193u + (unsigned)c; Q.phash[r] = P.hash[i];
        arena[id] = make_int2(P.id[i], c);
        Q.depth[r] = 0;
        if (a.has_lm) {
#pragma unroll
          for (int x = 0; x < kNgramMaxCtx; ++x) Q.ctx[r][x] = x == 0 ? a.lm.tok2word[c] : (x < C ? P.ctx[i][x - 1] : -1);
          Q.depth[r] = ngram_walk(a.lm, Q.ctx[r], Q.node[r], Q.acc[r]);
        }
      }
    }
    if (t + 1 < Tb) {
      if (tid < K) { s_cv[nxt][tid] = pv; s_ci[nxt][tid] = pi; }
      else if (tid == K) s_blank[nxt] = pv;
    }
    __syncthreads();
  }

  // ---- the n-best: the </s> term of the LM, a last ranking, the backtrace
  const Beam& P = s_beam[Tb & 1];
  const int nb = s_nb[Tb & 1];
  const int N4 = (nb + 3) & ~3;
  if (tid < N4) {
    float s = -INFINITY;
    if (tid < nb) {
      float lmv = P.lm[tid];
      if (a.has_lm) lmv += ngram_point(a.lm, P.depth[tid], P.node[tid], P.acc[tid], a.V - 1);
      s = lae(P.pb[tid], P.pnb[tid]) + a.lm_w * lmv + a.penalty * (float)P.len[tid];
      if (!(s > -INFINITY)) s = -INFINITY;
    }
    s_score[tid] = s;
  }
  __syncthreads();
  int32_t* __restrict__ out = a.out + (long)b * a.nbest * (2 + T);
  if (tid < nb) {
    const float s = s_score[tid];
    const int r = rank_of(s_score, N4, s, tid);
    if (r < a.nbest) {
      int32_t* o = out + (long)r * (2 + T);
      const bool live = s > -INFINITY;
      o[0] = __float_as_int(s);
      o[1] = live ? P.len[tid] : -1;
      if (live) {
        int node = P.id[tid];
        for (int pos = P.len[tid] - 1; pos >= 0 && node > 0; --pos) {
          const int2 e = arena[node];
          o[2 + pos] = e.y;
          node = e.x;
        }
      }
    }
  } else if (tid < a.nbest) {                           // fewer prefixes than nbest
    int32_t* o = out + (long)tid * (2 + T);
    o[0] = __float_as_int(-INFINITY);
    o[1] = -1;
  }
}

}  // namespace

extern "C" {

int64_t eamd_ctc_beam_workspace_bytes(int B, int T, int W) {
  if (B < 1 || T < 1 || W < 1) return 0;
  return (int64_t)B * ((int64_t)T * W + 1) * (int64_t)sizeof(int2);
}

int eamd_ctc_prefix_beam(const float* logp, int64_t ld, const float* cand_val, const int32_t* cand_id, const int32_t* hlens, int B,
                         int T, int V, int W, int K, int nbest, float penalty, const int32_t* tok2word, const float* uni_tok,
                         const float* node_bo, const int32_t* child_start, const int32_t* child_word, const int32_t* child_node,
                         const int32_t* succ_start, const int32_t* qsucc_tok, const float* qsucc_lp, int n_nodes, int N, int bos,
                         int unk, float ngram_weight, void* workspace, int64_t workspace_bytes, int32_t* out, void* stream) {
  if (!logp || !cand_val || !cand_id || !hlens || !workspace || !out) return EAMD_EINVAL;
  if (B < 1 || T < 1 || V < 3 || W < 1 || K < 1 || K > V - 2 || nbest < 1 || nbest > W || ld < V) return EAMD_EINVAL;
  if (W > kMaxW || K > kMaxK || T > kMaxT) return EAMD_EUNSUPPORTED;
  if (workspace_bytes < eamd_ctc_beam_workspace_bytes(B, T, W) || ((uintptr_t)workspace & 7)) return EAMD_EINVAL;
  BeamArgs a;
  a.has_lm = tok2word != nullptr;
  if (a.has_lm) {
    if (!uni_tok || !node_bo || !child_start || !child_word || !child_node || !succ_start || !qsucc_tok || !qsucc_lp)
      return EAMD_EINVAL;
    if (N < 1 || n_nodes < 1) return EAMD_EINVAL;
    if (N > kNgramMaxCtx + 1) return EAMD_EUNSUPPORTED;
  }
  a.logp = logp; a.ld = (long)ld; a.cval = cand_val; a.cid = cand_id; a.hlens = hlens;
  a.arena = (int2*)workspace; a.out = out;
  a.lm.tok2word = tok2word; a.lm.uni_tok = uni_tok; a.lm.node_bo = node_bo; a.lm.child_start = child_start;
  a.lm.child_word = child_word; a.lm.child_node = child_node; a.lm.succ_start = succ_start; a.lm.qsucc_tok = qsucc_tok;
  a.lm.qsucc_lp = qsucc_lp; a.lm.n_nodes = n_nodes; a.lm.V = V; a.lm.C = a.has_lm ? N - 1 : 0; a.lm.unk = unk;
  a.bos = bos; a.lm_w = a.has_lm ? ngram_weight : 0.f; a.penalty = penalty;
  a.T = T; a.V = V; a.W = W; a.K = K; a.nbest = nbest;
  int threads = (W * (K + 1) + EAMD_WAVE - 1) / EAMD_WAVE * EAMD_WAVE;
  threads = threads > kMaxThreads ? kMaxThreads : threads;
  hipLaunchKernelGGL(ctc_prefix_beam_kernel, dim3(B), dim3(threads), 0, (hipStream_t)stream, a);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
