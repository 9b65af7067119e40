// n-gram LM shallow fusion (reference: espnet/nets/scorers/ngram.py:12-102, NgramFullScorer / NgramPartScorer on kenlm):
// the full-vocabulary row log10 p(word(v) | history) of every running hypothesis in ONE launch.
//
// An ARPA back-off model gives  p(w | h) = lp(h' w) + sum of backoff(h'') over the suffixes h'' of h longer than h',
// h' = the longest suffix of h for which the n-gram (h' w) is listed.  The row over all w is therefore a function of the last
// N - 1 words only: the dense unigram row plus, for every suffix of the history that is a known context, a short list of
// overwrites.  Tables (espnet_amd/nets/ngram.py: ArpaLM): a trie of contexts stored most recent word first, so that the
// suffixes of one history are ONE root-to-leaf walk; per node a back-off weight, a range of sorted (word, child) edges and
// a range of (token id, log10-prob) successors already expanded to token ids.
//
//   one workgroup per row:
//     wave 0   ctx_new = (word(newest token), ctx_prev[0 .. N-3]); walk the trie along it (a 64-ary search per level: a
//              chunk boundary per lane and one ballot, 3 dependent loads for 5000 children where bisection takes 13);
//              depth D, nodes 0..D, acc_j = sum_{i=j+1..D} backoff(node_i) added in increasing i -> LDS
//     pass 0   logp[v] = uni_tok[v] + acc_0 for all v (16-byte stores where V and the row allow)
//     pass j   (1..D, a barrier between passes) logp[t] = lp + acc_j for the successors (t, lp) of node_j: the longer
//              context overwrites the shorter one - the ORDER of the passes is the back-off rule.
//   The row stays in global memory between the passes (V is unbounded; a pass is one coalesced sweep or a short scatter).
#include "common.h"
#include "ngram_query.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxCtx = 7;            // orders up to 8

struct NgramArgs {
  const int32_t* tok2word; const float* uni_tok; const float* node_bo;
  const int32_t* child_start; const int32_t* child_word; const int32_t* child_node;
  const int32_t* succ_start; const int32_t* succ_tok; const float* succ_lp;
  const int32_t* ctx_prev; long ctx_ld;
  const long long* tok; long tok_ld;
  float* logp; int32_t* ctx_new;
  int n_nodes, V, C, bos, unk, first, vec;
};

// position of `w` among the sorted words child_word[lo .. hi), or -1; called by every lane of ONE wave with the same arguments
__device__ __forceinline__ int find_child(const int32_t* __restrict__ child_word, int lo, int hi, int w, int lane) {
  while (hi - lo > EAMD_WAVE) {
    const int step = (hi - lo + EAMD_WAVE - 1) / EAMD_WAVE;
    const long idx = (long)lo + (long)lane * step;              // first word of this lane's chunk
    const bool le = idx < hi && child_word[idx] <= w;
    const unsigned long long m = __ballot(le);                  // sorted: a prefix of the lanes
    if (m == 0ULL) return -1;
    lo += (__popcll(m) - 1) * step;
    hi = lo + step < hi ? lo + step : hi;
  }
  const int idx = lo + lane;
  const unsigned long long m = __ballot(idx < hi && child_word[idx] == w);
  return m == 0ULL ? -1 : lo + __ffsll((long long)m) - 1;
}

__global__ __launch_bounds__(kThreads) void ngram_score_kernel(NgramArgs a) {
  __shared__ int s_node[kMaxCtx + 1];
  __shared__ float s_acc[kMaxCtx + 1];
  __shared__ int s_depth;
  const long row = blockIdx.x;
  const int tid = threadIdx.x, C = a.C, V = a.V;

  if (tid < EAMD_WAVE) {
    int ctx[kMaxCtx];
    int w0 = a.bos;
    if (!a.first) {
      const long long t = a.tok[row * a.tok_ld];
      w0 = (t >= 0 && t < V) ? a.tok2word[t] : a.unk;           // an id outside [0, V) is <unk>: never an index
    }
#pragma unroll
    for (int i = 0; i < kMaxCtx; ++i) {
      int w = -1;
      if (i == 0) w = w0;
      else if (i < C) w = a.ctx_prev[row * a.ctx_ld + (i - 1)];
      ctx[i] = w;
      if (i < C && tid == 0) a.ctx_new[row * C + i] = w;
    }
    float bo[kMaxCtx + 1];
    int depth = 0, node = 0;
    if (tid == 0) s_node[0] = 0;
#pragma unroll
    for (int j = 0; j < kMaxCtx; ++j) {
      bo[j + 1] = 0.f;
      if (j < C && depth == j && ctx[j] >= 0) {
        const int pos = find_child(a.child_word, a.child_start[node], a.child_start[node + 1], ctx[j], tid);
        const int next = pos >= 0 ? a.child_node[pos] : -1;
        if (next > 0 && next < a.n_nodes) {
          node = next;
          depth = j + 1;
          bo[j + 1] = a.node_bo[node];
          if (tid == 0) s_node[j + 1] = node;
        }
      }
    }
    if (tid == 0) {
      s_depth = depth;
#pragma unroll
      for (int j = 0; j <= kMaxCtx; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int i = 1; i <= kMaxCtx; ++i)
          if (i > j && i <= depth) acc += bo[i];
        s_acc[j] = acc;
      }
    }
  }
  __syncthreads();
  const int depth = s_depth;
  float* __restrict__ out = a.logp + row * (long)V;

  const float acc0 = s_acc[0];
  if (a.vec) {
    const f32x4* __restrict__ u4 = (const f32x4*)a.uni_tok;
    f32x4* o4 = (f32x4*)out;
    for (int q = tid; q < V / 4; q += kThreads) {
      f32x4 x = u4[q];
      x.x += acc0; x.y += acc0; x.z += acc0; x.w += acc0;
      o4[q] = x;
    }
  } else {
    for (int v = tid; v < V; v += kThreads) out[v] = a.uni_tok[v] + acc0;
  }
  for (int j = 1; j <= depth; ++j) {
    __syncthreads();                                            // pass j - 1 has landed: pass j overwrites it
    const int node = s_node[j];
    const float acc = s_acc[j];
    const int e = a.succ_start[node + 1];
    for (int k = a.succ_start[node] + tid; k < e; k += kThreads) {
      const int t = a.succ_tok[k];
      if ((unsigned)t < (unsigned)V) out[t] = a.succ_lp[k] + acc;
    }
  }
}

// eamd_ngram_score_pairs: one lane per (context, token) pair (ngram_query.h)
__global__ __launch_bounds__(kThreads) void ngram_pairs_kernel(NgramQueryTables g, const int32_t* __restrict__ ctx,
                                                               const long long* __restrict__ tok, float* __restrict__ lp,
                                                               int32_t* __restrict__ ctx_new, int n) {
  const long r = (long)blockIdx.x * kThreads + threadIdx.x;
  if (r >= n) return;
  int c[kNgramMaxCtx], node[kNgramMaxCtx + 1];
  float acc[kNgramMaxCtx + 1];
#pragma unroll
  for (int i = 0; i < kNgramMaxCtx; ++i) c[i] = i < g.C ? ctx[r * g.C + i] : -1;
  const int depth = ngram_walk(g, c, node, acc);
  const long long t = tok[r];
  const bool known = t >= 0 && t < g.V;
  lp[r] = known ? ngram_point(g, depth, node, acc, (int)t) : -INFINITY;
#pragma unroll
  for (int i = 0; i < kNgramMaxCtx; ++i)
    if (i < g.C) ctx_new[r * g.C + i] = i == 0 ? (known ? g.tok2word[t] : g.unk) : c[i - 1];
}

}  // namespace

extern "C" {

int eamd_ngram_score_pairs(const int32_t* tok2word, const float* uni_tok, const float* node_bo, const int32_t* child_start,
                           const int32_t* child_word, const int32_t* child_node, const int32_t* succ_start,
                           const int32_t* qsucc_tok, const float* qsucc_lp, int n_nodes, int V, int N, int unk,
                           const int32_t* ctx, const int64_t* tok, float* lp, int32_t* ctx_new, int n, void* stream) {
  if (!tok2word || !uni_tok || !node_bo || !child_start || !child_word || !child_node || !succ_start || !qsucc_tok || !qsucc_lp ||
      !tok || !lp)
    return EAMD_EINVAL;
  if (n < 1 || V < 1 || N < 1 || n_nodes < 1) return EAMD_EINVAL;
  if (N > kNgramMaxCtx + 1) return EAMD_EUNSUPPORTED;
  if (N > 1 && (!ctx || !ctx_new)) return EAMD_EINVAL;
  NgramQueryTables g;
  g.tok2word = tok2word; g.uni_tok = uni_tok; g.node_bo = node_bo; g.child_start = child_start; g.child_word = child_word;
  g.child_node = child_node; g.succ_start = succ_start; g.qsucc_tok = qsucc_tok; g.qsucc_lp = qsucc_lp;
  g.n_nodes = n_nodes; g.V = V; g.C = N - 1; g.unk = unk;
  hipLaunchKernelGGL(ngram_pairs_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, g, ctx,
                     (const long long*)tok, lp, ctx_new, n);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_ngram_score(const int32_t* tok2word, const float* uni_tok, const float* node_bo, const int32_t* child_start,
                     const int32_t* child_word, const int32_t* child_node, const int32_t* succ_start, const int32_t* succ_tok,
                     const float* succ_lp, int n_nodes, int V, int N, int bos, int unk, const int32_t* ctx_prev, int64_t ctx_ld,
                     const int64_t* tok, int64_t tok_ld, int first, float* logp, int32_t* ctx_new, int n, void* stream) {
  if (!tok2word || !uni_tok || !node_bo || !child_start || !child_word || !child_node || !succ_start || !succ_tok || !succ_lp ||
      !tok || !logp)
    return EAMD_EINVAL;
  if (n < 1 || V < 1 || N < 1 || n_nodes < 1 || ctx_ld < 0) return EAMD_EINVAL;
  if (N > kMaxCtx + 1) return EAMD_EUNSUPPORTED;
  if (N > 1 && (!ctx_prev || !ctx_new)) return EAMD_EINVAL;
  NgramArgs a;
  a.tok2word = tok2word; a.uni_tok = uni_tok; a.node_bo = node_bo; a.child_start = child_start; a.child_word = child_word;
  a.child_node = child_node; a.succ_start = succ_start; a.succ_tok = succ_tok; a.succ_lp = succ_lp;
  a.ctx_prev = ctx_prev; a.ctx_ld = (long)ctx_ld; a.tok = (const long long*)tok; a.tok_ld = (long)tok_ld;
  a.logp = logp; a.ctx_new = ctx_new; a.n_nodes = n_nodes; a.V = V; a.C = N - 1; a.bos = bos; a.unk = unk; a.first = first != 0;
  a.vec = V % 4 == 0 && !((uintptr_t)logp & 15) && !((uintptr_t)uni_tok & 15);
  hipLaunchKernelGGL(ngram_score_kernel, dim3(n), dim3(kThreads), 0, (hipStream_t)stream, a);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
