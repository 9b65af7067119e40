// Point queries on the flat ARPA tables of espnet_amd/nets/ngram.py (ArpaLM): log10 p(word(tok) | context) for ONE
// (context, token) pair by ONE lane, where ngram_score_kernel (ngram.hip) writes the whole vocabulary row of a context with a
// workgroup.  The value is bit-equal to that row's element: the same walk of the context trie (most recent word first, stops at
// the first -1 / unknown context), the same back-off sums acc_j = sum_{i=j+1..D} node_bo[node_i] added in increasing i from
// 0.f, and the row's last overwrite = the deepest node j <= D that lists the token.  "Lists the token" needs a search inside a
// node: qsucc_tok / qsucc_lp are the node's successors sorted by token id (ArpaLM.qsucc_tok / qsucc_lp; a (node, token) pair
// occurs once), bisected here.  Shared by eamd_ngram_score_pairs (ngram.hip) and the CTC prefix beam search (ctc_beam.hip).
#pragma once
#include "common.h"

constexpr int kNgramMaxCtx = 7;       // orders up to 8

struct NgramQueryTables {
  const int32_t* tok2word; const float* uni_tok; const float* node_bo;
  const int32_t* child_start; const int32_t* child_word; const int32_t* child_node;
  const int32_t* succ_start; const int32_t* qsucc_tok; const float* qsucc_lp;
  int n_nodes, V, C, unk;
};

// first position in the sorted a[lo .. hi) that is >= key
__device__ __forceinline__ int ngram_lower_bound(const int32_t* __restrict__ a, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the walk along ctx [C] (word ids, most recent first, -1 = empty): node[0 .. depth], acc[0 .. kNgramMaxCtx] -> depth
__device__ __forceinline__ int ngram_walk(const NgramQueryTables& g, const int* ctx, int* node, float* acc) {
  float bo[kNgramMaxCtx + 1];
  int depth = 0, cur = 0;
  node[0] = 0;
#pragma unroll
  for (int j = 0; j < kNgramMaxCtx; ++j) {
    bo[j + 1] = 0.f;
    node[j + 1] = 0;
    if (j < g.C && depth == j) {
      const int w = ctx[j];
      if (w >= 0) {
        const int lo = g.child_start[cur], hi = g.child_start[cur + 1];
        const int p = ngram_lower_bound(g.child_word, lo, hi, w);
        const int next = (p < hi && g.child_word[p] == w) ? g.child_node[p] : -1;
        if (next > 0 && next < g.n_nodes) {
          cur = next;
          depth = j + 1;
          bo[j + 1] = g.node_bo[cur];
          node[j + 1] = cur;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j <= kNgramMaxCtx; ++j) {
    float a = 0.f;
#pragma unroll
    for (int i = 1; i <= kNgramMaxCtx; ++i)
      if (i > j && i <= depth) a += bo[i];
    acc[j] = a;
  }
  return depth;
}

// log10 p(word(tok) | the walked context), 0 <= tok < V
__device__ __forceinline__ float ngram_point(const NgramQueryTables& g, int depth, const int* node, const float* acc, int tok) {
#pragma unroll
  for (int j = kNgramMaxCtx; j >= 1; --j) {
    if (j <= depth) {
      const int n = node[j];
      const int lo = g.succ_start[n], hi = g.succ_start[n + 1];
      const int p = ngram_lower_bound(g.qsucc_tok, lo, hi, tok);
      if (p < hi && g.qsucc_tok[p] == tok) return g.qsucc_lp[p] + acc[j];
    }
  }
  return g.uni_tok[tok] + acc[0];
}
