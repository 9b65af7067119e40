// Shared by the batched transducer search kernels (rnnt_alsd.hip, rnnt_tsd.hip, rnnt_nsc.hip, rnnt_default.hip): the beam
// bookkeeping every one of them does on W <= 16 slots per utterance.  Everything is forced inline: a step kernel pays for what it
// passes in, nothing else.
#pragma once

// numpy.logaddexp on doubles (npy_logaddexp)
__device__ __forceinline__ double al_logaddexp(double a, double b) {
  if (a == b) return a + 0.693147180559945309417232121458176568;
  const double d = a - b;
  if (d > 0) return a + log1p(exp(-d));
  if (d <= 0) return b + log1p(exp(d));
  return d;                                    // NaN
}

// numpy.logaddexp on floats (npy_logaddexpf)
__device__ __forceinline__ float al_logaddexpf(float a, float b) {
#pragma clang fp contract(off)
  if (a == b) return a + 0.693147180559945309417232121458176568f;
  const float d = a - b;
  if (d > 0) return a + log1pf(expf(-d));
  if (d <= 0) return b + log1pf(expf(d));
  return d;                                    // NaN
}

// Score sums of alsd / tsd.  Without an LM (LM = false) every sum is a double plus a float.  With RNNLM shallow fusion the reference
// adds lm_weight * torch.tensor(q, dtype=float32) to an extension's score, which turns the score into a float32 0-d tensor: from
// the first label on every later sum, and the logaddexp of a merge, runs in float32; only [blank] (u == 0 labels) and its chain of
// blank continuations stay double.  A score is still STORED as a double; with LM = true one with u > 0 holds a float32 value.  The
// float sums and the product are single IEEE operations: contraction is switched off in these functions (device code is compiled
// with -ffp-contract=fast, and HIP's __fmul_rn / __fadd_rn are plain operators that the compiler fuses into one multiply-add after
// inlining), so that wf * q is rounded to float32 before it is added, as torch rounds it.
//   rs_add    parent score S with u labels + a joint log-probability: a blank continuation, or the first half of an extension
//   rs_ext    an extension: rs_add, then + (float)lm_weight * q, the product rounded to float32 before the sum
//   rs_merge  the score of two equal label sequences of u labels
template <bool LM>
__device__ __forceinline__ double rs_add(double S, int u, float lp) {
#pragma clang fp contract(off)
  if (!LM || u == 0) return S + (double)lp;
  return (double)((float)S + lp);
}
template <bool LM>
__device__ __forceinline__ double rs_ext(double S, int u, float lp, float q, float wf) {
#pragma clang fp contract(off)
  if (!LM) return S + (double)lp;
  const float m = wf * q;                      // rounded to float32 before the sum
  const float s = (float)rs_add<true>(S, u, lp);
  return (double)(s + m);
}
template <bool LM>
__device__ __forceinline__ double rs_merge(double a, double b, int u) {
  if (!LM || u == 0) return al_logaddexp(a, b);
  return (double)al_logaddexpf((float)a, (float)b);
}

// how a score ranks: NaN counts as -inf
__device__ __forceinline__ double rs_key(double v) { return v != v ? -INFINITY : v; }

// position of entry `self` in sorted(score[0 .. n), reverse=True) over the entries with in(o): the entries with a larger key, or an
// equal key and an earlier index (stable: equal scores keep the list's order)
template <class In>
__device__ __forceinline__ int rs_rank(const double* score, int n, int self, In in) {
  const double key = rs_key(score[self]);
  int cnt = 0;
  for (int o = 0; o < n; ++o) {
    const double ok = rs_key(score[o]);
    cnt += (in(o) && (ok > key || (ok == key && o < self))) ? 1 : 0;
  }
  return cnt;
}
__device__ __forceinline__ int rs_rank(const double* score, int n, int self) {
  return rs_rank(score, n, self, [](int) { return true; });
}

// One wave: do two label rows hold the same labels 1 .. L?  Element e of a row is y[e] up to its parent's length pu and the
// appended token tk beyond it (a row that appends nothing passes pu >= L).  Both rows must be allocated to L + 1 elements: the two
// loads of a round are issued side by side whatever pu is, and what lies past pu is dropped after them.  64 labels at a time from the
// end: hypotheses of a beam share their beginnings, a difference shows in the first round.  Every lane of the wave must call it; all
// get the answer.
__device__ __forceinline__ bool rs_same_labels(const int* y1, int pu1, int tk1, const int* y2, int pu2, int tk2, int L, int lane) {
  bool eq = true;
  for (int hi = L; hi >= 1 && eq; hi -= 64) {
    const int e = hi - lane;
    bool same = true;
    if (e >= 1) {
      const int v1 = y1[e], v2 = y2[e];
      same = (e <= pu1 ? v1 : tk1) == (e <= pu2 ? v2 : tk2);
    }
    eq = __all(same ? 1 : 0) != 0;
  }
  return eq;
}

// a label row to write: elements 0 .. u of dst, element e from src[e] up to the parent's length pu, the appended token tk beyond
struct RsLabels {
  int* dst;
  const int* src;
  int pu, u, tk;
};

// the label rows of nn slots, `width` elements each at most, by the whole workgroup; row(m) says what slot m gets
template <int THREADS, class Row>
__device__ __forceinline__ void rs_copy_labels(int nn, int width, int tid, Row row) {
  for (int x = tid; x < nn * width; x += THREADS) {
    const int m = x / width, e = x - m * width;
    const RsLabels r = row(m);
    if (e > r.u) continue;
    r.dst[e] = e <= r.pu ? r.src[e] : r.tk;
  }
}

// tsd / nsc, an utterance that is over at a frame's last call: its nb hypotheses (count entry `cfrom`, block rows from0 ..) are
// carried unchanged to the other parity (count entry `cto`, block rows to0 ..)
template <int THREADS>
__device__ __forceinline__ void rs_carry_block(double* score, int* ulen, int* count, int* yseq, int ycap, int W, int cfrom, int cto,
                                               int from0, int to0, int tid) {
  const int nb = min(max(count[cfrom], 0), W);
  if (tid == 0) count[cto] = nb;
  if (tid < nb) {
    score[to0 + tid] = score[from0 + tid];
    ulen[to0 + tid] = ulen[from0 + tid];
  }
  rs_copy_labels<THREADS>(nb, ycap, tid, [&](int w) {
    const int u = min(max(ulen[from0 + w], 0), ycap - 1);
    return RsLabels{yseq + (long)(to0 + w) * ycap, yseq + (long)(from0 + w) * ycap, u, u, 0};
  });
}

// host: is no array handed in for two operands?  (a workgroup's stores would meet its own loads)
template <int N>
inline bool rs_distinct(const void* const (&p)[N]) {
  for (int x = 0; x < N; ++x)
    for (int y = x + 1; y < N; ++y)
      if (p[x] == p[y]) return false;
  return true;
}
