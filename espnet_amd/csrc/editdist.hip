// Error-rate scoring on the device (reference: espnet/nets/e2e_asr_common.py:103-246, ErrorCalculator): token ids ->
// symbol sequences (eamd_text_units) -> batched Levenshtein distance (eamd_edit_distance).  Integer work, bit-exact.
//
//   text_units    : one workgroup per row, two block scans.  Pass A keeps ids[:limit] (optionally the first of each run,
//                   itertools.groupby), replaces every kept id by its code points from a CSR token table and writes the
//                   row's code-point stream to `scratch` at the exclusive scan of the token lengths.  Pass B turns the
//                   stream into symbols at the exclusive scan of a per-code-point flag: chars = every code point that is
//                   not drop_cp; words = every code point that starts a run of non-0x20 (str.split()), whose thread walks
//                   the word and emits a 64-bit hash of its code points.  editdistance.eval compares hashes of the list
//                   items too, so a 64-bit hash per word gives up nothing the reference has.
//   edit_distance : one workgroup per pair, row by row over the shorter sequence.  Within a row
//                       x[j] = min(P[j] + 1, P[j-1] + (a_i != b_j)),   D[j] = min(x[j], D[j-1] + 1) = j + min_{k<=j}(x[k] - k)
//                   so the in-row dependency is a prefix-min of y[k] = x[k] - k: the (min,+) scan of the CTC prefix scorer.
//                   A thread owns ceil(n / 256) consecutive columns (its column chunk; the carry between chunks is the
//                   block scan of the threads' minima, held in registers and 4 LDS words), so a row of any length costs one
//                   block scan and two barriers.  The two DP rows live in LDS up to kEdLdsCols entries, else in the
//                   caller's workspace.
#include "common.h"
#include "select.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / EAMD_WAVE;
constexpr int kEdLdsCols = 4096;       // DP rows of up to this many entries (n + 1) stay in LDS: 2 rows x 16 KiB
constexpr int kEdInf = 1 << 29;

// exclusive prefix min over the workgroup's threads (kEdInf for thread 0).  One barrier: s_w must not be rewritten before the
// caller's next barrier.
__device__ __forceinline__ int block_excl_min(int v, int* s_w) {
  const int lane = threadIdx.x & (EAMD_WAVE - 1), w = threadIdx.x / EAMD_WAVE;
  int inc = v;
#pragma unroll
  for (int d = 1; d < EAMD_WAVE; d <<= 1) {
    const int o = __shfl_up(inc, d, EAMD_WAVE);
    if (lane >= d) inc = min(inc, o);
  }
  if (lane == EAMD_WAVE - 1) s_w[w] = inc;
  int ex = __shfl_up(inc, 1, EAMD_WAVE);
  if (lane == 0) ex = kEdInf;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kWaves; ++k)
    if (k < w) ex = min(ex, s_w[k]);
  return ex;
}

__global__ __launch_bounds__(kThreads) void edit_distance_kernel(const long long* __restrict__ a, long lda,
                                                                 const long long* __restrict__ b, long ldb,
                                                                 const int* __restrict__ alen, const int* __restrict__ blen,
                                                                 int* __restrict__ dist, int* __restrict__ ws, long ws_pair) {
  __shared__ int s_row[2 * kEdLdsCols];
  __shared__ int s_w[2][kWaves];
  const int p = blockIdx.x, tid = threadIdx.x;
  int m = min(max(alen[p], 0), (int)lda), n = min(max(blen[p], 0), (int)ldb);
  const long long* ra = a + (long)p * lda;
  const long long* rb = b + (long)p * ldb;
  if (m > n) {        // the distance is symmetric: rows over the shorter sequence, columns (the parallel axis) over the longer
    const long long* t = ra; ra = rb; rb = t;
    const int ti = m; m = n; n = ti;
  }
  if (m == 0) {       // uniform over the workgroup: no barrier is skipped by part of it
    if (tid == 0) dist[p] = n;
    return;
  }
  int* cur = (n + 1 <= kEdLdsCols) ? s_row : ws + (long)p * ws_pair;
  int* nxt = cur + (n + 1);
  for (int j = tid; j <= n; j += kThreads) cur[j] = j;
  const int K = (n + kThreads - 1) / kThreads;
  const int j0 = 1 + tid * K, j1 = min(n, j0 + K - 1);
  __syncthreads();
  for (int i = 1; i <= m; ++i) {
    const long long ai = ra[i - 1];
    // y[k] = x[k] - k over the thread's columns, parked in the new row; column 0 (D[i][0] = i) belongs to thread 0
    int best = (tid == 0) ? i : kEdInf;
    if (j0 <= j1) {
      int diag = cur[j0 - 1];
      for (int j = j0; j <= j1; ++j) {
        const int up = cur[j];
        const int y = min(up + 1, diag + (ai != rb[j - 1] ? 1 : 0)) - j;
        nxt[j] = y;
        best = min(best, y);
        diag = up;
      }
    }
    int carry = block_excl_min(best, s_w[i & 1]);
    if (tid == 0) { nxt[0] = i; carry = i; }
    for (int j = j0; j <= j1; ++j) {
      carry = min(carry, nxt[j]);
      nxt[j] = carry + j;
    }
    __syncthreads();
    int* t = cur; cur = nxt; nxt = t;
  }
  if (tid == 0) dist[p] = cur[n];
}

__device__ __forceinline__ unsigned long long word_hash(const int* __restrict__ s, int p, int n) {
  unsigned long long h = 0xcbf29ce484222325ull;      // FNV-1a over the word's code points (4 bytes each), then its length
  int q = p;
  for (; q < n && s[q] != 0x20; ++q) {
    unsigned int c = (unsigned int)s[q];
#pragma unroll
    for (int k = 0; k < 4; ++k) { h = (h ^ (c & 0xffu)) * 0x100000001b3ull; c >>= 8; }
  }
  h = (h ^ (unsigned long long)(q - p)) * 0x100000001b3ull;
  return h ^ (h >> 29);
}

__global__ __launch_bounds__(kThreads) void text_units_kernel(const int* __restrict__ ids, const int* __restrict__ limit,
                                                              const int* __restrict__ tok_off, const int* __restrict__ tok_cp,
                                                              int* __restrict__ scratch, long long* __restrict__ out,
                                                              int* __restrict__ outlen, int L, int V, int cap, int collapse,
                                                              int drop_cp, int words) {
  __shared__ int s_w[kWaves];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int* row = ids + (long)b * L;
  int* s = scratch + (long)b * cap;
  long long* o = out + (long)b * cap;
  const int lim = limit ? min(max(limit[b], 0), L) : L;
  // pass A: ids -> code-point stream
  int n = 0;
  for (int base = 0; base < lim; base += kThreads) {
    const int i = base + tid;
    int id = -1, off = 0, len = 0;
    if (i < lim) {
      id = row[i];
      if (id >= 0 && id < V && !(collapse && i > 0 && row[i - 1] == id)) {
        off = tok_off[id];
        len = tok_off[id + 1] - off;
      }
    }
    int tot;
    const int pos = n + block_excl_sum<kThreads>(len, s_w, &tot);
    for (int k = 0; k < len && pos + k < cap; ++k) s[pos + k] = tok_cp[off + k];
    n += tot;
  }
  n = min(n, cap);
  __syncthreads();          // the stream is read across threads below
  // pass B: stream -> symbols
  int cnt = 0;
  for (int base = 0; base < n; base += kThreads) {
    const int q = base + tid;
    int cp = 0x20, flag = 0;
    if (q < n) {
      cp = s[q];
      flag = words ? (cp != 0x20 && (q == 0 || s[q - 1] == 0x20)) : (cp != drop_cp);
    }
    int tot;
    const int pos = cnt + block_excl_sum<kThreads>(flag, s_w, &tot);
    if (flag) o[pos] = words ? (long long)word_hash(s, q, n) : (long long)cp;
    cnt += tot;
  }
  if (tid == 0) outlen[b] = cnt;
}

}  // namespace

extern "C" {

int64_t eamd_edit_distance_workspace_bytes(int B, int lda, int ldb) {
  if (B <= 0 || lda < 0 || ldb < 0) return 0;
  const int64_t n = lda > ldb ? lda : ldb;
  return (int64_t)B * 2 * (n + 1) * (int64_t)sizeof(int32_t);
}

int eamd_edit_distance(const int64_t* a, int lda, const int32_t* alen, const int64_t* b, int ldb, const int32_t* blen,
                       int32_t* dist, void* workspace, int64_t workspace_bytes, int B, void* stream) {
  if (!a || !b || !alen || !blen || !dist || !workspace || B <= 0 || lda <= 0 || ldb <= 0) return EAMD_EINVAL;
  if (workspace_bytes < eamd_edit_distance_workspace_bytes(B, lda, ldb)) return EAMD_EINVAL;
  const long n = lda > ldb ? lda : ldb;
  hipLaunchKernelGGL(edit_distance_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, (const long long*)a, (long)lda,
                     (const long long*)b, (long)ldb, alen, blen, dist, (int*)workspace, 2 * (n + 1));
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_text_units(const int32_t* ids, const int32_t* limit, const int32_t* tok_off, const int32_t* tok_cp,
                    int32_t* scratch, int64_t* out, int32_t* outlen, int B, int L, int V, int cap, int collapse,
                    int drop_cp, int mode, void* stream) {
  if (!ids || !tok_off || !tok_cp || !scratch || !out || !outlen || B <= 0 || L <= 0 || V <= 0 || cap <= 0)
    return EAMD_EINVAL;
  if (mode != EAMD_TEXT_CHARS && mode != EAMD_TEXT_WORDS) return EAMD_EINVAL;
  hipLaunchKernelGGL(text_units_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, ids, limit, tok_off, tok_cp, scratch,
                     (long long*)out, outlen, L, V, cap, collapse ? 1 : 0, drop_cp, mode == EAMD_TEXT_WORDS ? 1 : 0);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
