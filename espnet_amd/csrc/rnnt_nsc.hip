// Batched N-step constrained transducer beam search: the bookkeeping of one call (frame t, n-step v) for n utterances in one launch.
// reference: espnet/nets/beam_search_transducer.py:466-663 (nsc_beam_search without an LM), transducer/utils.py:75-93 (substract).
// Every frame takes nstep = N expansions (and, when N > 1, one more pass for the blank term of the last V) whatever the hypotheses
// are, so the utterances of a batch advance in lock-step; what the reference does with Python lists per utterance - sort `kept` by
// length, rescore every hypothesis by its shorter prefixes, expand `hyps` into its k extensions, append the blank continuations to
// S, keep the `beam` best extensions that are no member of `hyps` as V and, at the frame's end, the `beam` best of S + V as the next
// `kept` - is done here by one workgroup per utterance on W <= 16 slots, at most 16 * 16 = 256 extensions and W * N + W <= 80
// entries of S + V.
//
//   eamd_rnnt_nsc_step   reads eamd_transducer_expand_rows' record of the call's n * W rows (and, at v == 0, the frame's pair
//                        log-probabilities), the block that holds `hyps` and the S of the frame; on a call v < N appends to S and,
//                        when N > 1, writes V into block v + 1; on the frame's last call (v == N, or v == 0 when N == 1) writes the
//                        other parity of `kept` and the pair list of the next frame; and leaves per row what the rest of the pass
//                        needs: the block row whose prediction-network state it continues (par), the appended token (tok), the
//                        cell kernels' mask (live) and, per history level, the row of the stacked lin_dec outputs it takes (hidx).
//                        Selection is a rank-by-counting sort in LDS (rs_rank: stable, equal scores keep the list's order, NaN as
//                        -inf); prefix tests compare lengths and then tokens, one wave per pair (rs_same_labels).
// Prefix rescoring reads every pair term from the history rows of the LONGER hypothesis j: term a (a = delta .. 1) is
// logp(joint(enc_t, hist[a] of j))[y_j[len_j - a]], where hist[a] is lin_dec of the prediction output of y_j[:-a].  The reference
// takes the first term from hyps[i].y[-1]: the prediction output of the same labels, hence the same vector.
// Hypotheses live in N + 2 blocks of n * W rows: block 0 and block N + 1 are the two parities of `kept`, block v (1 <= v <= N) is
// the V of n-step v - 1 = the `hyps` of n-step v.  Block row = block * n * W + b * W + w.  With N == 1 the V of the one n-step goes
// straight into the next `kept` and block 1 is never written.  The lin_dec outputs are stacked [block][level][n * W]: level 0 = the
// row's own d, level a = hist[a]; hrow(block row, level) is a row of that stack.  Plain stores, no atomics, no scratch buffers: a
// workgroup owns its utterance's rows.
#include "common.h"
#include "rnnt_search.h"
#include "../../include/espnet_amd.h"

namespace {

constexpr int NS_W = 16;                       // slots per utterance at most
constexpr int NS_N = 4;                        // n-steps per frame at most
constexpr int NS_A = 3;                        // prefix_alpha at most
constexpr int NS_D = NS_W * NS_W;              // extensions at most: W slots x k <= W tokens
constexpr int NS_M = NS_W * NS_N + NS_W;       // entries of S + V at most
constexpr int NS_THREADS = 256;

__global__ __launch_bounds__(NS_THREADS) void rnnt_nsc_step_kernel(
    const float* __restrict__ rec, const float* __restrict__ pair_lp, const int* __restrict__ hlens, double* __restrict__ score,
    int* __restrict__ ulen, int* __restrict__ count, int* __restrict__ yseq, double* __restrict__ s_score, int* __restrict__ s_src,
    int* __restrict__ nS, int* __restrict__ par, long long* __restrict__ tok, unsigned char* __restrict__ live,
    int* __restrict__ hidx, int* __restrict__ pairs, int n, int W, int V, int T, int N, int alpha, int t, int v, int p) {
  __shared__ double d_score[NS_D];             // the extensions, in hyps' order
  __shared__ double m_score[NS_M];             // S, then V: what the next kept is chosen from
  __shared__ double h_score[NS_W], h_orig[NS_W];
  __shared__ float s_rec[NS_W * (1 + 2 * NS_W)];
  __shared__ float s_pl[NS_W * NS_A];
  __shared__ int m_src[NS_M], m_cand[NS_M];    // entry -> its block row; with N == 1, an entry of V -> its extension (else -1)
  __shared__ int h_ulen[NS_W], h_last[NS_W], s_perm[NS_W], s_sel[NS_W];
  __shared__ int k_src[NS_W], k_pu[NS_W], k_u[NS_W], k_tk[NS_W];   // new slot -> source row, its length, the new length, token
  __shared__ unsigned char s_pre[NS_W][NS_W];  // [i][j] = delta when slot i's labels are a proper prefix of slot j's, else 0
  __shared__ unsigned char d_ok[NS_D];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = min(W, V - 1), RW = 1 + 2 * k;
  const int ycap = 1 + T * N, SC = W * N, LV = 1 + alpha;
  const int R = n * W, rows = (N + 2) * R;
  const int kp = p ? N + 1 : 0, ko = p ? 0 : N + 1;
  const bool last = N == 1 || v == N;
  const int cin = v == 0 ? kp : v;
  const int Tb = max(0, hlens ? min(hlens[b], T) : T);
  const int row0 = b * W;
  const int in0 = cin * R + row0;
  const int out0 = (last ? ko : v + 1) * R + row0;
  auto hrow = [&](int br, int lvl) { return ((br / R) * LV + lvl) * R + br % R; };
  if (t >= Tb) {                               // the utterance is over: kept waits in parity p
    const int b0 = kp * R + row0;
    if (tid < W) {
      par[row0 + tid] = b0 + tid;
      tok[row0 + tid] = 0;
      live[row0 + tid] = 0;
      for (int a = 0; a < LV; ++a) hidx[a * R + row0 + tid] = hrow(b0 + tid, a);
    }
    if (last) rs_carry_block<NS_THREADS>(score, ulen, count, yseq, ycap, W, kp * n + b, ko * n + b, b0, out0, tid);
    return;
  }
  const int nc = min(max(count[cin * n + b], 0), W);
  int nm;                                      // entries of S + V the next kept is chosen from (last call only)
  if (v < N) {
    const int ns0 = v == 0 ? 0 : min(max(nS[b], 0), SC - W);
    for (int x = tid; x < W * RW; x += NS_THREADS) s_rec[x] = rec[(long)row0 * RW + x];
    if (tid < W) {
      const int u = tid < nc ? min(max(ulen[in0 + tid], 0), ycap - 1) : 0;
      h_ulen[tid] = u;
      h_orig[tid] = tid < nc ? score[in0 + tid] : 0.0;
      h_last[tid] = tid < nc ? yseq[(long)(in0 + tid) * ycap + u] : -1;
    }
    if (v == 0 && tid >= 64 && tid < 64 + W * alpha) s_pl[tid - 64] = pair_lp[(long)row0 * alpha + tid - 64];
    __syncthreads();
    // which slot's labels begin which other slot's: lengths, then the tokens of the shorter one
    const int dmax = v == 0 ? max(alpha, 1) : 1;
    for (int q = wave; q < nc * nc; q += NS_THREADS / 64) {
      const int i = q / nc, j = q - i * nc, L = h_ulen[i];
      const int dl = h_ulen[j] - L;
      const bool pre = dl >= 1 && dl <= dmax &&
                       rs_same_labels(yseq + (long)(in0 + i) * ycap, L, 0, yseq + (long)(in0 + j) * ycap, L, 0, L, lane);
      if (lane == 0) s_pre[i][j] = pre ? dl : 0;
    }
    // hyps: at v == 0 kept by length descending, stable; else the block's own order
    if (tid < nc) {
      int pos = tid;
      if (v == 0) {
        pos = 0;
        for (int o = 0; o < nc; ++o) pos += (h_ulen[o] > h_ulen[tid] || (h_ulen[o] == h_ulen[tid] && o < tid)) ? 1 : 0;
      }
      s_perm[pos] = tid;
    }
    __syncthreads();
    // prefix rescoring: hyps[j] gains every later hyps[i] that is a prefix of it within alpha labels, in ascending i, from the
    // scores as they were
    if (tid < nc) {
      const int j = s_perm[tid];
      double s = h_orig[j];
      if (v == 0 && alpha > 0) {
        for (int pi = tid + 1; pi < nc; ++pi) {
          const int i = s_perm[pi], dl = s_pre[i][j];
          if (dl >= 1 && dl <= alpha) {
            double curr = h_orig[i];
            for (int a = dl; a >= 1; --a) curr += (double)s_pl[j * alpha + a - 1];
            s = al_logaddexp(s, curr);
          }
        }
      }
      h_score[j] = s;
    }
    __syncthreads();
    // the extensions (substract: none that is a member of hyps) and the blank continuations, which go to S
    const int nd = nc * k;
    bool ok = false;
    if (tid < nd) {
      const int pos = tid / k, jx = tid - pos * k, w = s_perm[pos];
      const int tk = min(max((int)s_rec[w * RW + 1 + k + jx], 0), V - 1);
      d_score[tid] = h_score[w] + (double)s_rec[w * RW + 1 + jx];
      ok = true;
      for (int m = 0; m < nc; ++m) ok = ok && !(s_pre[w][m] == 1 && h_last[m] == tk);
      d_ok[tid] = ok ? 1 : 0;
    }
    if (tid < nc) {
      const int w = s_perm[tid];
      const double s = h_score[w] + (double)s_rec[w * RW];
      s_score[(long)b * SC + ns0 + tid] = s;
      s_src[(long)b * SC + ns0 + tid] = in0 + w;
      m_score[tid] = s;                        // read with N == 1 only (ns0 == 0)
      m_src[tid] = in0 + w;
      m_cand[tid] = -1;
    }
    if (tid == 0) nS[b] = ns0 + nc;
    const int nok = __syncthreads_count(ok ? 1 : 0);
    if (ok) {
      const int cnt = rs_rank(d_score, nd, tid, [&](int o) { return d_ok[o] != 0; });
      if (cnt < W) s_sel[cnt] = tid;
    }
    __syncthreads();
    const int nv = min(W, nok);
    if (N > 1) {                               // V is block v + 1
      if (tid == 0) count[(v + 1) * n + b] = nv;
      if (tid < W) {
        const int r = row0 + tid;
        if (tid < nv) {
          const int c = s_sel[tid], w = s_perm[c / k], jx = c % k;
          score[out0 + tid] = d_score[c];
          ulen[out0 + tid] = min(h_ulen[w] + 1, ycap - 1);
          par[r] = in0 + w;
          tok[r] = min(max((int)s_rec[w * RW + 1 + k + jx], 0), V - 1);
          live[r] = 1;
          hidx[r] = hrow(in0 + w, 0);
          for (int a = 1; a < LV; ++a) hidx[a * R + r] = hrow(in0 + w, a - 1);
        } else {
          par[r] = in0 + tid;
          tok[r] = 0;
          live[r] = 0;
          for (int a = 0; a < LV; ++a) hidx[a * R + r] = hrow(in0 + tid, a);
        }
      }
      rs_copy_labels<NS_THREADS>(nv, ycap, tid, [&](int m) {
        const int c = s_sel[m], w = s_perm[c / k], jx = c % k;
        return RsLabels{yseq + (long)(out0 + m) * ycap, yseq + (long)(in0 + w) * ycap, h_ulen[w], min(h_ulen[w] + 1, ycap - 1),
                        min(max((int)s_rec[w * RW + 1 + k + jx], 0), V - 1)};
      });
      return;
    }
    if (tid < nv) {                            // N == 1: S is this call's blank continuations, V follows
      m_score[nc + tid] = d_score[s_sel[tid]];
      m_src[nc + tid] = in0 + s_perm[s_sel[tid] / k];
      m_cand[nc + tid] = s_sel[tid];
    }
    nm = nc + nv;
  } else {
    // the finishing call: V (block N) gains its blank term; S of the frame comes first
    const int ns = min(max(nS[b], 0), SC);
    if (tid < nc) {
      m_score[ns + tid] = score[in0 + tid] + (double)rec[(long)(row0 + tid) * RW];
      m_src[ns + tid] = in0 + tid;
      m_cand[ns + tid] = -1;
    }
    if (tid >= 64 && tid < 64 + ns) {
      const int e = tid - 64;
      m_score[e] = s_score[(long)b * SC + e];
      m_src[e] = min(max(s_src[(long)b * SC + e], 0), rows - 1);
      m_cand[e] = -1;
    }
    nm = ns + nc;
  }
  __syncthreads();
  // the frame's end: the first W of sorted(S + V, reverse=True) are the next kept
  if (tid < nm) {
    const int cnt = rs_rank(m_score, nm, tid);
    if (cnt < W) s_sel[cnt] = tid;             // the extensions' s_sel has been read: m_cand holds it
  }
  __syncthreads();
  const int nn = min(W, nm);
  if (tid == 0) count[ko * n + b] = nn;
  if (tid < W) {
    const int r = row0 + tid;
    if (tid < nn) {
      const int e = s_sel[tid], src = m_src[e], c = m_cand[e];
      const int lv = c >= 0 ? 1 : 0;
      const int pu = lv ? h_ulen[src - in0] : min(max(ulen[src], 0), ycap - 1);
      const int u = lv ? min(pu + 1, ycap - 1) : pu;
      const int tk = lv ? min(max((int)s_rec[(src - in0) * RW + 1 + k + c % k], 0), V - 1) : 0;
      k_src[tid] = src;
      k_pu[tid] = pu;
      k_u[tid] = u;
      k_tk[tid] = tk;
      score[out0 + tid] = m_score[e];
      ulen[out0 + tid] = u;
      par[r] = src;
      tok[r] = tk;
      live[r] = lv;
      hidx[r] = hrow(src, 0);
      for (int a = 1; a < LV; ++a) {
        hidx[a * R + r] = hrow(src, lv ? a - 1 : a);
        // the next frame's pair term of depth a: (history row of the pass's joint rows, y[len - a])
        const int x = u + 1 - a, j = r * alpha + a - 1;
        if (a <= u) {
          pairs[2 * j] = a * R + r;
          pairs[2 * j + 1] = x <= pu ? min(max(yseq[(long)src * ycap + x], 0), V - 1) : tk;
        } else {
          pairs[2 * j] = -1;
          pairs[2 * j + 1] = 0;
        }
      }
    } else {
      par[r] = in0 + tid;
      tok[r] = 0;
      live[r] = 0;
      for (int a = 0; a < LV; ++a) hidx[a * R + r] = hrow(in0 + tid, a);
      for (int a = 1; a < LV; ++a) {
        pairs[2 * (r * alpha + a - 1)] = -1;
        pairs[2 * (r * alpha + a - 1) + 1] = 0;
      }
    }
  }
  __syncthreads();
  rs_copy_labels<NS_THREADS>(nn, ycap, tid, [&](int m) {
    return RsLabels{yseq + (long)(out0 + m) * ycap, yseq + (long)k_src[m] * ycap, k_pu[m], k_u[m], k_tk[m]};
  });
}

}  // namespace

extern "C" {

int eamd_rnnt_nsc_step(const float* rec, const float* pair_lp, const int32_t* hlens, double* score, int32_t* ulen, int32_t* count,
                       int32_t* yseq, double* s_score, int32_t* s_src, int32_t* nS, int32_t* par, int64_t* tok, uint8_t* live,
                       int32_t* hidx, int32_t* pairs, int n, int W, int V, int T, int N, int alpha, int t, int v, int p,
                       void* stream) {
  if (!rec || !pair_lp || !score || !ulen || !count || !yseq || !s_score || !s_src || !nS || !par || !tok || !live || !hidx || !pairs)
    return EAMD_EINVAL;
  if (n < 1 || W < 1 || V < 2 || T < 1 || t < 0 || v < 0 || (p != 0 && p != 1)) return EAMD_EINVAL;
  if (N >= 1 && v > (N == 1 ? 0 : N)) return EAMD_EINVAL;
  // one array handed in for two operands: a workgroup's stores would meet its own loads.  (The block a call reads and the block it
  // writes are told apart by (v, p) inside one allocation, so they cannot be the same.)
  const void* const ints[] = {ulen, count, yseq, s_src, nS, par, hidx, pairs};
  if (!rs_distinct(ints) || score == s_score || rec == pair_lp) return EAMD_EINVAL;
  if (W > NS_W || W > V || N < 1 || N > NS_N || alpha < 0 || alpha > NS_A) return EAMD_EUNSUPPORTED;
  if ((int64_t)(N + 2) * (1 + alpha) * n * W > 0x7fffffff || (int64_t)n * T > 0x7fffffff || 1 + (int64_t)T * N > 0x7fffffff / NS_W)
    return EAMD_EUNSUPPORTED;
  hipLaunchKernelGGL(rnnt_nsc_step_kernel, dim3(n), dim3(NS_THREADS), 0, (hipStream_t)stream, rec, pair_lp, hlens, score, ulen, count,
                     yseq, s_score, s_src, nS, par, reinterpret_cast<long long*>(tok), live, hidx, pairs, n, W, V, T, N, alpha, t, v, p);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
