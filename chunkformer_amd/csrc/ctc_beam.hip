// CTC prefix beam search (modules/search.py:131-249 with score() = log_add([s, ns])) on device:
//   ctc_topk_kernel   per-row top-k of logit - lse (or of log-probs), one wave per row, the row held
//                     as order-preserving integer keys in registers (V <= 5120) or re-read;
//   ctc_beam_kernel   the search, one workgroup per utterance, scores in f64.
//
// Hypothesis identity and token times are the PrefixTrie of beam.h (trie, map and time lists, one region per
// utterance in the workspace): a prefix is identified by its node id, an extension by the looked-up node
// or, when there is none, by its own slot (hypothesis, token) - two extensions never name the same new
// prefix.  A time list is copied by sharing its entry; an append or a replace-last makes the survivor's
// one entry.
//
// A frame: (1) one thread per (hypothesis, token) extension looks the child up; an extension whose
// child is in the beam is folded into that hypothesis' own slot, the others are candidates of their
// own; (2) one thread per hypothesis forms its unchanged-prefix candidate from the blank, the
// repeated token and the folded extension in the reference's visiting order (tokens in top-k order,
// hypotheses in beam order); (3) rank by counting on (total score descending, first created first),
// the first k are the new beam and insert their nodes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cfm.h"
#include "beam.h"
#include "cfm_common.h"
#include "cfm_kernels.h"
#include "status.h"
#include "workspace.h"

namespace cfm {

// ----------------------------------------------------------------------------- top-k
// One wave per row.  NPL > 0: the row in NPL registers per lane (V <= 64 * NPL), read once; NPL == 0: every
// pass re-reads the row.  lse is formed exactly as log_softmax_kernel (misc.hip) forms it, and the
// selection orders the VALUES written (logit - lse: two logits can round to one log-prob, and then the
// lower index comes first) as order-preserving integer keys.
//
// Selection by the rounds of beam.h (TopKRound).  Over the whole row that is k passes; for NPL > 4 the
// rounds run over a short candidate list instead: t0 = the k-th largest of the 64 per-lane maxima (at
// least k elements are >= t0, so every element of the top-k is), found by building t0 bit by bit from
// ballots; the elements >= t0 are appended to the wave's LDS list (their order there does not matter),
// typically k .. 2k of them.  A row with more than TOPK_CAND of them takes the whole-row rounds.
constexpr int TOPK_CAND = 256;

template <int NPL>
__global__ __launch_bounds__(256) void ctc_topk_kernel(const float* __restrict__ x, int M, int V, int k, int with_lse,
                                                       float* __restrict__ vals, int32_t* __restrict__ ids) {
  constexpr bool kList = NPL > 4;
  __shared__ uint32_t l_key[kList ? 4 : 1][kList ? TOPK_CAND : 1];
  __shared__ int l_idx[kList ? 4 : 1][kList ? TOPK_CAND : 1];
  __shared__ int l_cnt[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row_raw = blockIdx.x * 4 + w;
  if (!kList && row_raw >= M) return;
  const bool live = row_raw < M;            // the list path keeps every wave for the block barriers
  const int row = live ? row_raw : M - 1;
  const float* p = x + (size_t)row * V;
  constexpr int NR = NPL > 0 ? NPL : 1;
  float val[NR];
  uint32_t key[NR];
  float lse = 0.f;
  if constexpr (NPL > 0) {
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int v = lane + 64 * i;
      val[i] = v < V ? p[v] : -INFINITY;
    }
  }
  if (with_lse) {
    float mx = -INFINITY;
    if constexpr (NPL > 0) {
#pragma unroll
      for (int i = 0; i < NPL; ++i)
        if (lane + 64 * i < V && val[i] > mx) mx = val[i];
    } else {
      for (int v = lane; v < V; v += 64) { const float t = p[v]; if (t > mx) mx = t; }
    }
    mx = wave_max(mx);
    float s = 0.f;
    if constexpr (NPL > 0) {
#pragma unroll
      for (int i = 0; i < NPL; ++i)
        if (lane + 64 * i < V) s += __expf(val[i] - mx);
    } else {
      for (int v = lane; v < V; v += 64) s += __expf(p[v] - mx);
    }
    lse = mx + __logf(wave_sum(s));
  }
  if constexpr (NPL > 0) {
#pragma unroll
    for (int i = 0; i < NPL; ++i) key[i] = lane + 64 * i < V ? f2key(with_lse ? val[i] - lse : val[i]) : 0u;
  }

  int n_list = -1;   // >= 0: the rounds run over the wave's candidate list
  uint32_t ck[TOPK_CAND / 64];
  int ci[TOPK_CAND / 64];
  if constexpr (kList) {
    uint32_t lm = 0u;   // this lane's largest key (V > 256 here: every lane holds valid elements)
#pragma unroll
    for (int i = 0; i < NPL; ++i) lm = key[i] > lm ? key[i] : lm;
    uint32_t t0 = 0u;   // the largest t with at least k lane maxima >= t
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t c = t0 | (1u << bit);
      if (__popcll(__ballot(lm >= c)) >= k) t0 = c;
    }
    if (lane == 0) l_cnt[w] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      if (lane + 64 * i < V && key[i] >= t0) {
        const int at = atomicAdd(&l_cnt[w], 1);
        if (at < TOPK_CAND) { l_key[w][at] = key[i]; l_idx[w][at] = lane + 64 * i; }
      }
    }
    __syncthreads();
    const int c = l_cnt[w];
    if (c <= TOPK_CAND) {
      n_list = c;
#pragma unroll
      for (int q = 0; q < TOPK_CAND / 64; ++q) {
        const int j = lane + 64 * q;
        ck[q] = j < c ? l_key[w][j] : 0u;
        ci[q] = j < c ? l_idx[w][j] : TOPK_NONE;
      }
    }
  }
  if (!live) return;

  TopKRound top;
  for (int r = 0; r < k; ++r) {
    if (kList && n_list >= 0) {
#pragma unroll
      for (int q = 0; q < TOPK_CAND / 64; ++q)
        if (lane + 64 * q < n_list) top.see(ck[q], ci[q]);
    } else if constexpr (NPL > 0) {
#pragma unroll
      for (int i = 0; i < NPL; ++i)
        if (lane + 64 * i < V) top.see(key[i], lane + 64 * i);
    } else {
      for (int v = lane; v < V; v += 64) top.see(f2key(with_lse ? p[v] - lse : p[v]), v);
    }
    top.reduce64();
    if (lane == 0) {
      vals[(size_t)row * k + r] = key2f(top.bk);
      ids[(size_t)row * k + r] = top.bi;
    }
    top.next();
  }
}

int ctc_topk_rows(const float* x, int M, int V, int k, int with_lse, float* vals, int32_t* ids, hipStream_t st) {
  if (M <= 0) return 0;
  const dim3 g((M + 3) / 4), b(256);
  if (V <= 64) hipLaunchKernelGGL(ctc_topk_kernel<1>, g, b, 0, st, x, M, V, k, with_lse, vals, ids);
  else if (V <= 256) hipLaunchKernelGGL(ctc_topk_kernel<4>, g, b, 0, st, x, M, V, k, with_lse, vals, ids);
  else if (V <= 1024) hipLaunchKernelGGL(ctc_topk_kernel<16>, g, b, 0, st, x, M, V, k, with_lse, vals, ids);
  else if (V <= 5120) hipLaunchKernelGGL(ctc_topk_kernel<80>, g, b, 0, st, x, M, V, k, with_lse, vals, ids);
  else hipLaunchKernelGGL(ctc_topk_kernel<0>, g, b, 0, st, x, M, V, k, with_lse, vals, ids);
  CFM_CHECK_LAUNCH();
  return 0;
}

// ----------------------------------------------------------------------------- context graph tables
struct CtxTables {
  int n_nodes;
  const int32_t *fail, *trans_off, *trans_tok, *trans_next;
  const double *token_score, *node_score, *output_score;
};

CFM_DEV int ctx_find(const CtxTables& c, int node, int tok) {
  int lo = c.trans_off[node];
  const int end = c.trans_off[node + 1];
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c.trans_tok[mid] < tok) lo = mid + 1; else hi = mid;
  }
  return (lo < end && c.trans_tok[lo] == tok) ? c.trans_next[lo] : -1;
}

// forward_one_step (context_graph.py:215-254): the arc if there is one, else along the fail arcs to a
// node with the arc or to the root; at most n_nodes steps
CFM_DEV double ctx_step(const CtxTables& c, int state, int tok, int* next) {
  const int n = ctx_find(c, state, tok);
  if (n >= 0) { *next = n; return c.token_score[n] + c.output_score[n]; }
  int node = c.fail[state];
  for (int g = 0; g < c.n_nodes; ++g) {
    const int m = ctx_find(c, node, tok);
    if (m >= 0) { node = m; break; }
    if (node == 0) break;
    node = c.fail[node];
  }
  *next = node;
  return (c.node_score[node] - c.node_score[state]) + c.output_score[node];
}

// ----------------------------------------------------------------------------- beam search
constexpr int CMAX = BEAM_KMAX * (BEAM_KMAX + 1);

// The total a candidate is ranked by.  NaN (from a NaN or +inf log-prob) compares false both ways and
// would give several candidates one rank, so it is ranked as -inf and the error word is set: the
// totals then are never NaN, the creation-order keys are distinct, (total descending, key ascending)
// is a strict total order, and the ranks of n_valid candidates are exactly 0 .. n_valid - 1 - every beam
// slot below min(k, n_valid) is written once before it is read.
CFM_DEV double rank_key(double total, int32_t* err) {
  if (total != total) { err[0] = BEAM_ERR_NAN; return NINF; }
  return total;
}

struct BeamArgs {
  const float* vals;
  const int32_t* ids;
  const int32_t *row_start, *row_len;
  int rows, k, blank, has_ctx, with_times;
  CtxTables ctx;
  int32_t *out_tok, *out_time, *out_len, *n_hyps;
  double* out_score;
  int32_t* err;
  TrieRegions trie;
};

__global__ __launch_bounds__(256) void ctc_beam_kernel(const BeamArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, K = a.k;
  const int start = a.row_start[b], len = a.row_len[b];
  if (start < 0 || len < 0 || (long long)start + len > a.rows) {
    if (tid == 0) a.err[0] = BEAM_ERR_RANGE;
    return;
  }
  const PrefixTrie trie(a.trie, K, start, len, a.with_times);

  // the beam
  constexpr int KM = BEAM_KMAX;
  __shared__ int b_node[KM], b_tok[KM], b_ts[KM], b_tns[KM], b_tim[KM], b_cst[KM];
  __shared__ double b_s[KM], b_ns[KM], b_vs[KM], b_vns[KM], b_sc[KM], b_vit[KM], b_csc[KM];
  // the frame's candidates: slot h = hypothesis h unchanged, slot n + h * K + j = h extended by token j
  __shared__ int c_valid[CMAX], c_node[CMAX], c_par[CMAX], c_tok[CMAX], c_ts[CMAX], c_tnb[CMAX], c_tnm[CMAX],
      c_cst[CMAX], c_ord[CMAX];
  __shared__ double c_s[CMAX], c_ns[CMAX], c_vs[CMAX], c_vns[CMAX], c_csc[CMAX], c_tot[CMAX];
  __shared__ int tk_u[KM], merge_h[KM], n_valid;
  __shared__ double tk_p[KM];

  for (int i = tid; i < trie.cap; i += 256) trie.map[i] = 0;
  if (tid == 0) {
    b_node[0] = 0; b_tok[0] = -1; b_ts[0] = 0; b_tns[0] = 0; b_tim[0] = 0; b_cst[0] = 0;
    b_s[0] = 0.0; b_ns[0] = NINF; b_vs[0] = 0.0; b_vns[0] = 0.0; b_sc[0] = 0.0; b_vit[0] = 0.0; b_csc[0] = 0.0;
  }
  int n = 1;
  bool failed = false;
  __syncthreads();

  for (int t = 0; t < len; ++t) {
    const int ncand = n * (K + 1);
    if (tid < K) {
      tk_u[tid] = a.ids[(size_t)(start + t) * K + tid];
      tk_p[tid] = (double)a.vals[(size_t)(start + t) * K + tid];
      merge_h[tid] = -1;
    }
    if (tid == 0) n_valid = 0;
    for (int i = tid; i < ncand; i += 256) c_valid[i] = 0;
    __syncthreads();

    // (1) extensions
    if (tid < n * K) {
      const int h = tid / K, j = tid - h * K, u = tk_u[j];
      if (u != a.blank) {
        const int child = trie.find(b_node[h], u);
        int target = -1;
        if (child > 0)
          for (int h2 = 0; h2 < n; ++h2)
            if (b_node[h2] == child) target = h2;
        if (target >= 0) {
          merge_h[target] = h;   // the one hypothesis whose node is the parent of b_node[target]
        } else {
          const int c = n + tid;
          const double p = tk_p[j];
          const bool rep = u == b_tok[h];   // *u-u -> *uu: from the blank-ending paths only
          const double x = (rep ? b_s[h] : b_sc[h]) + p, v = (rep ? b_vs[h] : b_vit[h]) + p;
          c_s[c] = NINF; c_vs[c] = NINF; c_ts[c] = 0;
          c_ns[c] = x;
          if (NINF < v) { c_vns[c] = v; c_tnb[c] = rep ? b_ts[h] : b_tim[h]; c_tnm[c] = 1; }
          else { c_vns[c] = NINF; c_tnb[c] = 0; c_tnm[c] = 0; }
          int cst = 0;
          double csc = 0.0;
          if (a.has_ctx) csc = b_csc[h] + ctx_step(a.ctx, b_cst[h], u, &cst);
          c_cst[c] = cst; c_csc[c] = csc;
          c_node[c] = child > 0 ? child : -1; c_par[c] = b_node[h]; c_tok[c] = u;
          c_ord[c] = (j * K + h) * 2 + 1;
          c_tot[c] = rank_key(x + csc, a.err);
          c_valid[c] = 1;
          atomicAdd(&n_valid, 1);
        }
      }
    }
    __syncthreads();

    // (2) unchanged prefixes
    if (tid < n) {
      const int h = tid, mh = merge_h[h];
      int jb = -1, jl = -1;
      for (int j = 0; j < K; ++j) {
        if (tk_u[j] == a.blank) { if (jb < 0) jb = j; }
        else if (tk_u[j] == b_tok[h] && jl < 0) jl = j;
      }
      if (jb >= 0 || jl >= 0) {
        double s = NINF, vs = NINF, ns = NINF, vns = NINF, cur = NINF;
        int ts = 0, tnb = 0, tnm = 0, ord = 0x7fffffff;
        if (jb >= 0) {
          s = b_sc[h] + tk_p[jb]; vs = b_vit[h] + tk_p[jb]; ts = b_tim[h];
          ord = (jb * K + h) * 2;
        }
        if (jl >= 0) {
          const double p = tk_p[jl];
          auto folded = [&]() {   // the extension of hypothesis mh by this token
            const bool rep = tk_u[jl] == b_tok[mh];
            const double x = (rep ? b_s[mh] : b_sc[mh]) + p, v = (rep ? b_vs[mh] : b_vit[mh]) + p;
            ns = log_add(ns, x);
            if (vns < v) { vns = v; cur = p; tnb = rep ? b_ts[mh] : b_tim[mh]; tnm = 1; }
          };
          if (mh >= 0 && mh < h) folded();
          ns = log_add(ns, b_ns[h] + p);   // *uu -> *u
          if (vns < b_vns[h] + p) {
            vns = b_vns[h] + p;
            if (cur < p) { cur = p; tnb = b_tns[h]; tnm = 2; }
          }
          if (mh >= 0 && mh > h) folded();
          const int o1 = (jl * K + h) * 2, o2 = mh >= 0 ? (jl * K + mh) * 2 + 1 : 0x7fffffff;
          ord = min(ord, min(o1, o2));
        }
        c_s[h] = s; c_vs[h] = vs; c_ts[h] = ts; c_ns[h] = ns; c_vns[h] = vns; c_tnb[h] = tnb; c_tnm[h] = tnm;
        c_cst[h] = b_cst[h]; c_csc[h] = b_csc[h];
        c_node[h] = b_node[h]; c_par[h] = -1; c_tok[h] = b_tok[h];
        c_ord[h] = ord;
        c_tot[h] = rank_key(log_add(s, ns) + b_csc[h], a.err);
        c_valid[h] = 1;
        atomicAdd(&n_valid, 1);
      }
    }
    __syncthreads();

    // (3) prune: rank by (total descending, first created first); the first K are the new beam.  The
    // creation keys are distinct: an extension's is odd and names its own (hypothesis, token); an
    // unchanged prefix's is even and names its hypothesis, or is the odd key of the one extension folded
    // into it, whose own slot is then not a candidate.
    for (int i = tid; i < ncand; i += 256) {
      if (!c_valid[i]) continue;
      const double ti = c_tot[i];
      const int oi = c_ord[i];
      int rank = 0;
      for (int j = 0; j < ncand; ++j)
        if (c_valid[j] && (c_tot[j] > ti || (c_tot[j] == ti && c_ord[j] < oi))) ++rank;
      if (rank >= K) continue;
      const int fresh = 1 + t * K + rank;   // this survivor's node id, in the trie and in the time lists
      int node = c_node[i];
      if (node < 0) {
        node = fresh;
        if (!trie.insert(node, c_par[i], c_tok[i])) a.err[0] = BEAM_ERR_MAP;
      }
      int tns = 0;
      if (a.with_times && c_tnm[i] != 0) {
        const int base = c_tnb[i];
        tns = fresh;
        trie.time_append(tns, c_tnm[i] == 1 ? base : (base > 0 ? trie.tprev[base - 1] : 0), t);   // append / replace-last
      }
      const double s = c_s[i], ns = c_ns[i], vs = c_vs[i], vns = c_vns[i];
      b_node[rank] = node; b_tok[rank] = c_tok[i]; b_ts[rank] = c_ts[i]; b_tns[rank] = tns;
      b_tim[rank] = vs > vns ? c_ts[i] : tns;
      b_cst[rank] = c_cst[i]; b_csc[rank] = c_csc[i];
      b_s[rank] = s; b_ns[rank] = ns; b_vs[rank] = vs; b_vns[rank] = vns;
      b_sc[rank] = log_add(s, ns); b_vit[rank] = vs > vns ? vs : vns;
    }
    __syncthreads();
    n = min(K, n_valid);
    if (n < 1) { failed = true; break; }   // cannot happen: every token gives hypothesis 0 a candidate
    __syncthreads();
  }
  if (failed) {
    if (tid == 0) a.err[0] = BEAM_ERR_EMPTY;
    return;
  }

  // n-best in beam order (finalize replaces the context score and does not re-sort, search.py:227-235)
  if (tid == 0) a.n_hyps[b] = n;
  if (tid < K) {
    int L = 0;
    double score = 0.0;
    if (tid < n) {
      const double csc = a.has_ctx ? -a.ctx.node_score[b_cst[tid]] : b_csc[tid];
      score = b_sc[tid] + csc;
      // (the walks of PrefixTrie::tokens / frames, written out: calling them measured 1% slower per frame here)
      for (int nd = b_node[tid]; nd > 0 && L < len; nd = trie.par[nd - 1]) ++L;
      int32_t* ot = a.out_tok + (size_t)tid * a.rows + start;
      int i = L;
      for (int nd = b_node[tid]; nd > 0 && i > 0; nd = trie.par[nd - 1]) ot[--i] = trie.tok[nd - 1];
      if (a.with_times && a.out_time) {
        int32_t* om = a.out_time + (size_t)tid * a.rows + start;
        i = L;
        for (int tn = b_tim[tid]; tn > 0 && i > 0; tn = trie.tprev[tn - 1]) om[--i] = trie.tframe[tn - 1];
        while (i > 0) om[--i] = -1;
      }
    }
    a.out_len[(size_t)b * K + tid] = L;
    a.out_score[(size_t)b * K + tid] = score;
  }
}

}  // namespace cfm

// ----------------------------------------------------------------------------- C ABI
using namespace cfm;

struct cfm_ctx {
  int device = 0;
  void* block = nullptr;
  CtxTables t{};
};


cfm_status cfm_ctx_create(int32_t n_nodes, const int32_t* fail, const double* token_score, const double* node_score,
                          const double* output_score, int32_t n_trans, const int32_t* trans_node,
                          const int32_t* trans_token, const int32_t* trans_next, int32_t device, cfm_ctx** out) {
  if (!out || !fail || !token_score || !node_score || !output_score) return set_error(CFM_ERR_VALUE, "null argument");
  if (n_nodes < 1 || n_trans < 0 || (n_trans > 0 && (!trans_node || !trans_token || !trans_next)))
    return set_error(CFM_ERR_VALUE, "context graph: at least the root, and n_trans transitions");
  std::vector<int32_t> off(n_nodes + 1, 0);
  for (int i = 0; i < n_trans; ++i) {
    const bool sorted = i == 0 || trans_node[i] > trans_node[i - 1] ||
                        (trans_node[i] == trans_node[i - 1] && trans_token[i] > trans_token[i - 1]);
    if (trans_node[i] < 0 || trans_node[i] >= n_nodes || trans_next[i] < 1 || trans_next[i] >= n_nodes || !sorted)
      return set_error(CFM_ERR_VALUE, "context graph: transitions must be sorted by (node, token) and name valid nodes");
    off[trans_node[i] + 1]++;
  }
  for (int i = 0; i < n_nodes; ++i) {
    if (fail[i] < 0 || fail[i] >= n_nodes) return set_error(CFM_ERR_VALUE, "context graph: bad fail arc");
    off[i + 1] += off[i];
  }
  const size_t nI = align_up((size_t)n_nodes * 4), nO = align_up((size_t)(n_nodes + 1) * 4),
               nT = align_up((size_t)n_trans * 4 + 4), nD = align_up((size_t)n_nodes * 8);
  const size_t total = nI + nO + 2 * nT + 3 * nD;
  std::vector<char> img(total, 0);
  size_t o = 0;
  auto put = [&](const void* src, size_t bytes, size_t padded) {
    if (bytes) std::memcpy(img.data() + o, src, bytes);
    const size_t at = o;
    o += padded;
    return at;
  };
  const size_t oF = put(fail, (size_t)n_nodes * 4, nI), oO = put(off.data(), (size_t)(n_nodes + 1) * 4, nO);
  const size_t oTt = put(trans_token, (size_t)n_trans * 4, nT), oTn = put(trans_next, (size_t)n_trans * 4, nT);
  const size_t oDs = put(token_score, (size_t)n_nodes * 8, nD), oDn = put(node_score, (size_t)n_nodes * 8, nD);
  const size_t oDo = put(output_score, (size_t)n_nodes * 8, nD);
  if (hipSetDevice(device) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipSetDevice");
  void* blk = nullptr;
  if (hipMalloc(&blk, total) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "context graph: hipMalloc");
  if (hipMemcpy(blk, img.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(blk);
    return set_error(CFM_ERR_RUNTIME, "context graph: upload");
  }
  auto* h = new cfm_ctx();
  h->device = device;
  h->block = blk;
  char* d = (char*)blk;
  h->t.n_nodes = n_nodes;
  h->t.fail = (const int32_t*)(d + oF);
  h->t.trans_off = (const int32_t*)(d + oO);
  h->t.trans_tok = (const int32_t*)(d + oTt);
  h->t.trans_next = (const int32_t*)(d + oTn);
  h->t.token_score = (const double*)(d + oDs);
  h->t.node_score = (const double*)(d + oDn);
  h->t.output_score = (const double*)(d + oDo);
  *out = h;
  return CFM_OK;
}

void cfm_ctx_destroy(cfm_ctx* h) {
  if (!h) return;
  if (h->block) (void)hipFree(h->block);
  delete h;
}

// header (error word) | the trie's regions (beam.h) for k * rows nodes
static size_t beam_carve(void* ws, int rows, int k, bool with_times, BeamArgs& a) {
  Carver c(ws);
  a.err = c.take<int32_t>(64);
  a.trie = carve_trie(c, (size_t)k * (size_t)rows, with_times);
  return c.off;
}

size_t cfm_ctc_beam_workspace_bytes(int32_t rows, int32_t B, int32_t k, int32_t with_times, int32_t n_context_nodes) {
  (void)B;
  (void)n_context_nodes;   // the context tables live in the cfm_ctx handle
  if (rows < 0 || k < 1) return 0;
  BeamArgs a{};
  return beam_carve(nullptr, rows, k, with_times != 0, a);
}

cfm_status cfm_ctc_beam_search(const float* topk_logp, const int32_t* topk_ids, int32_t rows, int32_t k,
                               const int32_t* row_start, const int32_t* row_len, int32_t B, int32_t blank_id,
                               const cfm_ctx* context, int32_t* out_tokens, int32_t* out_times, int32_t* out_len,
                               double* out_score, int32_t* n_hyps, void* ws, size_t wsb, cfm_stream stream) {
  if (B < 0 || rows < 0) return set_error(CFM_ERR_VALUE, "bad rows / B");
  if (k < 1 || k > BEAM_KMAX) return set_error(CFM_ERR_VALUE, "beam size: 1 .. 16");
  if ((size_t)k * (size_t)rows > (size_t)0x3fffffff) return set_error(CFM_ERR_VALUE, "k * rows exceeds the node id range");
  if (B == 0) return CFM_OK;
  if ((rows > 0 && (!topk_logp || !topk_ids)) || !row_start || !row_len || !out_tokens || !out_len || !out_score ||
      !n_hyps || !ws)
    return set_error(CFM_ERR_VALUE, "null argument");
  int cur_dev = -1;
  if (hipGetDevice(&cur_dev) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipGetDevice");
  if (context && context->device != cur_dev) return set_error(CFM_ERR_VALUE, "context graph lives on another device");
  const int with_times = out_times != nullptr;
  if (wsb < cfm_ctc_beam_workspace_bytes(rows, B, k, with_times, 0))
    return set_error(CFM_ERR_VALUE, "beam search workspace too small");
  BeamArgs a{};
  a.vals = topk_logp; a.ids = topk_ids; a.row_start = row_start; a.row_len = row_len;
  a.rows = rows; a.k = k; a.blank = blank_id; a.has_ctx = context != nullptr; a.with_times = with_times;
  if (context) a.ctx = context->t;
  a.out_tok = out_tokens; a.out_time = out_times; a.out_len = out_len; a.out_score = out_score; a.n_hyps = n_hyps;
  beam_carve(ws, rows, k, with_times, a);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(ws, 0, 256, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(B), dim3(256), 0, st, a);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return set_error(CFM_ERR_RUNTIME, std::string("beam search: ") + hipGetErrorString(e));
  return CFM_OK;
}

cfm_status cfm_ctc_topk_logp(const float* logp, int32_t rows, int32_t V, int32_t k, float* topk_logp, int32_t* topk_ids,
                             cfm_stream stream) {
  if (rows < 0 || V < 1) return set_error(CFM_ERR_VALUE, "bad rows / V");
  if (k < 1 || k > BEAM_KMAX || k > V) return set_error(CFM_ERR_VALUE, "top-k: 1 <= k <= 16 and k <= V");
  if (rows == 0) return CFM_OK;
  if (!logp || !topk_logp || !topk_ids) return set_error(CFM_ERR_VALUE, "null argument");
  const int e = ctc_topk_rows(logp, rows, V, k, 0, topk_logp, topk_ids, (hipStream_t)stream);
  if (e) return set_error(CFM_ERR_RUNTIME, std::string("top-k: ") + hipGetErrorString((hipError_t)e));
  return CFM_OK;
}
