// Transducer prefix beam search (transducer/search/prefix_beam_search.py:41-146, the reference's mode
// rnnt_beam_search) over the cfm_rnnt handle, every utterance of a packed batch at once, shallow-fused with the CTC
// posterior of the frame: logp = log(tw * p_rnnt + cw * p_ctc).
//
// Rows: r = b * K + k (utterance b, beam slot k), R = B * K.  Frame t = 0 .. max(row_len) - 1; all utterances step
// together and an utterance with row_len <= t is left untouched by every kernel.  One frame is a fixed sequence of
// ordinary launches, none of which waits for another workgroup:
//
//   rb_embed_kernel        x = embed[last token] into the first LSTM layer's [x | h] input row
//   per LSTM layer         gemm<float> [x | h] . [W_ih | W_hh]^T + b  ->  rb_cell_kernel (new h, c; h is the next x)
//   gemm<float>            composed projection + pred_ffn of the top layer's h
//   rb_joint_in_kernel     z = tanh(enc_proj[row(b, t)] + pred)
//   gemm<float>            ffn_out: logits [R, V]
//   rb_fuse_topk_kernel    one workgroup per row: log-softmax, CTC fusion, top K (value descending, index ascending)
//   rb_prune_kernel        one workgroup per utterance: expansion, prefix fusion, second prune
//   rb_gather_kernel       the survivors' LSTM state by parent slot (the new state for an appended token, the old one
//                          for an unchanged hypothesis) into the other of two buffers
//
// A stateless handle (embedding / conv predictor) replaces the embed .. projection launches by sl_ctx_kernel (the slot's
// Kc context rows mixed into x), the ffn gemm<float> (embedding only), sl_norm_act_kernel and the pred_ffn gemm<float>,
// and rb_gather_kernel by sl_gather_kernel, which moves Kc - 1 int32 ids per slot (nothing with history_size 0).
//
// The predictor is evaluated for every live hypothesis at every frame, as the reference does; an unchanged
// hypothesis keeps its old state, so its next evaluation repeats the same values.
//
// Hypothesis identity and token times are the PrefixTrie of beam.h: a prefix has one node id however often it leaves
// and re-enters the beam, and an appended token makes the survivor's one time entry.  Every loop is bounded by a
// launch argument or a validated length; the error word (first word of the workspace) is set where the reference has
// no answer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cfm.h"
#include "../../include/cfm_ops.h"
#include "beam.h"
#include "cfm_common.h"
#include "cfm_kernels.h"
#include "rnnt.h"
#include "rnnt_beam.h"
#include "status.h"
#include "workspace.h"

namespace cfm {

constexpr int RB_CMAX = BEAM_KMAX * BEAM_KMAX;
constexpr int RB_LDS_KEYS = 8192;   // rows up to this many columns keep their fused keys in LDS

CFM_DEV bool rb_live(const RbLive& lv, int r, int* src_row) {
  if (!lv.ulen) { *src_row = r; return true; }
  const int b = r / lv.K, k = r - b * lv.K;
  if (lv.t >= lv.ulen[b] || k >= lv.n[b]) return false;
  *src_row = lv.ustart[b] + lv.t;
  return true;
}

__global__ __launch_bounds__(64) void rb_init_kernel(const int32_t* __restrict__ row_start,
                                                     const int32_t* __restrict__ row_len, int B, int K, int rows,
                                                     int max_len, int blank, int32_t* __restrict__ err,
                                                     int32_t* __restrict__ ustart, int32_t* __restrict__ ulen,
                                                     int32_t* __restrict__ n, int32_t* __restrict__ node,
                                                     int32_t* __restrict__ tok, int32_t* __restrict__ tptr,
                                                     double* __restrict__ score) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int s = row_start[b], len = row_len[b];
  if (s < 0 || len < 0 || s > rows || len > rows - s || len > max_len) {
    err[0] = BEAM_ERR_RANGE;
    s = 0;
    len = 0;
  }
  ustart[b] = s;
  ulen[b] = len;
  n[b] = 1;
  node[b * K] = 0;
  tok[b * K] = blank;
  tptr[b * K] = 0;
  score[b * K] = 0.0;
}

__global__ void rb_set_kernel(int32_t* p, int32_t v) { *p = v; }

__global__ __launch_bounds__(64) void rb_embed_kernel(RbLive lv, const int32_t* __restrict__ tok,
                                                      const float* __restrict__ embed, int V, int E,
                                                      float* __restrict__ xh, int ld) {
  const int r = blockIdx.x;
  int src;
  if (!rb_live(lv, r, &src)) return;
  const int tk = min(max(tok[r], 0), V - 1);
  const float4* e = reinterpret_cast<const float4*>(embed + (size_t)tk * E);
  float4* o = reinterpret_cast<float4*>(xh + (size_t)r * ld);
  for (int c = threadIdx.x; c < (E >> 2); c += 64) o[c] = e[c];
}

CFM_DEV float rb_sigm(float x) { return 1.f / (1.f + expf(-x)); }

// torch LSTM gate order i, f, g, o: c' = f c + i g, h' = o tanh(c'); h' also goes to `next` (the next layer's x)
__global__ __launch_bounds__(128) void rb_cell_kernel(RbLive lv, const float* __restrict__ gates, int H,
                                                      const float* __restrict__ c_old, float* __restrict__ c_new,
                                                      float* __restrict__ h_new, float* __restrict__ next, int next_ld) {
  const int r = blockIdx.x;
  int src;
  if (!rb_live(lv, r, &src)) return;
  const float* g = gates + (size_t)r * 4 * H;
  for (int e = threadIdx.x; e < H; e += 128) {
    const float ig = rb_sigm(g[e]), fg = rb_sigm(g[H + e]), gg = tanhf(g[2 * H + e]), og = rb_sigm(g[3 * H + e]);
    const float cv = fg * c_old[(size_t)r * H + e] + ig * gg;
    const float hv = og * tanhf(cv);
    c_new[(size_t)r * H + e] = cv;
    h_new[(size_t)r * H + e] = hv;
    if (next) next[(size_t)r * next_ld + e] = hv;
  }
}

__global__ __launch_bounds__(128) void rb_joint_in_kernel(RbLive lv, const float* __restrict__ enc_proj,
                                                          const float* __restrict__ pj, int J, float* __restrict__ z) {
  const int r = blockIdx.x;
  int src;
  if (!rb_live(lv, r, &src)) return;
  for (int j = threadIdx.x; j < J; j += 128)
    z[(size_t)r * J + j] = tanhf(enc_proj[(size_t)src * J + j] + pj[(size_t)r * J + j]);
}

// ----------------------------------------------------------------------------- the stateless predictors
// One workgroup per live row: the row's Kc context rows (id -1: a zero vector) and their mix into x.  embedding:
// x = sum_c (c_c . q_c) c_c / (n_head Kc), each dot product by one wave; conv: x[d] = sum_c tap[c][d] c_c[d] (+ bias).
__global__ __launch_bounds__(256) void sl_ctx_kernel(RbLive lv, RnntDev w, const int32_t* __restrict__ hist, int hist_ld,
                                                     const int32_t* __restrict__ last, int last_ld,
                                                     int32_t* __restrict__ ptok, float* __restrict__ x) {
  extern __shared__ float sl_rows[];   // [Kc][E], then [16] dot products
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int src;
  if (!rb_live(lv, r, &src)) return;
  const int E = w.E, Kc = w.Kc;
  float* dots = sl_rows + Kc * E;
  const int lt = last[(size_t)r * last_ld];
  if (ptok && tid == 0) ptok[r] = lt;
  for (int e = tid; e < Kc * E; e += 256) {
    const int c = e / E, d = e - c * E;
    const int id = c == Kc - 1 ? lt : hist[(size_t)r * hist_ld + c];
    sl_rows[e] = id >= 0 ? w.embed[(size_t)min(id, w.V - 1) * E + d] : 0.f;
  }
  __syncthreads();
  if (w.kind == CFM_RNNT_PRED_EMBEDDING) {
    for (int c = wid; c < Kc; c += 4) {
      float s = 0.f;
      for (int d = lane; d < E; d += 64) s = fmaf(sl_rows[c * E + d], w.tap[c * E + d], s);
      s = wave_sum(s);
      if (lane == 0) dots[c] = s;
    }
    __syncthreads();
    for (int d = tid; d < E; d += 256) {
      float a = 0.f;
      for (int c = 0; c < Kc; ++c) a = fmaf(dots[c], sl_rows[c * E + d], a);
      x[(size_t)r * E + d] = a / w.mix_div;
    }
  } else {
    for (int d = tid; d < E; d += 256) {
      float a = 0.f;
      for (int c = 0; c < Kc; ++c) a = fmaf(w.tap[c * E + d], sl_rows[c * E + d], a);
      x[(size_t)r * E + d] = w.cbias ? a + w.cbias[d] : a;
    }
  }
}

// y = act(LayerNorm(v)) per live row (two passes: the mean, then the variance about it), one workgroup per row.
// v may be y (the embedding kind runs it in place on the ffn output): element d is read and written by one thread only.
__global__ __launch_bounds__(256) void sl_norm_act_kernel(RbLive lv, RnntDev w, const float* v, float* y) {
  __shared__ float s_red[8];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int src;
  if (!rb_live(lv, r, &src)) return;
  const int E = w.E;
  const float* in = v + (size_t)r * E;
  float s = 0.f;
  for (int d = tid; d < E; d += 256) s += in[d];
  s = wave_sum(s);
  if (lane == 0) s_red[wid] = s;
  __syncthreads();
  const float mean = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) / (float)E;
  float q = 0.f;
  for (int d = tid; d < E; d += 256) { const float dd = in[d] - mean; q = fmaf(dd, dd, q); }
  q = wave_sum(q);
  if (lane == 0) s_red[4 + wid] = q;
  __syncthreads();
  const float rstd = 1.f / sqrtf(((s_red[4] + s_red[5]) + (s_red[6] + s_red[7])) / (float)E + w.ln_eps);
  for (int d = tid; d < E; d += 256)
    y[(size_t)r * E + d] = rnnt_act(w.act, (in[d] - mean) * rstd * w.gamma[d] + w.beta[d]);
}

// the survivors' id history: slot k < n[b] takes its parent's window shifted by the parent's last token (a token was
// appended) or the parent's history as it was.  hl = Kc - 1 >= 1 ids per slot.
__global__ __launch_bounds__(64) void sl_gather_kernel(RbLive lv, const int32_t* __restrict__ par,
                                                       const int32_t* __restrict__ chg, int R, int hl,
                                                       const int32_t* __restrict__ h_old,
                                                       const int32_t* __restrict__ ptok, int32_t* __restrict__ h_out) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  int src;
  if (r >= R || !rb_live(lv, r, &src)) return;
  const int b = r / lv.K;
  const int rp = b * lv.K + min(max(par[r], 0), lv.K - 1);
  const bool ch = chg[r] != 0;
  for (int c = 0; c < hl; ++c) {
    int v;
    if (!ch) v = h_old[(size_t)rp * hl + c];
    else v = c + 1 < hl ? h_old[(size_t)rp * hl + c + 1] : ptok[rp];
    h_out[(size_t)r * hl + c] = v;
  }
}

// ----------------------------------------------------------------------------- log-softmax + CTC fusion + top K
// One workgroup per row.  lp = (x - max) - log(sum exp(x - max)) as torch.log_softmax forms it, then
// f = log(tw exp(lp) + cw exp(ctc)) (no CTC row: the second term is 0), all f32.  The K largest f by (value
// descending, index ascending) are taken in K rounds over order-preserving keys: round q takes the largest key that
// comes after round q - 1's pick in that order, so nothing is marked or moved (the rounds of beam.h's TopKRound,
// written out here: with TopKRound this kernel measured 0.1% slower on a one-utterance search, where its latency is on
// the critical path of every frame).  The keys are formed once into LDS (V <= RB_LDS_KEYS) or formed again in every
// round; the fused row is never written to memory.
__global__ __launch_bounds__(256) void rb_fuse_topk_kernel(RbLive lv, const float* __restrict__ logits,
                                                           const float* __restrict__ ctc, int V, int K, float cw,
                                                           float tw, float* __restrict__ vals, int32_t* __restrict__ ids,
                                                           float* __restrict__ tr_v, int32_t* __restrict__ tr_i) {
  extern __shared__ uint32_t rb_keys[];
  __shared__ float s_red[4];
  __shared__ uint32_t s_k[2][4];
  __shared__ int s_i[2][4];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int src;
  if (!rb_live(lv, r, &src)) return;
  const float* x = logits + (size_t)r * V;
  const float* c = ctc ? ctc + (size_t)src * V : nullptr;
  float mx = -INFINITY;
  for (int v = tid; v < V; v += 256) mx = fmaxf(mx, x[v]);
  mx = wave_max(mx);
  if (lane == 0) s_red[wid] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int v = tid; v < V; v += 256) sum += expf(x[v] - mx);
  sum = wave_sum(sum);
  if (lane == 0) s_red[wid] = sum;
  __syncthreads();
  const float lse = logf((s_red[0] + s_red[1]) + (s_red[2] + s_red[3]));
  auto fused = [&](int v) -> uint32_t {
    const float lp = (x[v] - mx) - lse;
    const float f = logf(tw * expf(lp) + (c ? cw * expf(c[v]) : 0.f));
    return f2key(f);
  };
  const bool cached = V <= RB_LDS_KEYS;
  if (cached) {
    for (int v = tid; v < V; v += 256) rb_keys[v] = fused(v);
    __syncthreads();
  }
  uint32_t pk = 0xffffffffu;
  int pi = -1;
  for (int q = 0; q < K; ++q) {
    uint32_t bk = 0u;
    int bi = TOPK_NONE;
    for (int v = tid; v < V; v += 256) {
      const uint32_t kk = cached ? rb_keys[v] : fused(v);
      const bool after = kk < pk || (kk == pk && v > pi);
      if (after && (bi == TOPK_NONE || kk > bk)) { bk = kk; bi = v; }   // v ascends: the first of equal keys stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t ok = __shfl_xor(bk, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != TOPK_NONE && (bi == TOPK_NONE || ok > bk || (ok == bk && oi < bi))) { bk = ok; bi = oi; }
    }
    if (lane == 0) { s_k[q & 1][wid] = bk; s_i[q & 1][wid] = bi; }
    __syncthreads();
    bk = s_k[q & 1][0];
    bi = s_i[q & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const uint32_t ok = s_k[q & 1][w];
      const int oi = s_i[q & 1][w];
      if (oi != TOPK_NONE && (bi == TOPK_NONE || ok > bk || (ok == bk && oi < bi))) { bk = ok; bi = oi; }
    }
    pk = bk;
    pi = bi;
    if (tid == 0) {
      const int id = bi == TOPK_NONE ? 0 : bi;   // (K <= V: a round always finds one)
      const float f = bi == TOPK_NONE ? -INFINITY : key2f(bk);
      vals[(size_t)r * K + q] = f;
      ids[(size_t)r * K + q] = id;
      if (tr_v) {
        const size_t at = ((size_t)src * K + (r - r / K * K)) * K + q;
        tr_v[at] = f;
        tr_i[at] = id;
      }
    }
  }
}

// ----------------------------------------------------------------------------- expansion, prefix fusion, prune
struct RbBeam {
  int K, blank;
  const int32_t *ustart, *ulen;
  int32_t *err, *n, *node, *tok, *tptr, *par, *chg;
  double* score;
  TrieRegions trie;
  int32_t *tr_parent, *tr_token;                          // optional trace [rows, K]
  double* tr_score;
};

// Candidate c = h * K + j: hypothesis h with its j-th token, which is creation order (hypothesis ascending, rank
// ascending).  Blank keeps the hypothesis; a token appends.  Equal token lists can only be an extension (h, u)
// meeting the unchanged hypothesis h2 whose node is the child (node of h, u): the later of the two is dropped and
// the earlier takes log_add(earlier, later).  Each extension has at most one such partner and each unchanged
// hypothesis is the child of one (parent, token) only, so the pairs are disjoint.
__global__ __launch_bounds__(256) void rb_prune_kernel(const RbBeam a, int t, const float* __restrict__ tv,
                                                       const int32_t* __restrict__ ti) {
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K;
  const int len = a.ulen[b], start = a.ustart[b];
  if (t >= len) return;
  const PrefixTrie trie(a.trie, K, start, len, true);
  const int n = min(max(a.n[b], 1), K);
  const int ncand = n * K;

  __shared__ int b_node[BEAM_KMAX], b_tok[BEAM_KMAX], b_tptr[BEAM_KMAX];
  __shared__ double b_sc[BEAM_KMAX];
  __shared__ int c_valid[RB_CMAX], c_node[RB_CMAX], c_tok[RB_CMAX];
  __shared__ double c_raw[RB_CMAX], c_tot[RB_CMAX];
  __shared__ int n_valid;

  if (tid < n) {
    const int r = b * K + tid;
    b_node[tid] = a.node[r]; b_tok[tid] = a.tok[r]; b_tptr[tid] = a.tptr[r]; b_sc[tid] = a.score[r];
  }
  if (tid == 0) n_valid = 0;
  __syncthreads();

  // (1) candidates: score f32(hypothesis score) + logp in f32, as the reference's score tensor has it
  if (tid < ncand) {
    const int h = tid / K;
    const int u = ti[(size_t)b * K * K + tid];
    const float sc = (float)b_sc[h] + tv[(size_t)b * K * K + tid];
    double tot = (double)sc;
    if (tot != tot) { a.err[0] = BEAM_ERR_NAN; tot = NINF; }   // NaN is ranked as -inf
    c_raw[tid] = tot;
    c_tot[tid] = tot;
    c_tok[tid] = u;
    c_node[tid] = u == a.blank ? b_node[h] : trie.find(b_node[h], u);   // an extension: its node if it has one, else 0
    c_valid[tid] = 1;
  }
  __syncthreads();

  // (2) prefix fusion
  if (tid < ncand && c_tok[tid] != a.blank && c_node[tid] > 0) {
    int h2 = -1;
    for (int q = 0; q < n; ++q)
      if (b_node[q] == c_node[tid]) h2 = q;
    if (h2 >= 0) {
      int p = -1;
      for (int j = 0; j < K; ++j)
        if (c_tok[h2 * K + j] == a.blank) p = h2 * K + j;
      if (p >= 0) {
        const int first = min(tid, p), second = max(tid, p);
        c_valid[second] = 0;
        c_tot[first] = log_add(c_raw[first], c_raw[second]);
      }
    }
  }
  __syncthreads();

  // (3) second prune: rank by (total descending, creation order); the first K are the new beam
  if (tid < ncand && c_valid[tid]) {
    atomicAdd(&n_valid, 1);
    const double tot = c_tot[tid];
    int rank = 0;
    for (int j = 0; j < ncand; ++j)
      if (c_valid[j] && (c_tot[j] > tot || (c_tot[j] == tot && j < tid))) ++rank;
    if (rank < K) {
      const int h = tid / K, u = c_tok[tid], r = b * K + rank;
      const bool ext = u != a.blank;
      const int fresh = 1 + t * K + rank;   // this survivor's id, in the trie and in the time lists
      int node = c_node[tid], tp = b_tptr[h];
      if (ext) {
        if (node <= 0) {
          node = fresh;
          if (!trie.insert(node, b_node[h], u)) a.err[0] = BEAM_ERR_MAP;
        }
        tp = fresh;
        trie.time_append(tp, b_tptr[h], t);
      }
      a.node[r] = node;
      a.tok[r] = ext ? u : b_tok[h];
      a.tptr[r] = tp;
      a.score[r] = tot;
      a.par[r] = h;
      a.chg[r] = ext;
      if (a.tr_parent) {
        const size_t at = (size_t)(start + t) * K + rank;
        a.tr_parent[at] = h;
        a.tr_token[at] = u;
        a.tr_score[at] = tot;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    if (n_valid < 1) a.err[0] = BEAM_ERR_EMPTY;
    a.n[b] = min(K, max(n_valid, 1));
  }
}

// the survivors' LSTM state: slot k < n[b] takes its parent's new state (a token was appended) or old state
__global__ __launch_bounds__(128) void rb_gather_kernel(RbLive lv, const int32_t* __restrict__ par,
                                                        const int32_t* __restrict__ chg, int H,
                                                        const float* __restrict__ h_old, int h_old_ld,
                                                        const float* __restrict__ h_new, float* __restrict__ h_out,
                                                        int h_out_ld, const float* __restrict__ c_old,
                                                        const float* __restrict__ c_new, float* __restrict__ c_out) {
  const int r = blockIdx.x;
  int src;
  if (!rb_live(lv, r, &src)) return;
  const int b = r / lv.K;
  const int rp = b * lv.K + min(max(par[r], 0), lv.K - 1);
  const bool ch = chg[r] != 0;
  for (int e = threadIdx.x; e < H; e += 128) {
    h_out[(size_t)r * h_out_ld + e] = ch ? h_new[(size_t)rp * H + e] : h_old[(size_t)rp * h_old_ld + e];
    c_out[(size_t)r * H + e] = ch ? c_new[(size_t)rp * H + e] : c_old[(size_t)rp * H + e];
  }
}

// One thread per final slot: tokens by walking the trie, frames by walking the time list (PrefixTrie's finish walks)
__global__ __launch_bounds__(64) void rb_finish_kernel(const RbBeam a, int rows, int32_t* __restrict__ out_tok,
                                                       int32_t* __restrict__ out_time, int32_t* __restrict__ out_len,
                                                       double* __restrict__ out_score, int32_t* __restrict__ n_hyps) {
  const int b = blockIdx.x, k = threadIdx.x, K = a.K;
  const int len = a.ulen[b], start = a.ustart[b];
  const int n = min(max(a.n[b], 1), K);
  if (k == 0) n_hyps[b] = n;
  if (k >= K) return;
  int L = 0;
  double score = 0.0;
  if (k < n) {
    const PrefixTrie trie(a.trie, K, start, len, true);
    const int r = b * K + k;
    score = a.score[r];
    L = trie.tokens(a.node[r], out_tok + (size_t)k * rows + start);
    trie.frames(a.tptr[r], L, out_time + (size_t)k * rows + start);
  }
  out_len[(size_t)b * K + k] = L;
  out_score[(size_t)b * K + k] = score;
}

// ----------------------------------------------------------------------------- host side
// the GEMM operands in [N][K] layout, once per handle
int rb_weights(cfm_rnnt* h) {
  std::lock_guard<std::mutex> lock(h->beam_mu);
  if (h->beam_mem) return 0;
  const RnntDev& w = h->w;
  std::vector<float> img;
  std::vector<std::pair<size_t, const float**>> fix;
  auto put_t = [&](const std::vector<float>& src, int Kd, int ld, int N, const float** slot) {   // [Kd][ld] -> [N][Kd]
    const size_t off = (img.size() + 63) / 64 * 64;
    img.resize(off + (size_t)N * Kd);
    for (int k = 0; k < Kd; ++k)
      for (int nn = 0; nn < N; ++nn) img[off + (size_t)nn * Kd + k] = src[(size_t)k * ld + nn];
    fix.push_back({off, slot});
  };
  for (int l = 0; l < w.nl; ++l) {
    const int in = l == 0 ? w.E : w.H;
    put_t(h->host_wg[l], in + w.H, 4 * w.H, 4 * w.H, &h->bw_g[l]);
  }
  const bool sl = w.kind != CFM_RNNT_PRED_RNN;
  put_t(h->host_wp, sl ? w.E : w.H, w.J, w.J, &h->bw_p);   // (a stateless handle: pred_ffn alone, [J][E])
  if (w.kind == CFM_RNNT_PRED_EMBEDDING) put_t(h->host_wf, w.E, w.E, w.E, &h->bw_f);
  put_t(h->host_wo, w.J, w.Vp, w.V, &h->bw_o);
  void* mem = nullptr;
  if (hipMalloc(&mem, img.size() * 4) != hipSuccess) return 1;
  if (hipMemcpy(mem, img.data(), img.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(mem);
    return 1;
  }
  for (auto& f : fix) *f.second = (const float*)mem + f.first;
  h->beam_mem = mem;
  return 0;
}

RbWS rb_carve(const cfm_rnnt* h, void* base, int rows, int B, int K, size_t* total) {
  const RnntDev& w = h->w;
  const size_t R = (size_t)std::max(B, 1) * K, rw = std::max(rows, 1);
  Carver c(base);
  RbWS s;
  s.err = c.take<int32_t>(64);
  s.ustart = c.take<int32_t>(std::max(B, 1));
  s.ulen = c.take<int32_t>(std::max(B, 1));
  s.n = c.take<int32_t>(std::max(B, 1));
  s.node = c.take<int32_t>(R);
  s.tok = c.take<int32_t>(R);
  s.tptr = c.take<int32_t>(R);
  s.par = c.take<int32_t>(R);
  s.chg = c.take<int32_t>(R);
  s.score = c.take<double>(R);
  s.tv = c.take<float>(R * K);
  s.ti = c.take<int32_t>(R * K);
  s.trie = carve_trie(c, rw * K, true);
  s.zero_bytes = c.off;
  s.enc_proj = c.take<float>(rw * w.J);
  s.act_off = c.off;
  for (int l = 0; l < w.nl; ++l) {
    const size_t in = l == 0 ? w.E : w.H;
    for (int q = 0; q < 2; ++q) {
      s.xh[l][q] = c.take<float>(R * (in + w.H));
      s.c[l][q] = c.take<float>(R * w.H);
    }
    s.hn[l] = c.take<float>(R * w.H);
    s.cn[l] = c.take<float>(R * w.H);
  }
  s.gates = c.take<float>(R * 4 * w.H);
  s.pj = c.take<float>(R * w.J);
  s.z = c.take<float>(R * w.J);
  s.hist[0] = s.hist[1] = s.ptok = nullptr;
  s.sx = s.sy = nullptr;
  s.hist_off = s.hist_bytes = 0;
  if (w.kind != CFM_RNNT_PRED_RNN) {   // the state of a slot is Kc - 1 ids (none with history_size 0)
    s.sx = c.take<float>(R * w.E);
    s.sy = c.take<float>(R * w.E);
    s.ptok = c.take<int32_t>(R);
    s.hist_off = c.off;
    s.hist[0] = c.take<int32_t>(std::max<size_t>(R * (w.Kc - 1), 1));
    s.hist[1] = c.take<int32_t>(std::max<size_t>(R * (w.Kc - 1), 1));
    s.hist_bytes = c.off - s.hist_off;
  }
  s.act_bytes = c.off - s.act_off;
  s.logits = c.take<float>(R * w.V);
  if (total) *total = c.off;
  return s;
}

bool rb_geom_ok(const cfm_rnnt* h, int rows, int B, int K) {
  return h && rows >= 0 && B >= 0 && K >= 1 && K <= BEAM_KMAX && K <= h->w.V && (int64_t)B * K <= (1 << 20) &&
         (size_t)K * (size_t)rows <= (size_t)0x3fffffff;
}

// gemm<float> walks K in steps of 32
bool rb_widths_ok(const cfm_rnnt* h) { return h->w.E % 32 == 0 && h->w.H % 32 == 0 && h->w.J % 32 == 0; }

int rb_gemm(const float* A, int lda, const float* W, const float* bias, int M, int N, int Kd, float* out, int ldo,
            hipStream_t st) {
  EpiArgs e;
  e.bias = bias; e.out = out; e.ldo = ldo;
  return gemm<float>(EPI_STORE, ACT_NONE, A, lda, W, Kd, M, N, Kd, e, st);
}

// embedding, LSTM layers, composed projection + pred_ffn for the live rows: state (h in xh[l][cur]'s h part, c in
// c[l][cur]) -> hn / cn (the state after this token) and pj
cfm_status rb_predictor(const cfm_rnnt* h, const RbWS& s, const RbLive& lv, int R, int cur, hipStream_t st) {
  const RnntDev& w = h->w;
  hipLaunchKernelGGL(rb_embed_kernel, dim3(R), dim3(64), 0, st, lv, s.tok, w.embed, w.V, w.E, s.xh[0][cur], w.E + w.H);
  KCHK((int)hipGetLastError());
  for (int l = 0; l < w.nl; ++l) {
    const int in = l == 0 ? w.E : w.H;
    KCHK(rb_gemm(s.xh[l][cur], in + w.H, h->bw_g[l], w.bg[l], R, 4 * w.H, in + w.H, s.gates, 4 * w.H, st));
    float* next = l + 1 < w.nl ? s.xh[l + 1][cur] : nullptr;
    hipLaunchKernelGGL(rb_cell_kernel, dim3(R), dim3(128), 0, st, lv, s.gates, w.H, s.c[l][cur], s.cn[l], s.hn[l], next,
                       2 * w.H);
    KCHK((int)hipGetLastError());
  }
  KCHK(rb_gemm(s.hn[w.nl - 1], w.H, h->bw_p, w.bp, R, w.J, w.H, s.pj, w.J, st));
  return CFM_OK;
}

cfm_status sl_predictor(const cfm_rnnt* h, const RbLive& lv, const int32_t* hist, int hist_ld, const int32_t* last,
                        int last_ld, int R, int32_t* ptok, float* x, float* y, float* pj, hipStream_t st) {
  const RnntDev& w = h->w;
  const size_t lds = ((size_t)w.Kc * w.E + 16) * sizeof(float);   // <= 9 * 1024 + 16 floats
  hipLaunchKernelGGL(sl_ctx_kernel, dim3(R), dim3(256), lds, st, lv, w, hist, hist_ld, last, last_ld, ptok, x);
  KCHK((int)hipGetLastError());
  const float* v = x;
  if (w.kind == CFM_RNNT_PRED_EMBEDDING) {
    KCHK(rb_gemm(x, w.E, h->bw_f, w.bf, R, w.E, w.E, y, w.E, st));
    v = y;
  }
  hipLaunchKernelGGL(sl_norm_act_kernel, dim3(R), dim3(256), 0, st, lv, w, v, y);
  KCHK((int)hipGetLastError());
  KCHK(rb_gemm(y, w.E, h->bw_p, w.bp, R, w.J, w.E, pj, w.J, st));
  return CFM_OK;
}

int rb_init(const int32_t* row_start, const int32_t* row_len, int B, int K, int rows, int max_len, int blank,
            const RbWS& s, hipStream_t st) {
  hipLaunchKernelGGL(rb_init_kernel, dim3((B + 63) / 64), dim3(64), 0, st, row_start, row_len, B, K, rows, max_len,
                     blank, s.err, s.ustart, s.ulen, s.n, s.node, s.tok, s.tptr, s.score);
  return (int)hipGetLastError();
}

namespace {

size_t rb_topk_lds(int V) { return V <= RB_LDS_KEYS ? (size_t)V * 4 : 0; }

// the prune operator's one-utterance state
struct RbPruneOp {
  int32_t *in_start, *in_len, *ustart, *ulen;
};
size_t rb_prune_op_carve(void* base, int T, int K, RbBeam& a, RbPruneOp& o) {
  const size_t tk = (size_t)std::max(T, 1) * K;
  Carver c(base);
  a.K = K;
  a.err = c.take<int32_t>(64);
  o.in_start = c.take<int32_t>(1);
  o.in_len = c.take<int32_t>(1);
  o.ustart = c.take<int32_t>(1);
  o.ulen = c.take<int32_t>(1);
  a.ustart = o.ustart; a.ulen = o.ulen;
  a.n = c.take<int32_t>(1);
  a.node = c.take<int32_t>(K); a.tok = c.take<int32_t>(K); a.tptr = c.take<int32_t>(K);
  a.par = c.take<int32_t>(K); a.chg = c.take<int32_t>(K);
  a.score = c.take<double>(K);
  a.trie = carve_trie(c, tk, true);
  return c.off;
}

}  // namespace
}  // namespace cfm

using namespace cfm;

extern "C" {

size_t cfm_rnnt_beam_workspace_bytes(const cfm_rnnt* h, int32_t rows, int32_t B, int32_t beam) {
  if (!rb_geom_ok(h, rows, B, beam)) return 0;
  size_t t = 0;
  rb_carve(h, nullptr, rows, B, beam, &t);
  return t + 256;
}

cfm_status cfm_rnnt_beam_search(cfm_rnnt* h, const float* enc, int32_t rows, const float* ctc_logp,
                                const int32_t* row_start, const int32_t* row_len, int32_t B, int32_t max_len,
                                int32_t beam, float ctc_weight, float transducer_weight, int32_t* out_tokens,
                                int32_t* out_times, int32_t* out_len, double* out_score, int32_t* n_hyps,
                                int32_t* trace_parent, int32_t* trace_token, double* trace_score, float* trace_topv,
                                int32_t* trace_topi, void* ws, size_t wsb, cfm_stream stream) {
  if (!h) return set_error(CFM_ERR_VALUE, "null handle");
  if (!rb_geom_ok(h, rows, B, beam))
    return set_error(CFM_ERR_VALUE, "rnnt beam search: bad rows / B / beam (1 .. 16, at most the vocabulary)");
  if (!(ctc_weight >= 0.f) || !(transducer_weight >= 0.f) || !(ctc_weight + transducer_weight > 0.f))
    return set_error(CFM_ERR_VALUE, "rnnt beam search: weights must be >= 0 and not both 0");
  if (max_len < 0 || max_len > rows) return set_error(CFM_ERR_VALUE, "rnnt beam search: max_len outside 0 .. rows");
  if (!rb_widths_ok(h))
    return set_error(CFM_ERR_ASSERT, "rnnt beam search: embed_size, hidden_size and join_dim must be multiples of 32");
  if (B == 0) return CFM_OK;
  if ((rows > 0 && !enc) || !row_start || !row_len || !out_tokens || !out_times || !out_len || !out_score || !n_hyps ||
      !ws)
    return set_error(CFM_ERR_VALUE, "null argument");
  if (ctc_weight > 0.f && rows > 0 && !ctc_logp)
    return set_error(CFM_ERR_VALUE, "rnnt beam search: ctc_weight > 0 needs the CTC log-probs");
  const bool trace = trace_parent || trace_token || trace_score || trace_topv || trace_topi;
  if (trace && !(trace_parent && trace_token && trace_score && trace_topv && trace_topi))
    return set_error(CFM_ERR_VALUE, "rnnt beam search: the trace needs all five arrays");
  if (wsb < cfm_rnnt_beam_workspace_bytes(h, rows, B, beam)) return set_error(CFM_ERR_VALUE, "rnnt beam workspace too small");
  if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(enc)) & 15)
    return set_error(CFM_ERR_VALUE, "encoder rows / workspace must be 16-byte aligned");
  if (hipSetDevice(h->device) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipSetDevice");
  if (rb_weights(h)) return set_error(CFM_ERR_RUNTIME, "rnnt beam search: weights upload");
  const hipStream_t st = (hipStream_t)stream;
  const RnntDev& w = h->w;
  const int K = beam, R = B * K;
  const RbWS s = rb_carve(h, ws, rows, B, K, nullptr);
  if (hipMemsetAsync(s.err, 0, s.zero_bytes, st) != hipSuccess ||
      hipMemsetAsync((char*)ws + s.act_off, 0, s.act_bytes, st) != hipSuccess ||
      (s.hist_bytes && hipMemsetAsync((char*)ws + s.hist_off, 0xff, s.hist_bytes, st) != hipSuccess))   // ids -1
    return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
  if (trace && rows > 0) {
    const size_t rk = (size_t)rows * K;
    if (hipMemsetAsync(trace_parent, 0xff, rk * 4, st) != hipSuccess ||
        hipMemsetAsync(trace_token, 0xff, rk * 4, st) != hipSuccess ||
        hipMemsetAsync(trace_score, 0, rk * 8, st) != hipSuccess ||
        hipMemsetAsync(trace_topv, 0, rk * K * 4, st) != hipSuccess ||
        hipMemsetAsync(trace_topi, 0xff, rk * K * 4, st) != hipSuccess)
      return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
  }
  hipLaunchKernelGGL(rb_init_kernel, dim3((B + 63) / 64), dim3(64), 0, st, row_start, row_len, B, K, rows, max_len,
                     w.blank, s.err, s.ustart, s.ulen, s.n, s.node, s.tok, s.tptr, s.score);
  KCHK((int)hipGetLastError());
  if (rows > 0)
    KCHK(rb_gemm(enc, h->cfg.enc_dim, h->we, h->be, rows, w.J, h->cfg.enc_dim, s.enc_proj, w.J, st));
  RbBeam a{};
  a.K = K; a.blank = w.blank; a.ustart = s.ustart; a.ulen = s.ulen;
  a.err = s.err; a.n = s.n; a.node = s.node; a.tok = s.tok; a.tptr = s.tptr; a.par = s.par; a.chg = s.chg;
  a.score = s.score;
  a.trie = s.trie;
  a.tr_parent = trace ? trace_parent : nullptr; a.tr_token = trace ? trace_token : nullptr;
  a.tr_score = trace ? trace_score : nullptr;
  const float* ctc = ctc_weight > 0.f ? ctc_logp : nullptr;
  for (int t = 0; t < max_len; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    const RbLive lv{s.ustart, s.ulen, s.n, K, t};
    const bool sl = w.kind != CFM_RNNT_PRED_RNN;
    if (sl) {
      if (const cfm_status e = sl_predictor(h, lv, s.hist[cur], w.Kc - 1, s.tok, 1, R, s.ptok, s.sx, s.sy, s.pj, st))
        return e;
    } else if (const cfm_status e = rb_predictor(h, s, lv, R, cur, st)) {
      return e;
    }
    hipLaunchKernelGGL(rb_joint_in_kernel, dim3(R), dim3(128), 0, st, lv, s.enc_proj, s.pj, w.J, s.z);
    KCHK((int)hipGetLastError());
    KCHK(rb_gemm(s.z, w.J, h->bw_o, w.bo, R, w.V, w.J, s.logits, w.V, st));
    hipLaunchKernelGGL(rb_fuse_topk_kernel, dim3(R), dim3(256), rb_topk_lds(w.V), st, lv, s.logits, ctc, w.V, K,
                       ctc_weight, transducer_weight, s.tv, s.ti, trace ? trace_topv : nullptr,
                       trace ? trace_topi : nullptr);
    KCHK((int)hipGetLastError());
    hipLaunchKernelGGL(rb_prune_kernel, dim3(B), dim3(256), 0, st, a, t, s.tv, s.ti);
    KCHK((int)hipGetLastError());
    // the new beam's state into the other buffers (n[b] is the new count: slots the prune kernel wrote)
    if (sl && w.Kc > 1) {
      hipLaunchKernelGGL(sl_gather_kernel, dim3((R + 63) / 64), dim3(64), 0, st, lv, s.par, s.chg, R, w.Kc - 1,
                         s.hist[cur], s.ptok, s.hist[nxt]);
      KCHK((int)hipGetLastError());
    }
    for (int l = 0; l < w.nl; ++l) {
      const int in = l == 0 ? w.E : w.H;
      hipLaunchKernelGGL(rb_gather_kernel, dim3(R), dim3(128), 0, st, lv, s.par, s.chg, w.H, s.xh[l][cur] + in,
                         in + w.H, s.hn[l], s.xh[l][nxt] + in, in + w.H, s.c[l][cur], s.cn[l], s.c[l][nxt]);
      KCHK((int)hipGetLastError());
    }
  }
  hipLaunchKernelGGL(rb_finish_kernel, dim3(B), dim3(64), 0, st, a, rows, out_tokens, out_times, out_len, out_score,
                     n_hyps);
  KCHK((int)hipGetLastError());
  return CFM_OK;
}

int32_t cfm_rnnt_beam_error(const void* ws) {
  if (!ws) return 0;
  int32_t e = 0;
  if (hipMemcpy(&e, ws, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return e;
}

// ---- operator-level entry points (include/cfm_ops.h)
cfm_status cfm_op_rnnt_fused_topk(const float* logits, const float* ctc_logp, int32_t R, int32_t V, int32_t K,
                                  float ctc_weight, float transducer_weight, float* vals, int32_t* ids,
                                  cfm_stream stream) {
  if (R < 0 || V < 1 || K < 1 || K > BEAM_KMAX || K > V) return set_error(CFM_ERR_VALUE, "fused top-k: bad R / V / K");
  if (R == 0) return CFM_OK;
  if (!logits || !vals || !ids) return set_error(CFM_ERR_VALUE, "null argument");
  const RbLive lv{nullptr, nullptr, nullptr, K, 0};
  hipLaunchKernelGGL(rb_fuse_topk_kernel, dim3(R), dim3(256), rb_topk_lds(V), (hipStream_t)stream, lv, logits, ctc_logp,
                     V, K, ctc_weight, transducer_weight, vals, ids, (float*)nullptr, (int32_t*)nullptr);
  KCHK((int)hipGetLastError());
  return CFM_OK;
}

size_t cfm_op_rnnt_beam_prune_workspace_bytes(int32_t T, int32_t K) {
  if (T < 0 || K < 1 || K > BEAM_KMAX) return 0;
  RbBeam a{};
  RbPruneOp o{};
  return rb_prune_op_carve(nullptr, T, K, a, o) + 256;
}

cfm_status cfm_op_rnnt_beam_prune(const float* topk_vals, const int32_t* topk_ids, int32_t T, int32_t K, int32_t blank,
                                  int32_t* trace_parent, int32_t* trace_token, double* trace_score, int32_t* n_hyps,
                                  void* ws, size_t wsb, cfm_stream stream) {
  if (T < 0 || K < 1 || K > BEAM_KMAX) return set_error(CFM_ERR_VALUE, "beam prune: bad T / K");
  if (T == 0) return CFM_OK;
  if (!topk_vals || !topk_ids || !trace_parent || !trace_token || !trace_score || !n_hyps || !ws)
    return set_error(CFM_ERR_VALUE, "null argument");
  if (wsb < cfm_op_rnnt_beam_prune_workspace_bytes(T, K)) return set_error(CFM_ERR_VALUE, "beam prune workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  RbBeam a{};
  RbPruneOp o{};
  const size_t used = rb_prune_op_carve(ws, T, K, a, o);
  a.blank = blank;
  a.tr_parent = trace_parent; a.tr_token = trace_token; a.tr_score = trace_score;
  const size_t tk = (size_t)T * K;
  if (hipMemsetAsync(ws, 0, used, st) != hipSuccess || hipMemsetAsync(trace_parent, 0xff, tk * 4, st) != hipSuccess ||
      hipMemsetAsync(trace_token, 0xff, tk * 4, st) != hipSuccess || hipMemsetAsync(trace_score, 0, tk * 8, st) != hipSuccess)
    return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
  // one utterance: rows [0, T)
  hipLaunchKernelGGL(rb_set_kernel, dim3(1), dim3(1), 0, st, o.in_len, T);
  KCHK((int)hipGetLastError());
  hipLaunchKernelGGL(rb_init_kernel, dim3(1), dim3(64), 0, st, o.in_start, o.in_len, 1, K, T, T, blank, a.err, o.ustart,
                     o.ulen, a.n, a.node, a.tok, a.tptr, a.score);
  KCHK((int)hipGetLastError());
  for (int t = 0; t < T; ++t) {
    hipLaunchKernelGGL(rb_prune_kernel, dim3(1), dim3(256), 0, st, a, t, topk_vals + (size_t)t * K * K,
                       topk_ids + (size_t)t * K * K);
    KCHK((int)hipGetLastError());
    if (hipMemcpyAsync(n_hyps + t, a.n, 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return set_error(CFM_ERR_RUNTIME, "hipMemcpyAsync");
  }
  return CFM_OK;
}

size_t cfm_op_rnnt_predictor_step_workspace_bytes(const cfm_rnnt* h, int32_t R) {
  if (!h || R < 1 || R > (1 << 20) || h->w.kind == CFM_RNNT_PRED_RNN) return 0;
  return (size_t)R * h->w.E * sizeof(float) + 256;
}

cfm_status cfm_op_rnnt_predictor_step(cfm_rnnt* h, const int32_t* windows, int32_t R, float* y_out, float* pred_out,
                                      void* ws, size_t wsb, cfm_stream stream) {
  if (!h) return set_error(CFM_ERR_VALUE, "null handle");
  if (h->w.kind == CFM_RNNT_PRED_RNN) return set_error(CFM_ERR_VALUE, "predictor step: not a stateless handle");
  if (R < 1 || R > (1 << 20)) return set_error(CFM_ERR_VALUE, "predictor step: bad R");
  if (!windows || !y_out || !pred_out || !ws) return set_error(CFM_ERR_VALUE, "null argument");
  if (!rb_widths_ok(h))
    return set_error(CFM_ERR_ASSERT, "rnnt beam search: embed_size, hidden_size and join_dim must be multiples of 32");
  if (wsb < cfm_op_rnnt_predictor_step_workspace_bytes(h, R)) return set_error(CFM_ERR_VALUE, "predictor step workspace too small");
  if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(y_out) | reinterpret_cast<uintptr_t>(pred_out)) & 15)
    return set_error(CFM_ERR_VALUE, "workspace / outputs must be 16-byte aligned");
  if (hipSetDevice(h->device) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipSetDevice");
  if (rb_weights(h)) return set_error(CFM_ERR_RUNTIME, "rnnt beam search: weights upload");
  const RbLive lv{nullptr, nullptr, nullptr, 1, 0};
  const int Kc = h->w.Kc;
  return sl_predictor(h, lv, windows, Kc, windows + Kc - 1, Kc, R, nullptr, (float*)ws, y_out, pred_out,
                      (hipStream_t)stream);
}

size_t cfm_op_rnnt_lstm_step_workspace_bytes(const cfm_rnnt* h, int32_t R) {
  if (!h || R < 1 || R > (1 << 20) || h->w.kind != CFM_RNNT_PRED_RNN) return 0;
  size_t t = 0;
  rb_carve(h, nullptr, 0, R, 1, &t);
  return t + 256;
}

cfm_status cfm_op_rnnt_lstm_step(cfm_rnnt* h, const int32_t* tokens, const float* h_in, const float* c_in, int32_t R,
                                 float* h_out, float* c_out, float* pred_out, void* ws, size_t wsb, cfm_stream stream) {
  if (!h) return set_error(CFM_ERR_VALUE, "null handle");
  if (h->w.kind != CFM_RNNT_PRED_RNN) return set_error(CFM_ERR_VALUE, "lstm step: not an LSTM handle");
  if (R < 1 || R > (1 << 20)) return set_error(CFM_ERR_VALUE, "lstm step: bad R");
  if (!tokens || !h_in || !c_in || !h_out || !c_out || !pred_out || !ws) return set_error(CFM_ERR_VALUE, "null argument");
  if (!rb_widths_ok(h))
    return set_error(CFM_ERR_ASSERT, "rnnt beam search: embed_size, hidden_size and join_dim must be multiples of 32");
  if (wsb < cfm_op_rnnt_lstm_step_workspace_bytes(h, R)) return set_error(CFM_ERR_VALUE, "lstm step workspace too small");
  if (reinterpret_cast<uintptr_t>(ws) & 15) return set_error(CFM_ERR_VALUE, "workspace must be 16-byte aligned");
  if (hipSetDevice(h->device) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipSetDevice");
  if (rb_weights(h)) return set_error(CFM_ERR_RUNTIME, "rnnt beam search: weights upload");
  const hipStream_t st = (hipStream_t)stream;
  const RnntDev& w = h->w;
  RbWS s = rb_carve(h, ws, 0, R, 1, nullptr);
  const size_t RH = (size_t)R * w.H;
  if (hipMemcpyAsync(s.tok, tokens, (size_t)R * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return set_error(CFM_ERR_RUNTIME, "hipMemcpyAsync");
  for (int l = 0; l < w.nl; ++l) {
    const int in = l == 0 ? w.E : w.H;
    if (hipMemcpy2DAsync(s.xh[l][0] + in, (size_t)(in + w.H) * 4, h_in + l * RH, (size_t)w.H * 4, (size_t)w.H * 4, R,
                         hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(s.c[l][0], c_in + l * RH, RH * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return set_error(CFM_ERR_RUNTIME, "hipMemcpyAsync");
  }
  const RbLive lv{nullptr, nullptr, nullptr, 1, 0};
  if (const cfm_status e = rb_predictor(h, s, lv, R, 0, st)) return e;
  for (int l = 0; l < w.nl; ++l)
    if (hipMemcpyAsync(h_out + l * RH, s.hn[l], RH * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(c_out + l * RH, s.cn[l], RH * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return set_error(CFM_ERR_RUNTIME, "hipMemcpyAsync");
  if (hipMemcpyAsync(pred_out, s.pj, (size_t)R * w.J * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return set_error(CFM_ERR_RUNTIME, "hipMemcpyAsync");
  return CFM_OK;
}

}  // extern "C"
