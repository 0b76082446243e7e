// Attention decoding mode: the reference's autoregressive attention_beam_search (modules/search.py:252-355) over the
// left decoder of the cfm_aed handle (csrc/aed.h), every utterance of a masked batch at once, N = beam rows each.
//
// Rows: r = u * N + j (utterance u, beam j), R = B * N.  Step i = 1 .. feeds row r's last token at position i - 1; all
// running utterances step together, an utterance that is done (all beams ended, or its own limit reached, or rejected
// at begin) is frozen: its state words are never written again and the attention kernels skip its rows.
//
//   attdec_init_kernel     validates the utterance row ranges and limits (status word), start state
//   attdec_embed_kernel    x = embed[last token] * sqrt(d) + pe[i - 1]
//   the decoder blocks     aed_decoder_blocks (aed.h), with  self: K|V GEMM written straight into the self-attention
//                          cache at (layer, i - 1, r) -> attdec_self_kernel;  cross: attdec_cross_* (-> combine) over
//                          the memory K|V that begin projected
//   output_layer GEMM [R, V] (vocab_logits), ctc_topk_rows (logit - lse, top N, value descending / index ascending)
//   attdec_prune_kernel    one workgroup per utterance: finished-beam masking, top N of N * N, scores, tokens, end
//                          flags, trace row, ancestry, freezing, the count of running utterances
//   attdec_finish_kernel   backtrace through the trace, length penalty, selection
//
// The self-attention cache is never moved: position p of row r's hypothesis lives in slot anc[r][p] (a row index), its
// own newest row in slot r.  A prune copies the parents' ancestry rows (int32, i per beam) into the other of two
// buffers; the K|V rows stay where they were written.
//
// Cross-attention: the keys of an utterance are shared by its beams.  Workgroup (utterance, head, key split); the up
// to 16 beams are the 16 query columns of one wave:
//   generic   any type, head dim a multiple of 16 up to 128: lane (beam, quarter of the head's dims), keys one at a
//             time, every key row read once for all beams
//   mfma      bf16 / f16, head dim 64 / 128: the 32-key tile of attn_core.h, the beams on the lanes' column axis
// With more than one key split the parts write (m, l, unnormalised o) and attdec_combine_kernel merges them.
// Loops are bounded by launch arguments and validated lengths; plain vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/cfm.h"
#include "../../include/cfm_ops.h"
#include "aed.h"
#include "attn_core.h"
#include "beam.h"

namespace cfm {

constexpr int ATTDEC_MAX_SPLIT = 16;
enum { ADW_STATUS = 0, ADW_RUNNING = 1, ADW_INTS = 64 };
enum { ATTDEC_ST_UTT = 2, ATTDEC_ST_LIMIT = 5 };

// ----------------------------------------------------------------------------- state kernels
__global__ __launch_bounds__(64) void attdec_init_kernel(const int32_t* __restrict__ ustart_in,
                                                         const int32_t* __restrict__ ulen_in,
                                                         const int32_t* __restrict__ limit_in, int B, int N, int mem_rows,
                                                         int S, int sos, int32_t* __restrict__ words,
                                                         int32_t* __restrict__ ustart, int32_t* __restrict__ ulen,
                                                         int32_t* __restrict__ limit, int32_t* __restrict__ done,
                                                         int32_t* __restrict__ tok, float* __restrict__ score) {
  const int u = blockIdx.x, j = threadIdx.x;
  int s = ustart_in[u], n = ulen_in[u], lim = limit_in[u];
  int code = 0;
  if (s < 0 || n < 0 || s > mem_rows || n > mem_rows - s) code = ATTDEC_ST_UTT;
  else if (lim < 0 || lim > S) code = ATTDEC_ST_LIMIT;
  if (code) { s = 0; n = 0; lim = 0; }
  if (j < N) {
    tok[u * N + j] = sos;
    score[u * N + j] = j == 0 ? 0.f : -INFINITY;
  }
  if (j == 0) {
    ustart[u] = s; ulen[u] = n; limit[u] = lim;
    done[u] = lim == 0;
    if (lim > 0) atomicAdd(&words[ADW_RUNNING], 1);
    if (code) words[ADW_STATUS] = code;
  }
}

__global__ __launch_bounds__(128) void attdec_embed_kernel(const int32_t* __restrict__ tok, int d, int pos,
                                                           const float* __restrict__ embed, const float* __restrict__ pe,
                                                           float xscale, float* __restrict__ x) {
  const int r = blockIdx.x;
  const float4* e = reinterpret_cast<const float4*>(embed + (size_t)tok[r] * d);
  const float4* p = reinterpret_cast<const float4*>(pe + (size_t)pos * d);
  float4* o = reinterpret_cast<float4*>(x + (size_t)r * d);
  for (int c = threadIdx.x; c < (d >> 2); c += 128) {
    const float4 a = e[c], b = p[c];
    o[c] = make_float4(a.x * xscale + b.x, a.y * xscale + b.y, a.z * xscale + b.z, a.w * xscale + b.w);
  }
}

// ----------------------------------------------------------------------------- self-attention by gather
// One wave = one (row, head): lane (key lane 0 .. 15, quarter of the head's dims); key lane f takes the positions
// f, f + 16, ... with an online softmax of its own, the 16 streams are merged at the end.  n_keys >= 1 positions: p <
// n_keys - 1 from slot anc[r][p], the newest from slot r.  kv [position][R][K d | V d].
template <typename T, int DKQ>
__global__ __launch_bounds__(64) void attdec_self_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                         const int32_t* __restrict__ anc, int anc_ld, int n_keys, int R,
                                                         int N, int d, const int32_t* __restrict__ done,
                                                         T* __restrict__ out, float scale) {
  typedef typename Vec4<T>::type V4;
  constexpr int DK = 4 * DKQ;
  const int r = blockIdx.x;
  if (done && done[r / N]) return;
  const int lane = threadIdx.x, fr = lane & 15, part = lane >> 4;
  const int col = blockIdx.y * DK + part * DKQ;
  float qv[DKQ], acc[DKQ];
  {
    const T* qp = q + (size_t)r * d + col;
#pragma unroll
    for (int e = 0; e < DKQ; e += 4) {
      const V4 t = *reinterpret_cast<const V4*>(qp + e);
#pragma unroll
      for (int c = 0; c < 4; ++c) { qv[e + c] = to_f32(t[c]); acc[e + c] = 0.f; }
    }
  }
  float m = -INFINITY, l = 0.f;
  const size_t ld = 2 * (size_t)d;
  for (int j0 = 0; j0 < n_keys; j0 += 16) {
    const int j = j0 + fr, jj = min(j, n_keys - 1);
    int slot = r;
    if (jj < n_keys - 1) slot = min(max(anc[(size_t)r * anc_ld + jj], 0), R - 1);
    const T* kp = kv + ((size_t)jj * R + slot) * ld + col;
    const T* vp = kp + d;
    float s = 0.f, vv[DKQ];
#pragma unroll
    for (int e = 0; e < DKQ; e += 4) {
      const V4 kt = *reinterpret_cast<const V4*>(kp + e);
      const V4 vt = *reinterpret_cast<const V4*>(vp + e);
#pragma unroll
      for (int c = 0; c < 4; ++c) { s = fmaf(qv[e + c], to_f32(kt[c]), s); vv[e + c] = to_f32(vt[c]); }
    }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    s *= scale;
    if (j < n_keys) {
      const float mx = fmaxf(m, s);
      const float alpha = __expf(m - mx);   // first key: exp(-inf) = 0
      const float p = __expf(s - mx);
      l = l * alpha + p;
#pragma unroll
      for (int e = 0; e < DKQ; ++e) acc[e] = acc[e] * alpha + p * vv[e];
      m = mx;
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
    const float mx = fmaxf(m, m2);
    const float a = m == -INFINITY ? 0.f : __expf(m - mx), b = m2 == -INFINITY ? 0.f : __expf(m2 - mx);
    l = l * a + l2 * b;
#pragma unroll
    for (int e = 0; e < DKQ; ++e) acc[e] = acc[e] * a + __shfl_xor(acc[e], o, 64) * b;
    m = mx;
  }
  if (fr == 0) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    T* op = out + (size_t)r * d + col;
#pragma unroll
    for (int e = 0; e < DKQ; e += 4) {
      V4 t;
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = from_f32<T>(acc[e + c] * inv);
      *reinterpret_cast<V4*>(op + e) = t;
    }
  }
}

// ----------------------------------------------------------------------------- beam-shared cross-attention
// this workgroup's utterance, its key range [j0, j1) of the split (empty for a rejected range) and first key row
CFM_DEV bool ad_cross_range(const int32_t* ustart, const int32_t* ulen, const int32_t* done, int mem_rows, int& k0,
                            int& j0, int& j1) {
  const int u = blockIdx.x;
  if (done && done[u]) return false;
  int s = ustart[u], n = ulen[u];
  if (s < 0 || n < 0 || s > mem_rows || n > mem_rows - s) { s = 0; n = 0; }
  const int ns = gridDim.z, per = (n + ns - 1) / ns;
  k0 = s;
  j0 = min((int)blockIdx.z * per, n);
  j1 = min(j0 + per, n);
  return true;
}

// parts: part_o [split][R][d] f32 unnormalised, part_ml [split][R][H][2] f32 (m, l)
template <typename T, int DKQ>
__global__ __launch_bounds__(64) void attdec_cross_generic_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                                  int mem_rows, const int32_t* __restrict__ ustart,
                                                                  const int32_t* __restrict__ ulen,
                                                                  const int32_t* __restrict__ done, int R, int N, int d,
                                                                  T* __restrict__ out, float* __restrict__ part_o,
                                                                  float* __restrict__ part_ml, float scale) {
  typedef typename Vec4<T>::type V4;
  constexpr int DK = 4 * DKQ;
  int k0, j0, j1;
  if (!ad_cross_range(ustart, ulen, done, mem_rows, k0, j0, j1)) return;
  const int lane = threadIdx.x, fr = lane & 15, part = lane >> 4;
  const int H = gridDim.y, head = blockIdx.y;
  const int col = head * DK + part * DKQ;
  const int row = blockIdx.x * N + min(fr, N - 1);
  float qv[DKQ], acc[DKQ];
  {
    const T* qp = q + (size_t)row * d + col;
#pragma unroll
    for (int e = 0; e < DKQ; e += 4) {
      const V4 t = *reinterpret_cast<const V4*>(qp + e);
#pragma unroll
      for (int c = 0; c < 4; ++c) { qv[e + c] = to_f32(t[c]); acc[e + c] = 0.f; }
    }
  }
  float m = -INFINITY, l = 0.f;
  const size_t ld = 2 * (size_t)d;
  for (int j = j0; j < j1; ++j) {
    const T* kp = kv + (size_t)(k0 + j) * ld + col;
    const T* vp = kp + d;
    float s = 0.f, vv[DKQ];
#pragma unroll
    for (int e = 0; e < DKQ; e += 4) {
      const V4 kt = *reinterpret_cast<const V4*>(kp + e);
      const V4 vt = *reinterpret_cast<const V4*>(vp + e);
#pragma unroll
      for (int c = 0; c < 4; ++c) { s = fmaf(qv[e + c], to_f32(kt[c]), s); vv[e + c] = to_f32(vt[c]); }
    }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    s *= scale;
    const float mx = fmaxf(m, s);
    const float alpha = __expf(m - mx);
    const float p = __expf(s - mx);
    l = l * alpha + p;
#pragma unroll
    for (int e = 0; e < DKQ; ++e) acc[e] = acc[e] * alpha + p * vv[e];
    m = mx;
  }
  if (fr >= N) return;
  if (gridDim.z == 1) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    T* op = out + (size_t)row * d + col;
#pragma unroll
    for (int e = 0; e < DKQ; e += 4) {
      V4 t;
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = from_f32<T>(acc[e + c] * inv);
      *reinterpret_cast<V4*>(op + e) = t;
    }
  } else {
    float* op = part_o + ((size_t)blockIdx.z * R + row) * d + col;
#pragma unroll
    for (int e = 0; e < DKQ; ++e) op[e] = acc[e];
    if (part == 0) {
      float* mp = part_ml + (((size_t)blockIdx.z * R + row) * H + head) * 2;
      mp[0] = m;
      mp[1] = l;
    }
  }
}

// One wave: the utterance's beams are the 16 query columns (lanes past the beam repeat the last beam, never stored).
template <typename T, int DK>
__global__ __launch_bounds__(64) void attdec_cross_mfma_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                               int mem_rows, const int32_t* __restrict__ ustart,
                                                               const int32_t* __restrict__ ulen,
                                                               const int32_t* __restrict__ done, int R, int N, int d,
                                                               T* __restrict__ out, float* __restrict__ part_o,
                                                               float* __restrict__ part_ml, float scale) {
  typedef typename Vec4<T>::type V4;
  typedef typename Frag<T>::type F8;
  typedef AttnTile<DK> G;   // the tile's geometry and key permutation: attn_core.h
  constexpr int KS = G::KS, NJ = G::NJ, KP = G::KP, VP = G::VP, CH = G::CH;
  __shared__ __attribute__((aligned(16))) T ks[32 * KP];
  __shared__ __attribute__((aligned(16))) T vt[DK * VP];
  int k0, j0, j1;
  if (!ad_cross_range(ustart, ulen, done, mem_rows, k0, j0, j1)) return;
  const int lane = threadIdx.x, fr = lane & 15, gq = lane >> 4;
  const int H = gridDim.y, head = blockIdx.y;
  const int col = head * DK;
  const int row = blockIdx.x * N + min(fr, N - 1);
  const size_t ld = 2 * (size_t)d;
  const T* kb = kv;
  const T* vb = kv + d;
  F8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = ld8<T>(q + (size_t)row * d + col + 32 * s + 8 * gq);
  f32x4 o[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) o[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  for (int t0 = j0; t0 < j1; t0 += 32) {
    __syncthreads();   // the previous tile's reads are done
    for (int c = lane; c < 32 * CH; c += 64) {
      const int key = c / CH, ch = c - key * CH;
      const size_t at = (size_t)(k0 + min(t0 + key, j1 - 1)) * ld + col + 8 * ch;
      st8<T>(ks + key * KP + 8 * ch, ld8<T>(kb + at));
      const F8 t = ld8<T>(vb + at);
#pragma unroll
      for (int e = 0; e < 8; ++e) vt[(8 * ch + e) * VP + key] = t[e];
    }
    __syncthreads();
    float p[8];
    float mx = m;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
      const T* kp = ks + (16 * t2 + fr) * KP + 8 * gq;
#pragma unroll
      for (int s = 0; s < KS; ++s) a = mma16(ld8<T>(kp + 32 * s), qf[s], a);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = t0 + 16 * t2 + 4 * gq + r;
        const float sv = j < j1 ? a[r] * scale : -INFINITY;
        p[4 * t2 + r] = sv;
        mx = fmaxf(mx, sv);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float alpha = m == -INFINITY ? 0.f : __expf(m - mx);
    F8 pb;
    float ps = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float pv = p[e] == -INFINITY ? 0.f : __expf(p[e] - mx);
      ps += pv;
      pb[e] = from_f32<T>(pv);
    }
    l = l * alpha + ps;
    m = mx;
#pragma unroll
    for (int j = 0; j < NJ; ++j) o[j] *= alpha;
    // O^T += V^T . P^T: contraction index 8 gq + e <-> key 16 (e / 4) + 4 gq + (e % 4) on both operands
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const T* rp = vt + (16 * j + fr) * VP + 4 * gq;
      const V4 lo = *reinterpret_cast<const V4*>(rp), hi = *reinterpret_cast<const V4*>(rp + 16);
      const F8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      o[j] = mma16(a, pb, o[j]);
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (fr >= N) return;
  if (gridDim.z == 1) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    T* op = out + (size_t)row * d + col + 4 * gq;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      V4 t;
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] = from_f32<T>(o[j][r] * inv);
      *reinterpret_cast<V4*>(op + 16 * j) = t;
    }
  } else {
    float* op = part_o + ((size_t)blockIdx.z * R + row) * d + col + 4 * gq;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      *reinterpret_cast<f32x4*>(op + 16 * j) = o[j];
    if (gq == 0) {
      float* mp = part_ml + (((size_t)blockIdx.z * R + row) * H + head) * 2;
      mp[0] = m;
      mp[1] = l;
    }
  }
}

// out[r] = sum_s o_s e^(m_s - M) / sum_s l_s e^(m_s - M); a row whose parts are all empty gives 0
template <typename T>
__global__ __launch_bounds__(128) void attdec_combine_kernel(const float* __restrict__ part_o,
                                                             const float* __restrict__ part_ml, int ns, int R, int N,
                                                             int H, int dk, const int32_t* __restrict__ done,
                                                             T* __restrict__ out) {
  const int r = blockIdx.x, d = H * dk;
  if (done && done[r / N]) return;
  for (int c = threadIdx.x; c < d; c += 128) {
    const int head = c / dk;
    float M = -INFINITY;
    for (int s = 0; s < ns; ++s) M = fmaxf(M, part_ml[(((size_t)s * R + r) * H + head) * 2]);
    float L = 0.f, o = 0.f;
    for (int s = 0; s < ns; ++s) {
      const float* mp = part_ml + (((size_t)s * R + r) * H + head) * 2;
      if (mp[0] == -INFINITY) continue;
      const float w = __expf(mp[0] - M);
      L += mp[1] * w;
      o += part_o[((size_t)s * R + r) * d + c] * w;
    }
    out[(size_t)r * d + c] = from_f32<T>(L > 0.f ? o / L : 0.f);
  }
}

// ----------------------------------------------------------------------------- prune
// One workgroup per utterance.  Candidate c = b * N + k: beam b's k-th best token; a finished beam (fin) has the one
// candidate (score + 0, eos) at k = 0 and -inf elsewhere.  The N best by (value descending, c ascending), wave 0.
__global__ __launch_bounds__(256) void attdec_prune_kernel(int i, int N, int R, int S, int eos,
                                                           const float* __restrict__ tv, const int32_t* __restrict__ ti,
                                                           float* __restrict__ score, int32_t* __restrict__ tok,
                                                           int32_t* __restrict__ fin, const int32_t* __restrict__ anc_cur,
                                                           int32_t* __restrict__ anc_nxt, int32_t* __restrict__ tr_parent,
                                                           int32_t* __restrict__ tr_token, float* __restrict__ tr_score,
                                                           const int32_t* __restrict__ limit, int32_t* __restrict__ done,
                                                           int32_t* __restrict__ steps, int32_t* __restrict__ words) {
  __shared__ int s_par[BEAM_KMAX], s_tok[BEAM_KMAX];
  __shared__ float s_val[BEAM_KMAX];
  const int u = blockIdx.x, tid = threadIdx.x;
  if (done[u]) return;
  if (tid < 64) {
    const int lane = tid, N2 = N * N;
    uint32_t key[4];
    int ctok[4];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int c = lane + 64 * qd;
      key[qd] = 0u;
      ctok[qd] = eos;
      if (c < N2) {
        const int b = c / N, k = c - b * N, row = u * N + b;
        const bool f = fin[row] != 0;
        const float sc = score[row];
        const float val = f ? (k == 0 ? sc : -INFINITY) : sc + tv[(size_t)row * N + k];
        key[qd] = f2key(val);
        ctok[qd] = f ? eos : ti[(size_t)row * N + k];
      }
    }
    TopKRound top;
    for (int r = 0; r < N; ++r) {
#pragma unroll
      for (int qd = 0; qd < 4; ++qd)
        if (lane + 64 * qd < N2) top.see(key[qd], lane + 64 * qd);
      top.reduce64();
      const int sel = top.bi == TOPK_NONE ? 0 : top.bi;   // (N * N >= N candidates: always found)
      const int qs = sel >> 6;
      const int mine = qs == 0 ? ctok[0] : qs == 1 ? ctok[1] : qs == 2 ? ctok[2] : ctok[3];
      const int tk = __shfl(mine, sel & 63, 64);
      if (lane == 0) {
        s_par[r] = sel / N;
        s_tok[r] = tk;
        s_val[r] = key2f(top.bk);
      }
      top.next();
    }
  }
  __syncthreads();
  if (tid < N) {
    const int row = u * N + tid;
    score[row] = s_val[tid];
    tok[row] = s_tok[tid];
    fin[row] = s_tok[tid] == eos;
    const size_t t = (size_t)(i - 1) * R + row;
    tr_parent[t] = s_par[tid];
    tr_token[t] = s_tok[tid];
    tr_score[t] = s_val[tid];
  }
  // ancestry of the new beams: the parent's slots of positions 0 .. i - 2, and the parent's own row at i - 1
  for (int idx = tid; idx < N * i; idx += 256) {
    const int j = idx / i, p = idx - j * i;
    const int prow = u * N + s_par[j];
    anc_nxt[(size_t)(u * N + j) * S + p] = p == i - 1 ? prow : anc_cur[(size_t)prow * S + p];
  }
  if (tid == 0) {
    bool all = true;
    for (int j = 0; j < N; ++j) all = all && s_tok[j] == eos;
    steps[u] = i;
    if (all || i >= limit[u]) {
      done[u] = 1;
      atomicSub(&words[ADW_RUNNING], 1);
    }
  }
}

// ----------------------------------------------------------------------------- finish
// One workgroup per utterance, thread j = beam j: tokens by backtrace, the count of tokens != eos over the whole row
// (sos included), score / count^penalty in f32, and the first maximum (a NaN is the maximum, as torch.max has it)
__global__ __launch_bounds__(64) void attdec_finish_kernel(int N, int R, int S, int sos, int eos, float penalty,
                                                           const float* __restrict__ score,
                                                           const int32_t* __restrict__ steps,
                                                           const int32_t* __restrict__ tr_parent,
                                                           const int32_t* __restrict__ tr_token,
                                                           int32_t* __restrict__ tokens_out, int32_t* __restrict__ len_out,
                                                           float* __restrict__ final_out, int32_t* __restrict__ best_out) {
  __shared__ float s_f[BEAM_KMAX];
  const int u = blockIdx.x, j = threadIdx.x;
  if (j < N) {
    const int row = u * N + j, n = min(max(steps[u], 0), S);
    int cnt = sos != eos, b = j;
    for (int t = n - 1; t >= 0; --t) {
      const size_t at = (size_t)t * R + u * N + b;
      const int tk = tr_token[at];
      tokens_out[(size_t)row * S + t] = tk;
      cnt += tk != eos;
      b = min(max(tr_parent[at], 0), N - 1);
    }
    len_out[row] = n;
    const float f = score[row] / powf((float)cnt, penalty);
    s_f[j] = f;
    final_out[row] = f;
  }
  __syncthreads();
  if (j == 0) {
    int best = 0;
    for (int k = 1; k < N; ++k) {
      if (s_f[best] != s_f[best]) break;
      if (s_f[k] != s_f[k] || s_f[k] > s_f[best]) best = k;
    }
    best_out[u] = best;
  }
}

// ----------------------------------------------------------------------------- launchers
enum { AD_KERNEL_SELF = 0, AD_KERNEL_CROSS_GENERIC = 1, AD_KERNEL_CROSS_MFMA = 2 };

static bool ad_cross_mfma_takes(int dtype, int dk) { return dtype != CFM_DTYPE_F32 && (dk == 64 || dk == 128); }

template <typename T>
static int ad_self_attention(const T* q, const T* kv, const int32_t* anc, int anc_ld, int n_keys, int R, int N, int H,
                             int dk, const int32_t* done, T* out, hipStream_t st) {
  if (dk < 16 || dk > 128 || dk % 16) return -1;
  if (R <= 0 || n_keys <= 0) return 0;
  const float scale = 1.0f / std::sqrt((float)dk);
#define AD_SELF(Q_)                                                                                                   \
  case Q_:                                                                                                            \
    hipLaunchKernelGGL((attdec_self_kernel<T, Q_>), dim3(R, H), dim3(64), 0, st, q, kv, anc, anc_ld, n_keys, R, N, H * dk, \
                       done, out, scale);                                                                             \
    break;
  switch (dk / 4) {
    AD_SELF(4) AD_SELF(8) AD_SELF(12) AD_SELF(16) AD_SELF(20) AD_SELF(24) AD_SELF(28) AD_SELF(32)
    default: return -1;
  }
#undef AD_SELF
  CFM_CHECK_LAUNCH();
  return 0;
}

template <typename T>
static int ad_cross_attention(int kernel, const T* q, const T* kv, int mem_rows, const int32_t* ustart,
                              const int32_t* ulen, const int32_t* done, int B, int N, int H, int dk, int ns, T* out,
                              float* part_o, float* part_ml, hipStream_t st) {
  if (B <= 0) return 0;
  const int R = B * N, d = H * dk;
  const float scale = 1.0f / std::sqrt((float)dk);
  const dim3 grid(B, H, ns);
  if (kernel == AD_KERNEL_CROSS_MFMA) {
    if constexpr (sizeof(T) != 2) {
      return -1;
    } else {
      if (dk == 64)
        hipLaunchKernelGGL((attdec_cross_mfma_kernel<T, 64>), grid, dim3(64), 0, st, q, kv, mem_rows, ustart, ulen, done, R,
                           N, d, out, part_o, part_ml, scale);
      else if (dk == 128)
        hipLaunchKernelGGL((attdec_cross_mfma_kernel<T, 128>), grid, dim3(64), 0, st, q, kv, mem_rows, ustart, ulen, done,
                           R, N, d, out, part_o, part_ml, scale);
      else
        return -1;
    }
  } else {
    if (dk < 16 || dk > 128 || dk % 16) return -1;
#define AD_CROSS(Q_)                                                                                                     \
  case Q_:                                                                                                               \
    hipLaunchKernelGGL((attdec_cross_generic_kernel<T, Q_>), grid, dim3(64), 0, st, q, kv, mem_rows, ustart, ulen, done, R, \
                       N, d, out, part_o, part_ml, scale);                                                               \
    break;
    switch (dk / 4) {
      AD_CROSS(4) AD_CROSS(8) AD_CROSS(12) AD_CROSS(16) AD_CROSS(20) AD_CROSS(24) AD_CROSS(28) AD_CROSS(32)
      default: return -1;
    }
#undef AD_CROSS
  }
  CFM_CHECK_LAUNCH();
  if (ns > 1) {
    hipLaunchKernelGGL((attdec_combine_kernel<T>), dim3(R), dim3(128), 0, st, part_o, part_ml, ns, R, N, H, dk, done, out);
    CFM_CHECK_LAUNCH();
  }
  return 0;
}

// key splits of the cross-attention: a workgroup is one wave, so aim at 8 of them per compute unit over the
// (utterance, head, split) grid, in parts of at least 64 keys
static int ad_key_splits(int B, int H, int mem_rows) {
  const int wg = std::max(B * H, 1), target = 8 * std::max(cu_count(), 1);
  if (wg >= target) return 1;
  const int want = (target + wg - 1) / wg, by_keys = std::max(1, mem_rows / std::max(B, 1) / 64);
  return std::max(1, std::min(ATTDEC_MAX_SPLIT, std::min(want, by_keys)));
}

struct AdGeom {
  int B, N, R, mem_rows, S, ns;
};

template <typename T>
struct AttDec {
  struct WS {
    int32_t *words, *ustart, *ulen, *limit, *done, *steps, *tok, *fin, *anc, *tr_parent, *tr_token, *ti;
    float *score, *tr_score, *x, *logits, *tv, *part_o, *part_ml;
    T *h, *q, *ao, *hid, *memT, *mkv, *kvc;
    size_t zero_bytes;   // [words, tr_parent): zeroed at begin
  };
  static WS carve(const cfm_aed* a, void* base, const AdGeom& g, size_t* total) {
    const size_t d = a->cfg.d, ff = a->cfg.ff, V = a->cfg.V, nb = a->dec[0].layers.size();
    const size_t B = std::max(g.B, 1), R = std::max(g.R, 1), S = std::max(g.S, 1), mr = std::max(g.mem_rows, 1);
    Carver c(base);
    WS w;
    w.words = c.take<int32_t>(ADW_INTS);
    w.ustart = c.take<int32_t>(B);
    w.ulen = c.take<int32_t>(B);
    w.limit = c.take<int32_t>(B);
    w.done = c.take<int32_t>(B);
    w.steps = c.take<int32_t>(B);
    w.tok = c.take<int32_t>(R);
    w.fin = c.take<int32_t>(R);
    w.score = c.take<float>(R);
    w.anc = c.take<int32_t>(2 * R * S);
    w.zero_bytes = c.off;
    w.tr_parent = c.take<int32_t>(S * R);
    w.tr_token = c.take<int32_t>(S * R);
    w.tr_score = c.take<float>(S * R);
    w.ti = c.take<int32_t>(R * BEAM_KMAX);
    w.tv = c.take<float>(R * BEAM_KMAX);
    w.x = c.take<float>(R * d);
    w.h = c.take<T>(R * d);
    w.q = c.take<T>(R * d);
    w.ao = c.take<T>(R * d);
    w.hid = c.take<T>(R * ff);
    w.logits = c.take<float>(R * V);
    w.part_o = c.take<float>((size_t)g.ns * R * d);
    w.part_ml = c.take<float>((size_t)g.ns * R * a->cfg.H * 2);
    w.memT = sizeof(T) == 4 ? nullptr : c.take<T>(mr * d);
    w.mkv = c.take<T>(nb * mr * 2 * d);
    w.kvc = c.take<T>(nb * S * R * 2 * d);
    if (total) *total = c.off;
    return w;
  }
  static bool cross_mfma(const cfm_aed* a) { return ad_cross_mfma_takes(a->cfg.dtype, a->cfg.d / a->cfg.H); }

  static cfm_status begin(const cfm_aed* a, const AdGeom& g, const float* mem, const int32_t* ustart,
                          const int32_t* ulen, const int32_t* limit, void* ws, hipStream_t st) {
    const int d = a->cfg.d;
    WS w = carve(a, ws, g, nullptr);
    const size_t tr = (size_t)std::max(g.S, 1) * std::max(g.R, 1);
    if (hipMemsetAsync(w.words, 0, w.zero_bytes, st) != hipSuccess ||
        hipMemsetAsync(w.tr_parent, 0xff, align_up(tr * 4), st) != hipSuccess ||
        hipMemsetAsync(w.tr_token, 0xff, align_up(tr * 4), st) != hipSuccess ||
        hipMemsetAsync(w.tr_score, 0, align_up(tr * 4), st) != hipSuccess ||
        hipMemsetAsync(w.ao, 0, (size_t)g.R * d * sizeof(T), st) != hipSuccess)
      return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
    hipLaunchKernelGGL(attdec_init_kernel, dim3(g.B), dim3(64), 0, st, ustart, ulen, limit, g.B, g.N, g.mem_rows, g.S,
                       a->cfg.sos, w.words, w.ustart, w.ulen, w.limit, w.done, w.tok, w.score);
    KCHK((int)hipGetLastError());
    if (g.mem_rows > 0) {
      const T* memT;
      KCHK(aed_memory_rows<T>(mem, g.mem_rows, d, w.memT, st, &memT));
      // cross-attention K|V of every left-decoder block, once, over all encoder rows of the batch
      size_t l = 0;
      for (const AedLayerW& L : a->dec[0].layers) {
        KCHK(aed_memory_kv<T>(L, memT, g.mem_rows, d, w.mkv + l * (size_t)g.mem_rows * 2 * d, st));
        ++l;
      }
    }
    return CFM_OK;
  }

  static cfm_status steps(const cfm_aed* a, const AdGeom& g, int step0, int n_steps, void* ws, hipStream_t st) {
    const int d = a->cfg.d, V = a->cfg.V, H = a->cfg.H, dk = d / H, R = g.R, N = g.N, S = g.S;
    WS w = carve(a, ws, g, nullptr);
    const AedDecoderW& D = a->dec[0];
    const int ck = cross_mfma(a) ? AD_KERNEL_CROSS_MFMA : AD_KERNEL_CROSS_GENERIC;
    for (int i = step0; i < step0 + n_steps; ++i) {
      const int32_t* anc_cur = w.anc + (size_t)((i - 1) & 1) * R * S;
      int32_t* anc_nxt = w.anc + (size_t)(i & 1) * R * S;
      hipLaunchKernelGGL(attdec_embed_kernel, dim3(R), dim3(128), 0, st, w.tok, d, i - 1, D.embed, a->pe,
                         std::sqrt((float)d), w.x);
      KCHK((int)hipGetLastError());
      // self: this step's K|V row goes to (layer, position i - 1, slot r) and stays there; cross: the utterance's
      // rows as begin projected them, shared by its beams
      KCHK(aed_decoder_blocks<T>(
          D, a->cfg, R, w.x, w.h, w.q, w.ao, w.hid,
          [&](int l, const AedLayerW& L, const T* h) {
            T* kvl = w.kvc + (size_t)l * S * R * 2 * d;
            EpiArgs e; e.bias = L.bkv_s; e.out = kvl + (size_t)(i - 1) * R * 2 * d; e.ldo = 2 * d;
            if (const int r = gemm<T>(EPI_STORE, ACT_NONE, h, d, (const T*)L.wkv_s, d, R, 2 * d, d, e, st)) return r;
            const int r = ad_self_attention<T>(w.q, kvl, anc_cur, S, i, R, N, H, dk, w.done, w.ao, st);
            return r == -1 ? (int)hipErrorInvalidValue : r;
          },
          [&](int l, const AedLayerW&, const T* q) {
            const int r = ad_cross_attention<T>(ck, q, w.mkv + (size_t)l * g.mem_rows * 2 * d, g.mem_rows, w.ustart,
                                                w.ulen, w.done, g.B, N, H, dk, g.ns, w.ao, w.part_o, w.part_ml, st);
            return r == -1 ? (int)hipErrorInvalidValue : r;
          },
          st));
      KCHK(vocab_logits<T>(w.h, R, (const T*)D.out_w, D.out_b, V, d, w.logits, V, st));
      KCHK(ctc_topk_rows(w.logits, R, V, N, 1, w.tv, w.ti, st));
      hipLaunchKernelGGL(attdec_prune_kernel, dim3(g.B), dim3(256), 0, st, i, N, R, S, a->cfg.eos, w.tv, w.ti, w.score,
                         w.tok, w.fin, anc_cur, anc_nxt, w.tr_parent, w.tr_token, w.tr_score, w.limit, w.done, w.steps,
                         w.words);
      KCHK((int)hipGetLastError());
    }
    return CFM_OK;
  }

  static cfm_status finish(const cfm_aed* a, const AdGeom& g, float penalty, void* ws, int32_t* tokens, int32_t* lens,
                           float* final_scores, int32_t* best, int32_t* tr_parent, int32_t* tr_token, float* tr_score,
                           hipStream_t st) {
    WS w = carve(a, ws, g, nullptr);
    hipLaunchKernelGGL(attdec_finish_kernel, dim3(g.B), dim3(64), 0, st, g.N, g.R, g.S, a->cfg.sos, a->cfg.eos, penalty,
                       w.score, w.steps, w.tr_parent, w.tr_token, tokens, lens, final_scores, best);
    KCHK((int)hipGetLastError());
    const size_t tr = (size_t)g.S * g.R * 4;
    if (tr_parent && tr_token && tr_score && tr > 0) {
      if (hipMemcpyAsync(tr_parent, w.tr_parent, tr, hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipMemcpyAsync(tr_token, w.tr_token, tr, hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipMemcpyAsync(tr_score, w.tr_score, tr, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return set_error(CFM_ERR_RUNTIME, "hipMemcpyAsync");
    }
    return CFM_OK;
  }
};

static bool ad_geom(const cfm_aed* h, int B, int beam, int mem_rows, int max_steps, AdGeom& g) {
  if (!h || B < 1 || beam < 1 || beam > BEAM_KMAX || beam > h->cfg.V || mem_rows < 0 || max_steps < 0 ||
      max_steps > AED_MAX_POS || (int64_t)B * beam > (1 << 20))
    return false;
  if (hipSetDevice(h->device) != hipSuccess) return false;
  g.B = B; g.N = beam; g.R = B * beam; g.mem_rows = mem_rows; g.S = max_steps;
  g.ns = ad_key_splits(B, h->cfg.H, mem_rows);
  return true;
}

#define AD_DISPATCH(CALL)                                              \
  switch (h->cfg.dtype) {                                              \
    case CFM_DTYPE_F32: return AttDec<float>::CALL;                    \
    case CFM_DTYPE_BF16: return AttDec<bf16>::CALL;                    \
    case CFM_DTYPE_F16: return AttDec<f16>::CALL;                      \
  }

}  // namespace cfm

using namespace cfm;

extern "C" {

size_t cfm_attdec_workspace_bytes(const cfm_aed* h, int32_t B, int32_t beam, int32_t mem_rows, int32_t max_steps) {
  AdGeom g;
  if (!ad_geom(h, B, beam, mem_rows, max_steps, g)) return 0;
  size_t t = 0;
  switch (h->cfg.dtype) {
    case CFM_DTYPE_F32: AttDec<float>::carve(h, nullptr, g, &t); break;
    case CFM_DTYPE_BF16: AttDec<bf16>::carve(h, nullptr, g, &t); break;
    case CFM_DTYPE_F16: AttDec<f16>::carve(h, nullptr, g, &t); break;
    default: return 0;
  }
  return t + 4096;
}

cfm_status cfm_attdec_begin(const cfm_aed* h, const float* mem, int32_t mem_rows, const int32_t* utt_start,
                            const int32_t* utt_len, const int32_t* limit, int32_t B, int32_t beam, int32_t max_steps,
                            void* state, size_t state_bytes, cfm_stream stream) {
  AdGeom g;
  if (!ad_geom(h, B, beam, mem_rows, max_steps, g))
    return set_error(CFM_ERR_VALUE, "attention decoding: bad handle / B / beam (1 .. 16, at most V) / mem_rows / max_steps");
  if (!state || !utt_start || !utt_len || !limit || (mem_rows > 0 && !mem)) return set_error(CFM_ERR_VALUE, "null argument");
  if ((reinterpret_cast<uintptr_t>(mem) | reinterpret_cast<uintptr_t>(state)) & 15)
    return set_error(CFM_ERR_VALUE, "memory rows / state must be 16-byte aligned");
  if (state_bytes < cfm_attdec_workspace_bytes(h, B, beam, mem_rows, max_steps))
    return set_error(CFM_ERR_VALUE, "attention decoding state too small");
  AD_DISPATCH(begin(h, g, mem, utt_start, utt_len, limit, state, (hipStream_t)stream))
  return set_error(CFM_ERR_VALUE, "attention decoding: unknown dtype");
}

cfm_status cfm_attdec_steps(const cfm_aed* h, void* state, int32_t B, int32_t beam, int32_t mem_rows, int32_t max_steps,
                            int32_t first_step, int32_t n_steps, cfm_stream stream) {
  AdGeom g;
  if (!ad_geom(h, B, beam, mem_rows, max_steps, g) || !state)
    return set_error(CFM_ERR_VALUE, "attention decoding: bad handle / state / geometry");
  if (n_steps < 0 || first_step < 1 || first_step - 1 > max_steps - n_steps)
    return set_error(CFM_ERR_VALUE, "attention decoding: steps outside 1 .. max_steps");
  AD_DISPATCH(steps(h, g, first_step, n_steps, state, (hipStream_t)stream))
  return set_error(CFM_ERR_VALUE, "attention decoding: unknown dtype");
}

cfm_status cfm_attdec_finish(const cfm_aed* h, void* state, int32_t B, int32_t beam, int32_t mem_rows, int32_t max_steps,
                             float length_penalty, int32_t* tokens, int32_t* lengths, float* final_scores, int32_t* best,
                             int32_t* trace_parent, int32_t* trace_token, float* trace_score, cfm_stream stream) {
  AdGeom g;
  if (!ad_geom(h, B, beam, mem_rows, max_steps, g) || !state)
    return set_error(CFM_ERR_VALUE, "attention decoding: bad handle / state / geometry");
  if (!tokens || !lengths || !final_scores || !best) return set_error(CFM_ERR_VALUE, "null argument");
  AD_DISPATCH(finish(h, g, length_penalty, state, tokens, lengths, final_scores, best, trace_parent, trace_token,
                     trace_score, (hipStream_t)stream))
  return set_error(CFM_ERR_VALUE, "attention decoding: unknown dtype");
}

cfm_status cfm_op_decode_attention(int32_t dtype, int32_t kernel, const void* q, void* out, int32_t B, int32_t beam,
                                   int32_t H, int32_t dk, const void* kv, int32_t kv_rows, const int32_t* ancestry,
                                   int32_t ancestry_ld, int32_t n_keys, const int32_t* utt_start, const int32_t* utt_len,
                                   int32_t n_split, float* scratch, cfm_stream stream) {
  static const char* const KNAME[] = {"self-gather", "cross-generic", "cross-mfma"};
  if (kernel < 0 || kernel > 2) return set_error(CFM_ERR_VALUE, "decode attention: unknown kernel");
  if (dtype != CFM_DTYPE_F32 && dtype != CFM_DTYPE_BF16 && dtype != CFM_DTYPE_F16)
    return set_error(CFM_ERR_VALUE, "decode attention: unknown dtype");
  if (!q || !out || !kv) return set_error(CFM_ERR_VALUE, "decode attention: null argument");
  if (B <= 0 || beam <= 0 || beam > BEAM_KMAX || H <= 0 || dk <= 0 || kv_rows <= 0)
    return set_error(CFM_ERR_VALUE, "decode attention: bad B / beam / H / dk / kv_rows");
  const bool takes = kernel == AD_KERNEL_CROSS_MFMA ? ad_cross_mfma_takes(dtype, dk) : (dk % 16 == 0 && dk <= 128);
  if (!takes)
    return set_error(CFM_ERR_ASSERT, std::string("decode attention: the ") + KNAME[kernel] +
                                         " kernel does not take this configuration");
  hipStream_t st = (hipStream_t)stream;
  const int R = B * beam, d = H * dk;
  int r = -1;
  if (kernel == AD_KERNEL_SELF) {
    if (n_keys < 1 || n_keys > kv_rows || (n_keys > 1 && (!ancestry || ancestry_ld < n_keys - 1)))
      return set_error(CFM_ERR_VALUE, "decode attention: bad n_keys / ancestry");
#define AD_OP_SELF(T_) \
  r = ad_self_attention<T_>((const T_*)q, (const T_*)kv, ancestry, ancestry_ld, n_keys, R, beam, H, dk, nullptr, (T_*)out, st)
    if (dtype == CFM_DTYPE_F32) AD_OP_SELF(float);
    else if (dtype == CFM_DTYPE_F16) AD_OP_SELF(f16);
    else AD_OP_SELF(bf16);
#undef AD_OP_SELF
  } else {
    if (!utt_start || !utt_len || n_split < 1 || n_split > ATTDEC_MAX_SPLIT || (n_split > 1 && !scratch))
      return set_error(CFM_ERR_VALUE, "decode attention: bad utterance ranges / n_split / scratch");
    float* part_o = scratch;
    float* part_ml = scratch ? scratch + (size_t)n_split * R * d : nullptr;
#define AD_OP_CROSS(T_)                                                                                              \
  r = ad_cross_attention<T_>(kernel, (const T_*)q, (const T_*)kv, kv_rows, utt_start, utt_len, nullptr, B, beam, H, dk, \
                             n_split, (T_*)out, part_o, part_ml, st)
    if (dtype == CFM_DTYPE_F32) AD_OP_CROSS(float);
    else if (dtype == CFM_DTYPE_F16) AD_OP_CROSS(f16);
    else AD_OP_CROSS(bf16);
#undef AD_OP_CROSS
  }
  if (r == -1)
    return set_error(CFM_ERR_ASSERT, std::string("decode attention: the ") + KNAME[kernel] +
                                         " kernel does not take this configuration");
  if (r) return set_error(CFM_ERR_RUNTIME, std::string("decode attention (") + KNAME[kernel] + "): " +
                                               hipGetErrorString((hipError_t)r));
  return CFM_OK;
}

}  // extern "C"
