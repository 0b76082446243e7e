// Attention decoder consumer (model: hybrid CTC / attention checkpoints): the left-to-right and right-to-left
// TransformerDecoder of the reference (modules/decoder.py:35-226, 330-484, modules/decoder_layer.py:67-149,
// normalize_before path, dropout off) scoring the CTC prefix beam n-best against the encoder output, as
// attention_rescoring consumes it (modules/search.py:358-439 over asr_model.py:399-492).
//
// Everything works on PACKED token rows: hypothesis h = rows [hyp_start[h], + hyp_len[h]) (its sos row and its
// n tokens), a causal segment of its own -- the reference pads an utterance's hypotheses to a common length and
// masks the padded keys, which is the same thing -- and reads the encoder rows of its utterance
// [utt_row_start[u], + utt_row_len[u]) where they lie: the memory is never repeated per hypothesis, no
// [n_hyps, H, L, T'] score tensor and no [n_hyps, L, V] log-softmax exist.  One call, per direction:
//
//   aed_prepare_kernel   (once per call) validates every hypothesis (ranges, utterance, token ids) and writes its two
//                        segment descriptors (self: causal over its own rows; cross: its utterance's rows); a bad one
//                        gets empty descriptors and sets the status word, the others are unaffected
//   seg_scan_kernel      tile_off[s] = exclusive prefix sum of the segments' workgroup (16- or 64-query tile) counts
//   aed_embed_kernel     x = embed[token] * sqrt(d) + pe[pos] (embedding.py:31-58), the right-to-left direction
//                        reading the hypothesis' tokens in reverse by index; and the row's target id
//   the decoder blocks   aed_decoder_blocks (aed.h), with  self: K|V GEMM -> causal segment attention
//                        cross: K|V GEMM over ALL memory rows of the batch (once per layer) -> cross segment attention
//   then in row slabs: output_layer GEMM (vocab_logits) -> aed_head_kernel: logit[target] - lse, one float per row
//
// Segment attention (one kernel family for both uses): descriptor (Q0, NQ, K0, NK, CAUSAL): queries rows
// [Q0, Q0 + NQ) of q, keys rows [K0, K0 + NK) of the K|V rows, query i sees keys j < NK (causal: j <= i);
// out_i = softmax_j(q_i . k_j / sqrt(dk)) . V, online softmax in f32, no score tensor in memory; a query without a
// visible key gives a zero row.  One wave = 16 queries of one head; workgroup (tile, head), tile -> segment by
// binary search in tile_off (generic: one wave, 16 queries; mfma: four waves, 64 queries of one segment, sharing
// each staged key tile).  Rows no descriptor covers are never read or written.
//   generic   any type, dk a multiple of 16 up to 128: lane (query, quarter of the head's dims), keys one at a time
//   mfma      bf16 / f16, dk 64 / 128: the 32-key tile of attn_core.h, staged once for the workgroup's four waves
// Loops are bounded by the descriptor lengths; nothing waits on another workgroup; plain vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cfm.h"
#include "../../include/cfm_ops.h"
#include "aed.h"
#include "attn_core.h"
#include "cfm_common.h"
#include "cfm_kernels.h"
#include "status.h"

namespace cfm {

enum { SD_Q0 = 0, SD_NQ = 1, SD_K0 = 2, SD_NK = 3, SD_CAUSAL = 4, SD_INTS = 8 };
enum { AED_ST_HYP = 1, AED_ST_UTT = 2, AED_ST_TOKEN = 3, AED_ST_TILES = 4 };

struct Seg {
  int q0, nq, k0, nk, causal;
};

// a descriptor whose ranges lie inside their arrays, else an empty one (bad = true)
CFM_DEV Seg seg_load(const int32_t* __restrict__ desc, int s, int q_rows, int k_rows, bool& bad) {
  const int32_t* p = desc + (size_t)s * SD_INTS;
  Seg g{p[SD_Q0], p[SD_NQ], p[SD_K0], p[SD_NK], p[SD_CAUSAL]};
  bad = g.q0 < 0 || g.nq < 0 || g.q0 > q_rows || g.nq > q_rows - g.q0 || g.k0 < 0 || g.nk < 0 || g.k0 > k_rows ||
        g.nk > k_rows - g.k0;
  if (bad) g.nq = 0;
  return g;
}

// tile_off[0 .. n_seg]: exclusive prefix sum of ceil(NQ / tq) (tq = queries per workgroup of the kernel that
// follows), capped at `cap` (the launch's tile count)
__global__ __launch_bounds__(256) void seg_scan_kernel(const int32_t* __restrict__ desc, int n_seg, int q_rows, int k_rows,
                                                       int tq, int cap, int32_t* __restrict__ tile_off,
                                                       int32_t* __restrict__ status) {
  __shared__ int part[256];
  const int tid = threadIdx.x;
  const int per = (n_seg + 255) / 256;
  const int s0 = min(tid * per, n_seg), s1 = min(s0 + per, n_seg);
  int sum = 0;
  bool any_bad = false;
  for (int s = s0; s < s1; ++s) {
    bool bad;
    const Seg g = seg_load(desc, s, q_rows, k_rows, bad);
    any_bad |= bad;
    sum += (g.nq + tq - 1) / tq;
  }
  part[tid] = sum;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < tid; ++t) base += part[t];
  for (int s = s0; s < s1; ++s) {
    bool bad;
    const Seg g = seg_load(desc, s, q_rows, k_rows, bad);
    tile_off[s] = min(base, cap);
    base += (g.nq + tq - 1) / tq;
  }
  if (tid == 255) tile_off[n_seg] = min(base, cap);
  if (any_bad) *status = AED_ST_HYP;
  if (tid == 255 && base > cap) *status = AED_ST_TILES;   // overlapping query ranges: more tiles than rows allow
}

// this workgroup's segment and tile of TQ queries; false = past the last tile
template <int TQ>
CFM_DEV bool seg_find(const int32_t* __restrict__ desc, const int32_t* __restrict__ tile_off, int n_seg, int q_rows,
                      int k_rows, Seg& g, int& qi0, int& nqt) {
  const int tile = blockIdx.x;
  if (tile >= tile_off[n_seg]) return false;
  int lo = 0, hi = n_seg - 1;   // last s with tile_off[s] <= tile (segments without tiles share an offset)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_off[mid] <= tile) lo = mid; else hi = mid - 1;
  }
  bool bad;
  g = seg_load(desc, lo, q_rows, k_rows, bad);
  qi0 = (tile - tile_off[lo]) * TQ;
  nqt = min(TQ, g.nq - qi0);
  return nqt > 0;
}

template <typename T, int DKQ>
__global__ __launch_bounds__(64) void seg_attn_generic_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ k,
                                                              const T* __restrict__ v, int ldkv, T* __restrict__ out,
                                                              int ldo, const int32_t* __restrict__ desc,
                                                              const int32_t* __restrict__ tile_off, int n_seg, int q_rows,
                                                              int k_rows, float scale) {
  typedef typename Vec4<T>::type V4;
  constexpr int DK = 4 * DKQ;
  Seg g;
  int qi0, nqt;
  if (!seg_find<16>(desc, tile_off, n_seg, q_rows, k_rows, g, qi0, nqt)) return;
  const int lane = threadIdx.x, fr = lane & 15, part = lane >> 4;
  const int col = blockIdx.y * DK + part * DKQ;
  const int qi = qi0 + min(fr, nqt - 1);
  float qv[DKQ], acc[DKQ];
  {
    const T* qp = q + (size_t)(g.q0 + qi) * ldq + col;
#pragma unroll
    for (int e = 0; e < DKQ; e += 4) {
      const V4 t = *reinterpret_cast<const V4*>(qp + e);
#pragma unroll
      for (int c = 0; c < 4; ++c) { qv[e + c] = to_f32(t[c]); acc[e + c] = 0.f; }
    }
  }
  const int kend = g.causal ? min(g.nk, qi0 + nqt) : g.nk;   // keys any query of the tile sees
  const int lim = g.causal ? min(g.nk, qi + 1) : g.nk;       // keys j < lim are visible to this lane's query
  float m = -INFINITY, l = 0.f;
  for (int j = 0; j < kend; ++j) {
    const T* kp = k + (size_t)(g.k0 + j) * ldkv + col;
    const T* vp = v + (size_t)(g.k0 + j) * ldkv + col;
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
    if (j < lim) {
      const float mx = fmaxf(m, s);
      const float alpha = __expf(m - mx);   // first visible key: exp(-inf) = 0
      const float p = __expf(s - mx);
      l = l * alpha + p;
#pragma unroll
      for (int e = 0; e < DKQ; ++e) acc[e] = acc[e] * alpha + p * vv[e];
      m = mx;
    }
  }
  if (fr < nqt) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    T* op = out + (size_t)(g.q0 + qi) * ldo + col;
#pragma unroll
    for (int e = 0; e < DKQ; e += 4) {
      V4 t;
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = from_f32<T>(acc[e + c] * inv);
      *reinterpret_cast<V4*>(op + e) = t;
    }
  }
}

constexpr int SEG_MFMA_TQ = 64;   // queries per workgroup of the MFMA kernel: four waves of 16

template <typename T, int DK>
__global__ __launch_bounds__(256) void seg_attn_mfma_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ k,
                                                            const T* __restrict__ v, int ldkv, T* __restrict__ out, int ldo,
                                                            const int32_t* __restrict__ desc,
                                                            const int32_t* __restrict__ tile_off, int n_seg, int q_rows,
                                                            int k_rows, float scale) {
  typedef typename Vec4<T>::type V4;
  typedef typename Frag<T>::type F8;
  typedef AttnTile<DK> G;   // the tile's geometry and key permutation: attn_core.h
  constexpr int KS = G::KS, NJ = G::NJ, KP = G::KP, VP = G::VP, CH = G::CH;
  __shared__ __attribute__((aligned(16))) T ks[32 * KP];
  __shared__ __attribute__((aligned(16))) T vt[DK * VP];
  Seg g;
  int qb0, nqb;   // the workgroup's 64 queries: the segment's [qb0, qb0 + nqb)
  if (!seg_find<SEG_MFMA_TQ>(desc, tile_off, n_seg, q_rows, k_rows, g, qb0, nqb)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, gq = lane >> 4;
  const int col = blockIdx.y * DK;
  const int qw0 = qb0 + 16 * wave;                  // this wave's 16 queries (past the segment: repeats, never stored)
  const bool stores = 16 * wave + fr < nqb;
  const int qi = min(qw0 + fr, qb0 + nqb - 1);      // clamped: the lanes past the segment repeat its last query
  F8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = ld8<T>(q + (size_t)(g.q0 + qi) * ldq + col + 32 * s + 8 * gq);
  f32x4 o[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) o[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int kend = g.causal ? min(g.nk, qb0 + nqb) : g.nk;                      // keys any query of the workgroup sees
  const int kend_w = g.causal ? min(g.nk, min(qw0 + 16, qb0 + nqb)) : g.nk;    // ... of this wave
  const int lim = g.causal ? min(g.nk, qi + 1) : g.nk;                          // keys j < lim: this lane's query
  float m = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < kend; j0 += 32) {
    __syncthreads();   // the previous tile's reads are done
    // K rows and V^T of keys j0 .. j0 + 31 (rows past the segment repeat its last row: their p is 0)
#pragma unroll
    for (int c = tid; c < 32 * CH; c += 256) {
      const int key = c / CH, ch = c - key * CH;
      const size_t row = (size_t)(g.k0 + min(j0 + key, g.nk - 1)) * ldkv + col + 8 * ch;
      st8<T>(ks + key * KP + 8 * ch, ld8<T>(k + row));
      const F8 t = ld8<T>(v + row);
#pragma unroll
      for (int e = 0; e < 8; ++e) vt[(8 * ch + e) * VP + key] = t[e];
    }
    __syncthreads();
    if (j0 >= kend_w) continue;   // wave-uniform: causal tiles past this wave's queries
    // S^T: keys j0 + 16 t2 + (4 gq + r) on the rows, this lane's query on the column
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
        const int j = j0 + 16 * t2 + 4 * gq + r;
        const float sv = j < lim ? a[r] * scale : -INFINITY;
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
  if (stores) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    T* op = out + (size_t)(g.q0 + qi) * ldo + col + 4 * gq;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      V4 t;
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] = from_f32<T>(o[j][r] * inv);
      *reinterpret_cast<V4*>(op + 16 * j) = t;
    }
  }
}

static int seg_tile_cap(int q_rows, int n_seg, int tq) { return (q_rows + tq - 1) / tq + n_seg; }
// tile offsets for a kernel whose workgroups take tq queries (16: generic, SEG_MFMA_TQ: mfma)
static int seg_scan(const int32_t* desc, int n_seg, int q_rows, int k_rows, int tq, int32_t* tile_off, int32_t* status,
                    hipStream_t st) {
  hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(256), 0, st, desc, n_seg, q_rows, k_rows, tq,
                     seg_tile_cap(q_rows, n_seg, tq), tile_off, status);
  CFM_CHECK_LAUNCH();
  return 0;
}

// -1: the kernel does not take this head dim
template <typename T>
static int seg_attention_generic(const T* q, int ldq, const T* k, const T* v, int ldkv, T* out, int ldo,
                                 const int32_t* desc, const int32_t* tile_off, int n_seg, int q_rows, int k_rows, int H,
                                 int dk, hipStream_t st) {
  if (dk < 16 || dk > 128 || dk % 16) return -1;
  const int cap = seg_tile_cap(q_rows, n_seg, 16);
  if (cap <= 0 || n_seg <= 0) return 0;
  const float scale = 1.0f / std::sqrt((float)dk);
#define SEG_GEN(Q_)                                                                                                  \
  case Q_:                                                                                                           \
    hipLaunchKernelGGL((seg_attn_generic_kernel<T, Q_>), dim3(cap, H), dim3(64), 0, st, q, ldq, k, v, ldkv, out, ldo, \
                       desc, tile_off, n_seg, q_rows, k_rows, scale);                                                \
    break;
  switch (dk / 4) {
    SEG_GEN(4) SEG_GEN(8) SEG_GEN(12) SEG_GEN(16) SEG_GEN(20) SEG_GEN(24) SEG_GEN(28) SEG_GEN(32)
    default: return -1;
  }
#undef SEG_GEN
  CFM_CHECK_LAUNCH();
  return 0;
}

template <typename T>
static int seg_attention_mfma(const T* q, int ldq, const T* k, const T* v, int ldkv, T* out, int ldo, const int32_t* desc,
                              const int32_t* tile_off, int n_seg, int q_rows, int k_rows, int H, int dk, hipStream_t st) {
  if constexpr (sizeof(T) != 2) {
    return -1;
  } else {
    if (dk != 64 && dk != 128) return -1;
    if (ldq % 8 || ldkv % 8 || ldo % 4) return -1;
    const int cap = seg_tile_cap(q_rows, n_seg, SEG_MFMA_TQ);
    if (cap <= 0 || n_seg <= 0) return 0;
    const float scale = 1.0f / std::sqrt((float)dk);
    if (dk == 64)
      hipLaunchKernelGGL((seg_attn_mfma_kernel<T, 64>), dim3(cap, H), dim3(256), 0, st, q, ldq, k, v, ldkv, out, ldo, desc,
                         tile_off, n_seg, q_rows, k_rows, scale);
    else
      hipLaunchKernelGGL((seg_attn_mfma_kernel<T, 128>), dim3(cap, H), dim3(256), 0, st, q, ldq, k, v, ldkv, out, ldo, desc,
                         tile_off, n_seg, q_rows, k_rows, scale);
    CFM_CHECK_LAUNCH();
    return 0;
  }
}

// ----------------------------------------------------------------------------- decoder kernels
// One workgroup per hypothesis: ranges, utterance and token ids checked; descriptors written (empty when bad).
__global__ __launch_bounds__(256) void aed_prepare_kernel(const int32_t* __restrict__ tokens, int n_tok,
                                                          const int32_t* __restrict__ hyp_start,
                                                          const int32_t* __restrict__ hyp_len,
                                                          const int32_t* __restrict__ hyp_utt, int n_hyps,
                                                          const int32_t* __restrict__ utt_start,
                                                          const int32_t* __restrict__ utt_len, int B, int mem_rows, int V,
                                                          int32_t* __restrict__ d_self, int32_t* __restrict__ d_cross,
                                                          int32_t* __restrict__ status) {
  const int h = blockIdx.x;
  const int s = hyp_start[h], n = hyp_len[h], u = hyp_utt[h];
  int code = 0;
  int us = 0, ul = 0;
  if (s < 0 || n < 1 || s > n_tok || n > n_tok - s || n > AED_MAX_POS) code = AED_ST_HYP;
  else if (u < 0 || u >= B) code = AED_ST_UTT;
  else {
    us = utt_start[u];
    ul = utt_len[u];
    if (us < 0 || ul < 0 || us > mem_rows || ul > mem_rows - us) code = AED_ST_UTT;
  }
  if (code == 0) {
    int bad = 0;
    for (int j = 1 + (int)threadIdx.x; j < n; j += 256) {   // row 0 is the sos row whatever it holds
      const int t = tokens[s + j];
      bad |= (t < 0 || t >= V);
    }
    if (__syncthreads_or(bad)) code = AED_ST_TOKEN;
  }
  if (threadIdx.x == 0) {
    const bool ok = code == 0;
    int32_t* a = d_self + (size_t)h * SD_INTS;
    int32_t* c = d_cross + (size_t)h * SD_INTS;
    a[SD_Q0] = ok ? s : 0; a[SD_NQ] = ok ? n : 0; a[SD_K0] = ok ? s : 0; a[SD_NK] = ok ? n : 0; a[SD_CAUSAL] = 1;
    c[SD_Q0] = ok ? s : 0; c[SD_NQ] = ok ? n : 0; c[SD_K0] = ok ? us : 0; c[SD_NK] = ok ? ul : 0; c[SD_CAUSAL] = 0;
    a[5] = a[6] = a[7] = c[5] = c[6] = c[7] = 0;
    if (!ok) *status = code;
  }
}

// x rows and targets of one hypothesis (one workgroup); reverse: the tokens read back to front by index
__global__ __launch_bounds__(256) void aed_embed_kernel(const int32_t* __restrict__ tokens,
                                                        const int32_t* __restrict__ d_self, int d, int sos, int eos,
                                                        int reverse, const float* __restrict__ embed,
                                                        const float* __restrict__ pe, float xscale, float* __restrict__ x,
                                                        int32_t* __restrict__ target) {
  const int32_t* a = d_self + (size_t)blockIdx.x * SD_INTS;
  const int s = a[SD_Q0], n = a[SD_NQ];   // n = tokens + 1; 0 for a rejected hypothesis
  const int d4 = d >> 2;
  for (int idx = threadIdx.x; idx < n * d4; idx += 256) {
    const int j = idx / d4, c = idx - j * d4;
    // input of row j: sos, then the tokens (row 1 + i of the hypothesis holds token i) forwards or backwards
    const int tok = j == 0 ? sos : tokens[s + (reverse ? n - j : j)];
    const float4 e = reinterpret_cast<const float4*>(embed + (size_t)tok * d)[c];
    const float4 p = reinterpret_cast<const float4*>(pe + (size_t)j * d)[c];
    reinterpret_cast<float4*>(x + (size_t)(s + j) * d)[c] =
        make_float4(e.x * xscale + p.x, e.y * xscale + p.y, e.z * xscale + p.z, e.w * xscale + p.w);
  }
  for (int j = threadIdx.x; j < n; j += 256)
    target[s + j] = j == n - 1 ? eos : tokens[s + (reverse ? n - 1 - j : j + 1)];
}

// out[row0 + r] = logits[r][target] - lse(logits[r]) (lse formed as log_softmax_rows forms it), one wave per row;
// rows without a target (rejected hypotheses, rows of no hypothesis) are left as they are
__global__ __launch_bounds__(256) void aed_head_kernel(const float* __restrict__ logits, int M, int V,
                                                       const int32_t* __restrict__ target, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int t = target[row];
  if (t < 0 || t >= V) return;
  const float* p = logits + (size_t)row * V;
  float mx = -INFINITY;
  for (int v = lane; v < V; v += 64) mx = fmaxf(mx, p[v]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int v = lane; v < V; v += 64) s += __expf(p[v] - mx);
  const float lse = mx + __logf(wave_sum(s));
  if (lane == 0) out[row] = p[t] - lse;
}

template <typename T>
struct AedT : public cfm_aed {
  struct WS {
    int32_t *status, *d_self, *d_cross, *tile_off, *target;
    float *x, *logits;
    T *h, *q, *kv, *ao, *hid, *memT, *mkv;
  };
  int slab_rows() const { return logit_slab_rows(cfg.V); }   // rows of the output head's logit slab
  WS carve(void* base, int tokens, int mem_rows, size_t* total) const {
    const size_t d = cfg.d, ff = cfg.ff, n = (size_t)std::max(tokens, 1), mr = (size_t)std::max(mem_rows, 1);
    Carver c(base);
    WS w;
    w.status = c.take<int32_t>(64);
    w.d_self = c.take<int32_t>(n * SD_INTS);
    w.d_cross = c.take<int32_t>(n * SD_INTS);
    w.tile_off = c.take<int32_t>(n + 1);
    w.target = c.take<int32_t>(n);
    w.x = c.take<float>(n * d);
    w.h = c.take<T>(n * d);
    w.q = c.take<T>(n * d);
    w.kv = c.take<T>(n * 2 * d);
    w.ao = c.take<T>(n * d);
    w.hid = c.take<T>(n * ff);
    w.memT = sizeof(T) == 4 ? nullptr : c.take<T>(mr * d);
    w.mkv = c.take<T>(mr * 2 * d);
    w.logits = c.take<float>((size_t)std::min<size_t>(n, slab_rows()) * cfg.V);
    if (total) *total = c.off;
    return w;
  }
  size_t ws_bytes(int tokens, int mem_rows) const override {
    size_t t = 0;
    carve(nullptr, tokens, mem_rows, &t);
    return t + 4096;
  }

  bool uses_mfma() const { return sizeof(T) == 2 && (cfg.d / cfg.H == 64 || cfg.d / cfg.H == 128); }
  int attention(const T* q, const T* kv, T* out, const int32_t* desc, const int32_t* tile_off, int n_seg, int q_rows,
                int k_rows, hipStream_t st) const {
    const int d = cfg.d, H = cfg.H, dk = d / H;
    int r = -1;
    if (uses_mfma())
      r = seg_attention_mfma<T>(q, d, kv, kv + d, 2 * d, out, d, desc, tile_off, n_seg, q_rows, k_rows, H, dk, st);
    else
      r = seg_attention_generic<T>(q, d, kv, kv + d, 2 * d, out, d, desc, tile_off, n_seg, q_rows, k_rows, H, dk, st);
    return r == -1 ? (int)hipErrorInvalidValue : r;
  }

  cfm_status score(const float* mem, int mem_rows, const int32_t* utt_start, const int32_t* utt_len, int B,
                   const int32_t* tokens, int n_tok, const int32_t* hyp_start, const int32_t* hyp_len,
                   const int32_t* hyp_utt, int n_hyps, int dirs, float* out_l2r, float* out_r2l, void* ws, size_t wsb,
                   hipStream_t st) const override {
    const int d = cfg.d, V = cfg.V;
    if (wsb < ws_bytes(n_tok, mem_rows)) return set_error(CFM_ERR_VALUE, "attention decoder workspace too small");
    WS w = carve(ws, n_tok, mem_rows, nullptr);
    if (hipMemsetAsync(w.status, 0, 256, st) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
    hipLaunchKernelGGL(aed_prepare_kernel, dim3(n_hyps), dim3(256), 0, st, tokens, n_tok, hyp_start, hyp_len, hyp_utt,
                       n_hyps, utt_start, utt_len, B, mem_rows, V, w.d_self, w.d_cross, w.status);
    KCHK((int)hipGetLastError());
    // one scan serves both attention uses: they share the query ranges
    KCHK(seg_scan(w.d_self, n_hyps, n_tok, n_tok, uses_mfma() ? SEG_MFMA_TQ : 16, w.tile_off, w.status, st));
    const T* memT;
    KCHK(aed_memory_rows<T>(mem, mem_rows, d, w.memT, st, &memT));
    for (int dir = 0; dir < 2; ++dir) {
      if (!(dirs >> dir & 1)) continue;
      const AedDecoderW& D = dec[dir];
      float* outp = dir == 0 ? out_l2r : out_r2l;
      // rows of no (accepted) hypothesis: x zero (finite through the row-wise kernels), no target (never written)
      if (hipMemsetAsync(w.x, 0, (size_t)n_tok * d * sizeof(float), st) != hipSuccess ||
          hipMemsetAsync(w.target, 0xff, (size_t)n_tok * sizeof(int32_t), st) != hipSuccess)
        return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
      hipLaunchKernelGGL(aed_embed_kernel, dim3(n_hyps), dim3(256), 0, st, tokens, w.d_self, d, cfg.sos, cfg.eos, dir,
                         D.embed, pe, std::sqrt((float)d), w.x, w.target);
      KCHK((int)hipGetLastError());
      // self: causal inside each hypothesis; cross: K|V of every memory row of the batch in one GEMM per block
      KCHK(aed_decoder_blocks<T>(
          D, cfg, n_tok, w.x, w.h, w.q, w.ao, w.hid,
          [&](int, const AedLayerW& L, const T* h) {
            EpiArgs e; e.bias = L.bkv_s; e.out = w.kv; e.ldo = 2 * d;
            if (const int r = gemm<T>(EPI_STORE, ACT_NONE, h, d, (const T*)L.wkv_s, d, n_tok, 2 * d, d, e, st)) return r;
            return attention(w.q, w.kv, w.ao, w.d_self, w.tile_off, n_hyps, n_tok, n_tok, st);
          },
          [&](int, const AedLayerW& L, const T* q) {
            if (const int r = aed_memory_kv<T>(L, memT, mem_rows, d, w.mkv, st)) return r;
            return attention(q, w.mkv, w.ao, w.d_cross, w.tile_off, n_hyps, n_tok, mem_rows, st);
          },
          st));
      const int slab = slab_rows();   // output layer in row slabs
      for (int r0 = 0; r0 < n_tok; r0 += slab) {
        const int nr = std::min(slab, n_tok - r0);
        KCHK(vocab_logits<T>(w.h + (size_t)r0 * d, nr, (const T*)D.out_w, D.out_b, V, d, w.logits, V, st));
        hipLaunchKernelGGL(aed_head_kernel, dim3((nr + 3) / 4), dim3(256), 0, st, w.logits, nr, V, w.target + r0,
                           outp + r0);
        KCHK((int)hipGetLastError());
      }
    }
    return CFM_OK;
  }
};

static uint16_t aed_bf16_bits(float f) {   // round-to-nearest-even f32 -> bf16 bits (host)
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffff) ? 0x40 : 0));
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <typename T>
static cfm_status aed_build(const cfm_aed_config& cfg, const std::map<std::string, std::pair<const float*, int64_t>>& hw,
                            int device, cfm_aed** out) {
  auto M = std::make_unique<AedT<T>>();
  M->cfg = cfg;
  M->device = device;
  const int d = cfg.d, ff = cfg.ff, V = cfg.V;
  std::vector<char> img;
  std::vector<std::pair<size_t, void**>> fix;
  auto reserve = [&](size_t bytes) {
    const size_t off = align_up(img.size());
    img.resize(off + align_up(bytes));
    return off;
  };
  auto get = [&](const std::string& k, int64_t numel) -> const float* {
    auto it = hw.find(k);
    if (it == hw.end()) throw std::string("missing weight " + k);
    if (it->second.second != numel)
      throw std::string("weight " + k + ": numel " + std::to_string(it->second.second) + " != " + std::to_string(numel));
    return it->second.first;
  };
  auto put_f32 = [&](const float* src, size_t n, float** slot) {
    const size_t off = reserve(n * 4);
    std::memcpy(img.data() + off, src, n * 4);
    fix.push_back({off, (void**)slot});
  };
  // one or two [rows, K] matrices stacked along N, as T
  auto put_T = [&](const float* a, const float* b, size_t n_each, void** slot) {
    const size_t total = n_each * (b ? 2 : 1);
    const size_t off = reserve(total * sizeof(T));
    T* p = reinterpret_cast<T*>(img.data() + off);
    for (size_t i = 0; i < total; ++i) {
      const float f = i < n_each ? a[i] : b[i - n_each];
      if constexpr (sizeof(T) == 4) p[i] = f;
      else if constexpr (std::is_same<T, f16>::value) p[i] = (f16)f;
      else { const uint16_t r = aed_bf16_bits(f); std::memcpy(&p[i], &r, 2); }
    }
    fix.push_back({off, slot});
  };
  auto put_bias2 = [&](const float* a, const float* b, size_t n, float** slot) {
    const size_t off = reserve(2 * n * 4);
    std::memcpy(img.data() + off, a, n * 4);
    std::memcpy(img.data() + off + n * 4, b, n * 4);
    fix.push_back({off, (void**)slot});
  };
  try {
    {   // PositionalEncoding.pe (embedding.py:31-38): f32 arguments as the reference forms them
      const size_t off = reserve((size_t)AED_MAX_POS * d * 4);
      float* p = reinterpret_cast<float*>(img.data() + off);
      for (int i = 0; i < d / 2; ++i) {
        const float div = (float)std::exp((double)((float)(2 * i) * (float)(-(std::log(10000.0) / d))));
        for (int pos = 0; pos < AED_MAX_POS; ++pos) {
          const float a = (float)pos * div;
          p[(size_t)pos * d + 2 * i] = (float)std::sin((double)a);
          p[(size_t)pos * d + 2 * i + 1] = (float)std::cos((double)a);
        }
      }
      fix.push_back({off, (void**)&M->pe});
    }
    for (int dir = 0; dir < 2; ++dir) {
      const std::string P = dir == 0 ? "decoder.left_decoder." : "decoder.right_decoder.";
      AedDecoderW& D = M->dec[dir];
      if (dir == 1 && !hw.count(P + "embed.0.weight")) continue;   // decoder: transformer (no right decoder)
      D.present = true;
      const int nb = dir == 0 ? cfg.num_blocks : cfg.r_num_blocks;
      D.layers.resize(nb);
      put_f32(get(P + "embed.0.weight", (int64_t)V * d), (size_t)V * d, &D.embed);
      put_f32(get(P + "after_norm.weight", d), d, &D.an_w);
      put_f32(get(P + "after_norm.bias", d), d, &D.an_b);
      put_T(get(P + "output_layer.weight", (int64_t)V * d), nullptr, (size_t)V * d, &D.out_w);
      put_f32(get(P + "output_layer.bias", V), V, &D.out_b);
      for (int l = 0; l < nb; ++l) {
        AedLayerW& L = D.layers[l];
        const std::string Q = P + "decoders." + std::to_string(l) + ".";
        const size_t dd = (size_t)d * d;
        auto W = [&](const std::string& k, int64_t n) { return get(Q + k, n); };
        put_T(W("self_attn.linear_q.weight", dd), nullptr, dd, &L.wq_s);
        put_T(W("self_attn.linear_k.weight", dd), W("self_attn.linear_v.weight", dd), dd, &L.wkv_s);
        put_T(W("self_attn.linear_out.weight", dd), nullptr, dd, &L.wo_s);
        put_T(W("src_attn.linear_q.weight", dd), nullptr, dd, &L.wq_c);
        put_T(W("src_attn.linear_k.weight", dd), W("src_attn.linear_v.weight", dd), dd, &L.wkv_c);
        put_T(W("src_attn.linear_out.weight", dd), nullptr, dd, &L.wo_c);
        put_T(W("feed_forward.w_1.weight", (int64_t)ff * d), nullptr, (size_t)ff * d, &L.w1);
        put_T(W("feed_forward.w_2.weight", (int64_t)ff * d), nullptr, (size_t)ff * d, &L.w2);
        put_f32(W("self_attn.linear_q.bias", d), d, &L.bq_s);
        put_bias2(W("self_attn.linear_k.bias", d), W("self_attn.linear_v.bias", d), d, &L.bkv_s);
        put_f32(W("self_attn.linear_out.bias", d), d, &L.bo_s);
        put_f32(W("src_attn.linear_q.bias", d), d, &L.bq_c);
        put_bias2(W("src_attn.linear_k.bias", d), W("src_attn.linear_v.bias", d), d, &L.bkv_c);
        put_f32(W("src_attn.linear_out.bias", d), d, &L.bo_c);
        put_f32(W("feed_forward.w_1.bias", ff), ff, &L.b1);
        put_f32(W("feed_forward.w_2.bias", d), d, &L.b2);
        put_f32(W("norm1.weight", d), d, &L.n1w); put_f32(W("norm1.bias", d), d, &L.n1b);
        put_f32(W("norm2.weight", d), d, &L.n2w); put_f32(W("norm2.bias", d), d, &L.n2b);
        put_f32(W("norm3.weight", d), d, &L.n3w); put_f32(W("norm3.bias", d), d, &L.n3b);
      }
    }
  } catch (const std::string& e) {
    return set_error(CFM_ERR_VALUE, e);
  }
  // (the slots point into D.layers' storage, which is final: every resize happened before its puts)
  if (hipSetDevice(device) != hipSuccess || hipMalloc(&M->dev_mem, img.size()) != hipSuccess ||
      hipMemcpy(M->dev_mem, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess)
    return set_error(CFM_ERR_RUNTIME, std::string("attention decoder weights upload: ") + hipGetErrorString(hipGetLastError()));
  for (auto& f : fix) *f.second = static_cast<char*>(M->dev_mem) + f.first;
  *out = M.release();
  return CFM_OK;
}

}  // namespace cfm

using namespace cfm;

extern "C" {

cfm_status cfm_aed_create(const cfm_aed_config* cfg, const cfm_tensor_view* weights, int32_t n, int32_t device,
                          cfm_aed** out) {
  if (!cfg || !weights || !out || n <= 0) return set_error(CFM_ERR_VALUE, "null argument");
  const int d = cfg->d, H = cfg->H;
  if (d <= 0 || H <= 0 || d % H) return set_error(CFM_ERR_VALUE, "attention decoder: d must divide into the heads");
  const int dk = d / H;
  if (dk % 16 || dk > 128) return set_error(CFM_ERR_VALUE, "attention decoder: head dim a multiple of 16 up to 128");
  if (d % 64 || cfg->ff <= 0 || cfg->ff % 64) return set_error(CFM_ERR_VALUE, "attention decoder: d and ff multiples of 64");
  if (cfg->V < 2 || cfg->sos < 0 || cfg->sos >= cfg->V || cfg->eos < 0 || cfg->eos >= cfg->V)
    return set_error(CFM_ERR_VALUE, "attention decoder: sos / eos outside the vocabulary");
  if (cfg->num_blocks < 0 || cfg->r_num_blocks < 0) return set_error(CFM_ERR_VALUE, "attention decoder: bad block counts");
  std::map<std::string, std::pair<const float*, int64_t>> hw;
  for (int i = 0; i < n; ++i)
    if (weights[i].name && weights[i].data) hw[weights[i].name] = {weights[i].data, weights[i].numel};
  switch (cfg->dtype) {
    case CFM_DTYPE_F32: return aed_build<float>(*cfg, hw, device, out);
    case CFM_DTYPE_BF16: return aed_build<bf16>(*cfg, hw, device, out);
    case CFM_DTYPE_F16: return aed_build<f16>(*cfg, hw, device, out);
  }
  return set_error(CFM_ERR_VALUE, "attention decoder: unknown dtype");
}

void cfm_aed_destroy(cfm_aed* h) { delete h; }

size_t cfm_aed_workspace_bytes(const cfm_aed* h, int32_t tokens, int32_t mem_rows) {
  return (h && tokens >= 0 && mem_rows >= 0) ? h->ws_bytes(tokens, mem_rows) : 0;
}

cfm_status cfm_aed_score(const cfm_aed* h, const float* mem, int32_t mem_rows, const int32_t* utt_start,
                         const int32_t* utt_len, int32_t B, const int32_t* tokens, int32_t n_tok, const int32_t* hyp_start,
                         const int32_t* hyp_len, const int32_t* hyp_utt, int32_t n_hyps, int32_t dirs, float* out_l2r,
                         float* out_r2l, void* ws, size_t wsb, cfm_stream stream) {
  if (!h) return set_error(CFM_ERR_VALUE, "null handle");
  if (mem_rows < 0 || B < 0 || n_tok < 0 || n_hyps < 0 || n_hyps > n_tok)
    return set_error(CFM_ERR_VALUE, "attention decoder: bad mem_rows / B / tokens / n_hyps");
  if (dirs < 1 || dirs > 3) return set_error(CFM_ERR_VALUE, "attention decoder: direction_mask is 1 (left to right), 2 or 3");
  if ((dirs & 2) && !h->dec[1].present) return set_error(CFM_ERR_ASSERT, "attention decoder: the model has no right decoder");
  if (!ws) return set_error(CFM_ERR_VALUE, "null argument");
  if (hipSetDevice(h->device) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipSetDevice");
  if (n_hyps == 0) {   // nothing to score: the status word still reads 0
    if (wsb < 4) return set_error(CFM_ERR_VALUE, "attention decoder workspace too small");
    if (hipMemsetAsync(ws, 0, 4, (hipStream_t)stream) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
    return CFM_OK;
  }
  if ((mem_rows > 0 && !mem) || !utt_start || !utt_len || !tokens || !hyp_start || !hyp_len || !hyp_utt ||
      ((dirs & 1) && !out_l2r) || ((dirs & 2) && !out_r2l))
    return set_error(CFM_ERR_VALUE, "null argument");
  if ((reinterpret_cast<uintptr_t>(mem) | reinterpret_cast<uintptr_t>(ws)) & 15)
    return set_error(CFM_ERR_VALUE, "memory rows / workspace must be 16-byte aligned");
  return h->score(mem, mem_rows, utt_start, utt_len, B, tokens, n_tok, hyp_start, hyp_len, hyp_utt, n_hyps, dirs, out_l2r,
                  out_r2l, ws, wsb, (hipStream_t)stream);
}

cfm_status cfm_op_seg_attention(int32_t dtype, int32_t kernel, const void* q, int32_t q_rows, const void* kv,
                                int32_t k_rows, const int32_t* desc, int32_t n_seg, int32_t H, int32_t dk, void* out,
                                int32_t* scratch, cfm_stream stream) {
  static const char* const KNAME[] = {"generic", "mfma"};
  if (!q || !kv || !desc || !out || !scratch) return set_error(CFM_ERR_VALUE, "segment attention: null argument");
  if (kernel != CFM_SEG_ATTN_GENERIC && kernel != CFM_SEG_ATTN_MFMA)
    return set_error(CFM_ERR_VALUE, "segment attention: unknown kernel");
  if (dtype != CFM_DTYPE_F32 && dtype != CFM_DTYPE_BF16 && dtype != CFM_DTYPE_F16)
    return set_error(CFM_ERR_VALUE, "segment attention: unknown dtype");
  if (H <= 0 || dk <= 0 || q_rows <= 0 || k_rows <= 0 || n_seg <= 0)
    return set_error(CFM_ERR_VALUE, "segment attention: bad H / dk / q_rows / k_rows / n_seg");
  hipStream_t st = (hipStream_t)stream;
  const int d = H * dk;
  // the eligibility of the selected kernel first: nothing is launched for a shape it does not take
  const bool takes = kernel == CFM_SEG_ATTN_GENERIC ? (dk % 16 == 0 && dk <= 128)
                                                    : (dtype != CFM_DTYPE_F32 && (dk == 64 || dk == 128));
  if (!takes)
    return set_error(CFM_ERR_ASSERT, std::string("segment attention: the ") + KNAME[kernel] +
                                         " kernel does not take this configuration");
  int32_t* status = scratch;
  int32_t* tile_off = scratch + 1;
  if (hipMemsetAsync(status, 0, 4, st) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
  KCHK(seg_scan(desc, n_seg, q_rows, k_rows, kernel == CFM_SEG_ATTN_MFMA ? SEG_MFMA_TQ : 16, tile_off, status, st));
  int r = -1;
#define SEG_CALL(FN, T_)                                                                                            \
  r = FN<T_>((const T_*)q, d, (const T_*)kv, (const T_*)kv + d, 2 * d, (T_*)out, d, desc, tile_off, n_seg, q_rows, \
             k_rows, H, dk, st)
  if (kernel == CFM_SEG_ATTN_GENERIC) {
    if (dtype == CFM_DTYPE_F32) SEG_CALL(seg_attention_generic, float);
    else if (dtype == CFM_DTYPE_F16) SEG_CALL(seg_attention_generic, f16);
    else SEG_CALL(seg_attention_generic, bf16);
  } else {
    if (dtype == CFM_DTYPE_F16) SEG_CALL(seg_attention_mfma, f16);
    else SEG_CALL(seg_attention_mfma, bf16);
  }
#undef SEG_CALL
  if (r == -1)
    return set_error(CFM_ERR_ASSERT, std::string("segment attention: the ") + KNAME[kernel] +
                                         " kernel does not take this configuration");
  if (r) return set_error(CFM_ERR_RUNTIME, std::string("segment attention (") + KNAME[kernel] + "): " +
                                               hipGetErrorString((hipError_t)r));
  return CFM_OK;
}

}  // extern "C"
