// RNN-T greedy search (the encoder's transducer consumer), gfx950.
//
// Replaces transducer/search/greedy_search.py:6-92 (optimized_search / batch_greedy_search) as the
// reference calls it from endless_decode / batch_decode (chunkformer_model.py:439-448, 533-543),
// with the shipped predictor / joint (RNNPredictor lstm, predictor.py:66-208; TransducerJoint
// prejoin + add + tanh + ffn_out, joint.py:74-111).  Blank id 0.
//
//   1. enc_proj = enc . enc_ffn^T + b for every frame: one f32 MFMA GEMM (gemm<float>);
//   2. rnnt_greedy_kernel: ONE persistent workgroup per utterance runs the whole search, with the
//      utterance's state (last token, LSTM h / c, predictor output) in LDS:
//        - the predictor (embedding -> LSTM layers -> projection -> pred_ffn) is evaluated once per
//          emitted token: optimized_search recomputes predictor.forward_step at every step, but its
//          input (last non-blank token, committed LSTM state) only changes on an emission;
//        - the joint (tanh(enc_proj[t] + pred) . ffn_out^T + b, argmax) is evaluated for a block of
//          RF consecutive frames at once, reading ffn_out once per block; the frames before the
//          block's first non-blank decision are blank under the same predictor state, exactly as
//          the sequential loop decides them, and the search resumes at that frame.
//      Every loop iteration either advances the frame or counts an emission against the frame's
//      n_steps budget, so the kernel ends after at most T * (n_steps + 1) iterations.
//   A stateless handle (embedding / conv predictor, cfm_rnnt_create_ex) runs the same kernel with the predictor
//   replaced by sl_predictor: the state is the window of the last K token ids, the predictor a gather of K
//   embedding rows, their mix, (embedding) one E x E product, LayerNorm, the activation and the E x J pred_ffn.
//   Matrix-vector products read transposed f32 weights [K][M] with one float4 of outputs per
//   thread (coalesced rows, the input vector broadcast from LDS); argmax ties go to the lower id
//   like torch.argmax.  Everything is f32 (log_softmax is monotone: argmax of the logits).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cfm.h"
#include "cfm_common.h"
#include "cfm_kernels.h"
#include "rnnt.h"
#include "status.h"

namespace cfm {

constexpr int RNNT_NT = 512;   // threads per workgroup (8 waves)
constexpr int RNNT_RF = 8;     // frames per joint block
// y[0:M) = WT^T x + bias (WT [K][M] row-major, M % 4 == 0); x, y, red in LDS.  Outputs are split
// into float4 groups; when there are fewer groups than threads the K range is split too and the
// partial sums reduced through `red` ([ks][M] floats).
CFM_DEV void matvec(const float* __restrict__ WT, int K, int M, const float* x, const float* __restrict__ bias,
                    float* y, float* red, int tid) {
  const int groups = M >> 2;
  int ks = RNNT_NT / groups;
  ks = ks < 1 ? 1 : (ks > 8 ? 8 : ks);
  const int kc = (K + ks - 1) / ks;
  const float4* W4 = reinterpret_cast<const float4*>(WT);
  for (int w = tid; w < groups * ks; w += RNNT_NT) {
    const int g = w % groups, s = w / groups;
    const int k0 = s * kc, k1 = min(K, k0 + kc);
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    const float4* col = W4 + g;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) {
      const float4 wv = col[(size_t)k * groups];
      const float xv = x[k];
      acc.x = fmaf(wv.x, xv, acc.x);
      acc.y = fmaf(wv.y, xv, acc.y);
      acc.z = fmaf(wv.z, xv, acc.z);
      acc.w = fmaf(wv.w, xv, acc.w);
    }
    if (ks == 1) {
      const float4 b = reinterpret_cast<const float4*>(bias)[g];
      reinterpret_cast<float4*>(y)[g] = make_float4(acc.x + b.x, acc.y + b.y, acc.z + b.z, acc.w + b.w);
    } else {
      reinterpret_cast<float4*>(red + (size_t)s * M)[g] = acc;
    }
  }
  if (ks > 1) {
    __syncthreads();
    for (int m = tid; m < M; m += RNNT_NT) {
      float v = 0.f;
      for (int s = 0; s < ks; ++s) v += red[(size_t)s * M + m];
      y[m] = v + bias[m];
    }
  }
  __syncthreads();
}

CFM_DEV float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// the predictor for input token `tok` and committed state (h, c): new state (hn, cn) and
// pj = pred_ffn(projection(h_top)) (joint.py:87-88 pre-projection of the predictor output)
CFM_DEV void predictor(const RnntDev& w, int tok, const float* h, const float* c, float* hn, float* cn, float* xin,
                       float* gates, float* pvec, float* pj, float* red, int tid) {
  const int H = w.H;
  for (int e = tid; e < w.E; e += RNNT_NT) xin[e] = w.embed[(size_t)tok * w.E + e];
  int in = w.E;
  for (int l = 0; l < w.nl; ++l) {
    for (int e = tid; e < H; e += RNNT_NT) xin[in + e] = h[l * H + e];
    __syncthreads();
    matvec(w.wg[l], in + H, 4 * H, xin, w.bg[l], gates, red, tid);
    for (int e = tid; e < H; e += RNNT_NT) {   // torch LSTM gate order i, f, g, o
      const float ig = sigm(gates[e]), fg = sigm(gates[H + e]), gg = tanhf(gates[2 * H + e]),
                  og = sigm(gates[3 * H + e]);
      const float cv = fg * c[l * H + e] + ig * gg;
      cn[l * H + e] = cv;
      const float hv = og * tanhf(cv);
      hn[l * H + e] = hv;
      xin[e] = hv;   // the next layer's input
    }
    __syncthreads();
    in = H;
  }
  matvec(w.wp, H, w.J, xin, w.bp, pj, red, tid);   // composed projection + pred_ffn (cfm_rnnt_create)
}

// The stateless predictors (predictor.py:210-471) for the id window win[0 .. Kc) (oldest first, -1 = a position before
// the sos: a zero vector): the Kc embedding rows into LDS, the mix (embedding: Kc dot products with the summed
// pos_embed heads, the weighted sum of the rows and the E x E ffn; conv: the per-channel taps), LayerNorm, activation
// and pj = pred_ffn(y).  sc: 32 floats of reductions.
CFM_DEV void sl_predictor(const RnntDev& w, const int* win, float* rows, float* x, float* y, float* pj, float* red,
                          float* sc, int tid) {
  const int E = w.E, Kc = w.Kc, lane = tid & 63, wid = tid >> 6;
  for (int e = tid; e < Kc * E; e += RNNT_NT) {
    const int c = e / E, d = e - c * E, id = win[c];
    rows[e] = id >= 0 ? w.embed[(size_t)id * E + d] : 0.f;
  }
  __syncthreads();
  if (w.kind == CFM_RNNT_PRED_EMBEDDING) {
    for (int c = wid; c < Kc; c += RNNT_NT / 64) {
      float s = 0.f;
      for (int d = lane; d < E; d += 64) s = fmaf(rows[c * E + d], w.tap[c * E + d], s);
      s = wave_sum(s);
      if (lane == 0) sc[c] = s;
    }
    __syncthreads();
    for (int d = tid; d < E; d += RNNT_NT) {
      float a = 0.f;
      for (int c = 0; c < Kc; ++c) a = fmaf(sc[c], rows[c * E + d], a);
      x[d] = a / w.mix_div;
    }
    __syncthreads();
    matvec(w.wf, E, E, x, w.bf, y, red, tid);
  } else {
    for (int d = tid; d < E; d += RNNT_NT) {
      float a = 0.f;
      for (int c = 0; c < Kc; ++c) a = fmaf(w.tap[c * E + d], rows[c * E + d], a);
      y[d] = w.cbias ? a + w.cbias[d] : a;
    }
    __syncthreads();
  }
  // LayerNorm (two passes, as torch: mean, then the variance about it) and the activation
  float s = 0.f;
  for (int d = tid; d < E; d += RNNT_NT) s += y[d];
  s = wave_sum(s);
  if (lane == 0) sc[16 + wid] = s;
  __syncthreads();
  float mean = 0.f;
  for (int q = 0; q < RNNT_NT / 64; ++q) mean += sc[16 + q];
  mean /= (float)E;
  float v = 0.f;
  for (int d = tid; d < E; d += RNNT_NT) { const float dd = y[d] - mean; v = fmaf(dd, dd, v); }
  v = wave_sum(v);
  if (lane == 0) sc[24 + wid] = v;
  __syncthreads();
  float var = 0.f;
  for (int q = 0; q < RNNT_NT / 64; ++q) var += sc[24 + q];
  const float rstd = 1.f / sqrtf(var / (float)E + w.ln_eps);
  for (int d = tid; d < E; d += RNNT_NT) y[d] = rnnt_act(w.act, (y[d] - mean) * rstd * w.gamma[d] + w.beta[d]);
  __syncthreads();
  matvec(w.wp, E, w.J, y, w.bp, pj, red, tid);
}

// SL: a stateless handle.  The carried state is the id window instead of h / c; the joint block, the argmax and the
// commit logic are the same code.
template <bool SL>
__global__ __launch_bounds__(RNNT_NT) void rnnt_greedy_kernel(RnntDev w, const float* __restrict__ enc_proj,
                                                              const int32_t* __restrict__ row_start,
                                                              const int32_t* __restrict__ row_len, int n_steps,
                                                              int32_t* __restrict__ out) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int H = w.H, J = w.J, nl = w.nl;
  const int b = blockIdx.x;
  const int r0 = row_start[b], T = row_len[b];
  // LDS carve (floats)
  float* h = lds;                        // [nl][H] committed state
  float* c = h + nl * H;
  float* hn = c + nl * H;                // [nl][H] state after the last predictor evaluation
  float* cn = hn + nl * H;
  float* xin = cn + nl * H;              // [max(E, H) + H]
  float* gates = xin + (max(w.E, H) + H);   // [4H]
  float* pvec = gates + 4 * H;           // [P]
  float* pj = pvec + w.P;                // [J]
  // ... of a stateless handle: the window's rows, the mixed vector, the predictor output, reductions, the window
  float* rows = lds;                     // [Kc][E]
  float* sx = rows + w.Kc * w.E;         // [E]
  float* sy = sx + w.E;                  // [E]
  float* sc = sy + w.E;                  // [32]
  int* win = reinterpret_cast<int*>(sc + 32);   // [16]
  if constexpr (SL) pj = sc + 48;
  float* z = pj + J;                     // [RF][J] joint inputs of the block
  float* red = z + RNNT_RF * J;          // [4 * NT] split-K partials (ks * M <= 4 * NT)
  float* wbest = red + 4 * RNNT_NT;      // [8 waves][RF] best value
  int* wbidx = reinterpret_cast<int*>(wbest + 8 * RNNT_RF);  // [8][RF] its id
  int* ctl = wbidx + 8 * RNNT_RF;        // [RF] decisions of the block

  int tok = w.blank;
  if constexpr (SL) {
    if (tid < w.Kc) win[tid] = tid == w.Kc - 1 ? tok : -1;
    __syncthreads();
    sl_predictor(w, win, rows, sx, sy, pj, red, sc, tid);
  } else {
    for (int e = tid; e < nl * H; e += RNNT_NT) { h[e] = 0.f; c[e] = 0.f; }
    __syncthreads();
    predictor(w, tok, h, c, hn, cn, xin, gates, pvec, pj, red, tid);
  }

  int t = 0, step = 0;
  while (t < T) {
    const int nf = min(RNNT_RF, T - t);
    // joint inputs z[f] = tanh(enc_proj[t + f] + pj)
    for (int e = tid; e < nf * J; e += RNNT_NT) {
      const int f = e / J, j = e - f * J;
      z[e] = tanhf(enc_proj[(size_t)(r0 + t + f) * J + j] + pj[j]);
    }
    __syncthreads();
    // logits of the block: threads over float4 groups of the (padded) vocabulary, all frames
    float bv[RNNT_RF];
    int bi[RNNT_RF];
#pragma unroll
    for (int f = 0; f < RNNT_RF; ++f) { bv[f] = -INFINITY; bi[f] = 0x7fffffff; }
    const int vg = w.Vp >> 2;
    const float4* W4 = reinterpret_cast<const float4*>(w.wo);
    for (int g = tid; g < vg; g += RNNT_NT) {
      float4 acc[RNNT_RF];
#pragma unroll
      for (int f = 0; f < RNNT_RF; ++f) acc[f] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
      for (int j = 0; j < J; ++j) {
        const float4 wv = W4[(size_t)j * vg + g];
#pragma unroll
        for (int f = 0; f < RNNT_RF; ++f) {
          const float zv = z[f * J + j];
          acc[f].x = fmaf(wv.x, zv, acc[f].x);
          acc[f].y = fmaf(wv.y, zv, acc[f].y);
          acc[f].z = fmaf(wv.z, zv, acc[f].z);
          acc[f].w = fmaf(wv.w, zv, acc[f].w);
        }
      }
      const float4 bb = reinterpret_cast<const float4*>(w.bo)[g];
#pragma unroll
      for (int f = 0; f < RNNT_RF; ++f) {
        const float v4[4] = {acc[f].x + bb.x, acc[f].y + bb.y, acc[f].z + bb.z, acc[f].w + bb.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)   // ascending ids: strict > keeps the lowest id of a tie
          if (v4[q] > bv[f]) { bv[f] = v4[q]; bi[f] = 4 * g + q; }
      }
    }
    // argmax per frame: wave (value, lowest id), then across the 8 waves
#pragma unroll
    for (int f = 0; f < RNNT_RF; ++f) {
      float v = bv[f];
      int i = bi[f];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
      }
      if (lane == 0) { wbest[wid * RNNT_RF + f] = v; wbidx[wid * RNNT_RF + f] = i; }
    }
    __syncthreads();
    if (tid < RNNT_RF) {
      float v = wbest[tid];
      int i = wbidx[tid];
      for (int q = 1; q < RNNT_NT / 64; ++q) {
        const float ov = wbest[q * RNNT_RF + tid];
        const int oi = wbidx[q * RNNT_RF + tid];
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
      }
      ctl[tid] = i;
    }
    __syncthreads();
    int f = 0;
    while (f < nf && ctl[f] == w.blank) ++f;   // uniform: every thread reads the same LDS words
    __syncthreads();
    if (f == nf) {   // the whole block is blank under this predictor state
      t += nf;
      step = 0;
      continue;
    }
    if (f > 0) { t += f; step = 0; }
    const int k = ctl[f];
    if (tid == 0) out[(size_t)(r0 + t) * n_steps + step] = k;
    ++step;
    tok = (unsigned)k < (unsigned)w.V ? k : w.blank;   // NaN logits leave no valid id: never index past embed
    if constexpr (SL) {
      // commit the emission: the id window shifts by k
      const int nv = tid + 1 < w.Kc ? win[tid + 1] : tok;
      __syncthreads();
      if (tid < w.Kc) win[tid] = nv;
      __syncthreads();
      sl_predictor(w, win, rows, sx, sy, pj, red, sc, tid);
    } else {
      // commit the emission: the predictor's new state becomes the state, k the next input
      for (int e = tid; e < nl * H; e += RNNT_NT) { h[e] = hn[e]; c[e] = cn[e]; }
      __syncthreads();
      predictor(w, tok, h, c, hn, cn, xin, gates, pvec, pj, red, tid);
    }
    if (step == n_steps) { ++t; step = 0; }
  }
}

// ---- one long utterance over many CUs (B small: endless_decode's B = 1) ------------------------
//
// The single-workgroup search above streams every predictor / joint weight (≈19 MB for the vie recipe)
// through ONE CU per emission.  rnnt_grid_kernel runs G workgroups per utterance instead; each owns a
// fixed slice of every matrix-vector product's outputs (LSTM units with their four gates, projection
// and pred_ffn outputs, vocabulary columns), stored block-major so a workgroup's slice is one
// contiguous, coalesced stream.  The phases of an emission (nl LSTM layers, the composed projection +
// pred_ffn, the joint's candidates) are separated by grid barriers on per-utterance flag words; the shared vectors
// (h / c state slots, projection and pred_ffn outputs, per-workgroup argmax candidates) live in the
// workspace.  Every workgroup reduces the candidates in the same order, so all of them take the same
// decisions and leave the loop together.  A barrier that does not complete within ~2^21 polls sets
// the workspace's error word, after which every workgroup leaves at its next barrier.
constexpr int RG_NT = 256;     // threads per workgroup (4 waves)
constexpr int RG_MAXB = 32;    // utterances on the grid path (B * G <= CUs)
constexpr int RG_MAXG = 256;   // workgroups per utterance

// the contiguous range of M4 output groups owned by part p of G
CFM_DEV void rg_range(int M4, int G, int p, int& g0, int& n) {
  g0 = (int)((long long)M4 * p / G);
  n = (int)((long long)M4 * (p + 1) / G) - g0;
}

// Grid barrier over the G workgroups of one utterance: workgroup p publishes the barrier's epoch in
// its own flag word (no contended atomic: a counter serialised the G arrivals, ≈0.1 µs each), wave 0
// of every workgroup polls all G flags (one load per lane) until each holds the epoch.
// ATOM = false: release / acquire by agent-scope fences around the flag store / after the poll (an
// L2 write-back and invalidate on gfx950: the weight slices then come from the MALL every phase).
// ATOM = true: every access to the exchanged vectors is itself an agent-scope relaxed atomic (sc1:
// coherent across the XCDs' L2s), so the barrier only has to order completion: each wave waits for
// its stores (vmcnt(0)) before the workgroup barrier, the flag store follows, and the readers' loads
// issue after their poll returned -- no cache-wide fence, the weight slices stay in L2.
// Returns false on timeout (after ~2^21 polls the error word is set) or when another workgroup set it.
template <bool ATOM>
CFM_DEV bool rg_barrier(unsigned long long* flags, int G, int part, unsigned long long epoch, int* err, int* lflag) {
  if constexpr (ATOM) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    if (lane == 0) {
      if constexpr (!ATOM) __threadfence();   // release this workgroup's stores (agent scope)
      __hip_atomic_store(flags + part, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int ok = 1;
    unsigned spins = 0;
    for (;;) {
      bool ready = true;
      for (int q = lane; q < G; q += 64)
        ready &= __hip_atomic_load(flags + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= epoch;
      if (__builtin_amdgcn_ballot_w64(!ready) == 0) break;
      if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { ok = 0; break; }
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1u << 21)) {
        if (lane == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
    }
    if constexpr (!ATOM) __threadfence();   // acquire the other workgroups' stores
    if (lane == 0) *lflag = ok;
  }
  __syncthreads();
  return *lflag != 0;
}
#ifndef RG_UNROLL
#define RG_UNROLL 4    // weight loads in flight per thread in the predictor matvecs (16: 10-35% slower)
#endif
#ifndef RG_JUNROLL
#define RG_JUNROLL 2   // ... in the joint (8: slower)
#endif
// accesses to the vectors the workgroups exchange (see rg_barrier)
template <bool ATOM, class V>
CFM_DEV V sh_ld(const V* p) {
  if constexpr (ATOM) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <bool ATOM, class V>
CFM_DEV void sh_st(V* p, V v) {
  if constexpr (ATOM) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
// dst[0:n) (LDS) = src[0:n) (an exchanged vector, n <= 8 NT): every load issued before the first
// LDS store, so the copy costs one round trip
template <bool ATOM>
CFM_DEV void rg_fetch(float* dst, const float* src, int n) {
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = (int)threadIdx.x + i * RG_NT;
    v[i] = e < n ? sh_ld<ATOM>(src + e) : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = (int)threadIdx.x + i * RG_NT;
    if (e < n) dst[e] = v[i];
  }
}

// Partial sums of the ks = NT / np threads (s, jj), tid = s * np + jj, down to one per column: xor
// shuffles across the lanes of a wave that share jj (np < 64), then the 4 waves' (or, for np >= 64,
// the ks) partials through LDS, summed in a fixed order by thread jj.  rg_parts(np) = partials left.
CFM_DEV int rg_parts(int np) { return np < 64 ? RG_NT / 64 : RG_NT / np; }
CFM_DEV float4 rg_wave_reduce(float4 v, int np) {
  for (int o = np; o < 64; o <<= 1) {
    v.x += __shfl_xor(v.x, o, 64);
    v.y += __shfl_xor(v.y, o, 64);
    v.z += __shfl_xor(v.z, o, 64);
    v.w += __shfl_xor(v.w, o, 64);
  }
  return v;
}
// the LDS slot of this thread's reduced partial, or -1 when the thread holds none
CFM_DEV int rg_slot(int np) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (np >= 64) return tid;                             // slot q * np + jj with q = s
  return lane < np ? (tid >> 6) * np + lane : -1;       // q = wave, jj = lane
}

// sums[jj] = sum_k Wb[k][jj] * x[k] for jj < n (Wb: this workgroup's [K][n] float4 slice), threads
// (s, jj) = (tid / np, tid % np) with np = pow2 >= n: a wave reads whole consecutive rows of the
// slice; the ks = NT / np partial sums are added in order through `red`.  fin(jj, sum) runs on the
// thread jj < n.
template <class F>
CFM_DEV void rg_matvec(const float4* __restrict__ Wb, int K, int n, const float* x, float4* red, F&& fin) {
  const int tid = threadIdx.x;
  if (n <= 0) return;
  int np = 1;
  while (np < n) np <<= 1;
  const int ks = RG_NT / np, jj = tid % np, s = tid / np;
  float4 acc = {0.f, 0.f, 0.f, 0.f};
  if (jj < n) {
    // several loads in flight per thread: the loop is latency-bound, not bandwidth-bound
#pragma unroll RG_UNROLL
    for (int k = s; k < K; k += ks) {
      const float4 wv = Wb[(size_t)k * n + jj];
      const float xv = x[k];
      acc.x = fmaf(wv.x, xv, acc.x);
      acc.y = fmaf(wv.y, xv, acc.y);
      acc.z = fmaf(wv.z, xv, acc.z);
      acc.w = fmaf(wv.w, xv, acc.w);
    }
  }
  acc = rg_wave_reduce(acc, np);
  const int slot = rg_slot(np);
  if (slot >= 0) red[slot] = acc;
  __syncthreads();
  if (tid < n) {
    float4 v = red[tid];
    const int parts = rg_parts(np);
    for (int q = 1; q < parts; ++q) {
      const float4 o = red[tid + q * np];
      v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    fin(tid, v);
  }
  __syncthreads();
}

__host__ __device__ size_t rnnt_grid_lds_bytes(const RnntDev& w);

// LDSW: the workgroup's weight slices are copied into LDS once (after the work area of
// rnnt_grid_lds_bytes) and every emission's matrix-vector products read them there, not from the
// MALL / HBM after each barrier's acquire
template <bool LDSW, bool ATOM>
__global__ __launch_bounds__(RG_NT) void rnnt_grid_kernel(RnntDev w, RnntGrid gw, float* __restrict__ scratch,
                                                          int per_utt, unsigned long long* __restrict__ bars,
                                                          int* __restrict__ err, const float* __restrict__ enc_proj,
                                                          const int32_t* __restrict__ row_start,
                                                          const int32_t* __restrict__ row_len, int n_steps,
                                                          int32_t* __restrict__ out) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  // an error word set before the launch (option grid_force_error, tests of the caller's fallback): every
  // workgroup leaves before its first barrier
  if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  const int G = gw.G, utt = blockIdx.x / G, part = blockIdx.x - utt * G;
  const int H = w.H, J = w.J, P = w.P, E = w.E, nl = w.nl;
  const int r0 = row_start[utt], T = row_len[utt];
  // workspace of the utterance: state slots, projection / pred_ffn outputs, candidates (2 parities)
  float* hs = scratch + (size_t)utt * per_utt;   // [2][nl][H]
  float* cs = hs + 2 * nl * H;                   // [2][nl][H]
  float* pvec = cs + 2 * nl * H;                 // [P]
  float* pj = pvec + P;                          // [J]
  float* candv = pj + J;                         // [2][G][RF]
  int* candi = reinterpret_cast<int*>(candv + 2 * G * RNNT_RF);   // [2][G][RF]
  unsigned long long* flags = bars + (size_t)utt * RG_MAXG;   // [G] barrier epochs, one word per workgroup
  // LDS: x vector, z block, partial sums, pred_ffn output, decisions
  float* x = lds;                                // [max(E, H) + H]
  float* z = x + (max(E, H) + H);                // [RF][J]
  float* lpj = z + RNNT_RF * J;                  // [J]
  float4* red = reinterpret_cast<float4*>(lpj + J + ((4 - ((max(E, H) + H + RNNT_RF * J + J) & 3)) & 3));  // [NT * RF]
  int* dec = reinterpret_cast<int*>(red + RG_NT * RNNT_RF);   // [RF]
  int* lflag = dec + RNNT_RF;
  unsigned long long epoch = 0;
  auto sync = [&]() { return rg_barrier<ATOM>(flags, G, part, ++epoch, err, lflag); };

  // this workgroup's output ranges and weight slices
  int u0, nu, pg0, pn, v0, nv;
  rg_range(H, G, part, u0, nu);
  rg_range(P >> 2, G, part, pg0, pn);   // (P = J: the composed projection + pred_ffn)
  rg_range(w.Vp >> 2, G, part, v0, nv);
  const float4* sl_wp = gw.wp + (size_t)H * pg0;
  const float4* sl_wo = gw.wo + (size_t)J * v0;
  float4* wcache = reinterpret_cast<float4*>(lds + rnnt_grid_lds_bytes(w) / 4);   // [layers][wp][wo]
  if constexpr (LDSW) {
    float4* c = wcache;
    auto copy = [&](const float4* src, size_t n4) {
      for (size_t i = tid; i < n4; i += RG_NT) c[i] = src[i];
      c += n4;
    };
    int in = E;
    for (int l = 0; l < nl; ++l) {
      copy(gw.wg[l] + (size_t)(in + H) * u0, (size_t)(in + H) * nu);
      in = H;
    }
    copy(sl_wp, (size_t)H * pn);
    sl_wp = c - (size_t)H * pn;
    copy(sl_wo, (size_t)J * nv);
    sl_wo = c - (size_t)J * nv;
    __syncthreads();
  }

  int cur = 0;   // committed state slot (zero-initialised by the host)
  // the predictor for token `tok` from slot cur into slot cur ^ 1; pj -> lpj
  auto predictor = [&](int tok) -> bool {
    int in = E;
    const float4* wl = wcache;   // LDSW: layer l's slice follows layer l - 1's
    for (int l = 0; l < nl; ++l) {
      if (l == 0) {
        for (int e = tid; e < in; e += RG_NT) x[e] = w.embed[(size_t)tok * E + e];
      } else {
        rg_fetch<ATOM>(x, hs + ((size_t)(cur ^ 1) * nl + (l - 1)) * H, in);
      }
      rg_fetch<ATOM>(x + in, hs + ((size_t)cur * nl + l) * H, H);
      __syncthreads();
      float* cold = cs + ((size_t)cur * nl + l) * H;
      float* cnew = cs + ((size_t)(cur ^ 1) * nl + l) * H;
      float* hnew = hs + ((size_t)(cur ^ 1) * nl + l) * H;
      const float4* bq = gw.bg[l];
      if constexpr (!LDSW) wl = gw.wg[l] + (size_t)(in + H) * u0;
      rg_matvec(wl, in + H, nu, x, red, [&](int jj, float4 a) {
        const int u = u0 + jj;
        const float4 b = bq[u];
        const float ig = sigm(a.x + b.x), fg = sigm(a.y + b.y), gg = tanhf(a.z + b.z), og = sigm(a.w + b.w);
        const float cv = fg * cold[u] + ig * gg;
        cnew[u] = cv;   // (read back only by this workgroup)
        sh_st<ATOM>(hnew + u, og * tanhf(cv));
      });
      if (!sync()) return false;
      wl += (size_t)(in + H) * nu;
      in = H;
    }
    {
      const float* ht = hs + ((size_t)(cur ^ 1) * nl + (nl - 1)) * H;
      rg_fetch<ATOM>(x, ht, H);
      __syncthreads();
      const int g0 = pg0, n = pn;
      const float4* b4 = reinterpret_cast<const float4*>(w.bp);
      rg_matvec(sl_wp, H, n, x, red, [&](int jj, float4 a) {   // composed projection + pred_ffn
        const float4 b = b4[g0 + jj];
        float* o = pj + 4 * (g0 + jj);
        sh_st<ATOM>(o, a.x + b.x); sh_st<ATOM>(o + 1, a.y + b.y); sh_st<ATOM>(o + 2, a.z + b.z); sh_st<ATOM>(o + 3, a.w + b.w);
      });
      if (!sync()) return false;
    }
    rg_fetch<ATOM>(lpj, pj, J);
    __syncthreads();
    return true;
  };

  if (!predictor(w.blank)) return;
  int np = 1;
  while (np < nv) np <<= 1;
  const int ks = RG_NT / np, jj = tid % np, sp = tid / np;
  const float4* wo = sl_wo;
  const float4* bo4 = reinterpret_cast<const float4*>(w.bo);
  int t = 0, step = 0;
  while (t < T) {
    const int nf = min(RNNT_RF, T - t);
    for (int e = tid; e < RNNT_RF * J; e += RG_NT) {
      const int f = e / J, j = e - f * J;
      z[e] = f < nf ? tanhf(enc_proj[(size_t)(r0 + t + f) * J + j] + lpj[j]) : 0.f;
    }
    __syncthreads();
    // this workgroup's vocabulary columns for all RF frames
    float4 acc[RNNT_RF];
#pragma unroll
    for (int f = 0; f < RNNT_RF; ++f) acc[f] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (jj < nv) {
#pragma unroll RG_JUNROLL
      for (int k = sp; k < J; k += ks) {
        const float4 wv = wo[(size_t)k * nv + jj];
#pragma unroll
        for (int f = 0; f < RNNT_RF; ++f) {
          const float zv = z[f * J + k];
          acc[f].x = fmaf(wv.x, zv, acc[f].x);
          acc[f].y = fmaf(wv.y, zv, acc[f].y);
          acc[f].z = fmaf(wv.z, zv, acc[f].z);
          acc[f].w = fmaf(wv.w, zv, acc[f].w);
        }
      }
    }
    {
      const int slot = rg_slot(np);
#pragma unroll
      for (int f = 0; f < RNNT_RF; ++f) {
        const float4 v = rg_wave_reduce(acc[f], np);
        if (slot >= 0) red[f * RG_NT + slot] = v;
      }
    }
    __syncthreads();
    // (frame, column group) sums in order, then each frame's best over this workgroup's columns
    float* sv = z;   // z is consumed: reuse as [RF][np] best values / ids
    int* si = reinterpret_cast<int*>(z + RNNT_RF * 64);
    for (int e = tid; e < RNNT_RF * nv; e += RG_NT) {
      const int f = e / nv, c = e - f * nv;
      float4 v = red[f * RG_NT + c];
      const int parts = rg_parts(np);
      for (int q = 1; q < parts; ++q) {
        const float4 o = red[f * RG_NT + c + q * np];
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      }
      const float4 b = bo4[v0 + c];
      const float v4[4] = {v.x + b.x, v.y + b.y, v.z + b.z, v.w + b.w};
      float bv = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (v4[q] > bv) { bv = v4[q]; bi = 4 * (v0 + c) + q; }
      sv[f * 64 + c] = bv;
      si[f * 64 + c] = bi;
    }
    __syncthreads();
    const int par = (int)(epoch & 1);
    if (tid < RNNT_RF) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int c = 0; c < nv; ++c)   // ascending ids: strict > keeps the lowest id of a tie
        if (sv[tid * 64 + c] > bv) { bv = sv[tid * 64 + c]; bi = si[tid * 64 + c]; }
      sh_st<ATOM>(candv + ((size_t)par * G + part) * RNNT_RF + tid, bv);
      sh_st<ATOM>(candi + ((size_t)par * G + part) * RNNT_RF + tid, bi);
    }
    if (!sync()) return;
    if (tid < RNNT_RF) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int q = 0; q < G; ++q) {   // parts in ascending vocabulary order
        const float v = sh_ld<ATOM>(candv + ((size_t)par * G + q) * RNNT_RF + tid);
        if (v > bv) { bv = v; bi = sh_ld<ATOM>(candi + ((size_t)par * G + q) * RNNT_RF + tid); }
      }
      dec[tid] = bi;
    }
    __syncthreads();
    int f = 0;
    while (f < nf && dec[f] == w.blank) ++f;
    if (f == nf) {
      t += nf;
      step = 0;
      __syncthreads();
      continue;
    }
    if (f > 0) { t += f; step = 0; }
    const int k = dec[f];
    __syncthreads();
    if (part == 0 && tid == 0) out[(size_t)(r0 + t) * n_steps + step] = k;
    ++step;
    cur ^= 1;   // commit: the evaluated state becomes the state, k the next input
    if (!predictor((unsigned)k < (unsigned)w.V ? k : w.blank)) return;   // (NaN logits: no valid id)
    if (step == n_steps) { ++t; step = 0; }
  }
}

__host__ __device__ size_t rnnt_grid_lds_bytes(const RnntDev& w) {
  const size_t fl = (size_t)((w.E > w.H ? w.E : w.H) + w.H) + RNNT_RF * w.J + w.J;
  return (fl + 3) / 4 * 16 + (size_t)RG_NT * RNNT_RF * 16 + 2 * RNNT_RF * 4 + 16;
}

size_t rnnt_lds_bytes(const RnntDev& w) {
  const size_t H = w.H, J = w.J, P = w.P;
  if (w.kind != CFM_RNNT_PRED_RNN) {   // the stateless carve: rows, x, y, reductions + window, pj, then as below
    const size_t f = (size_t)w.Kc * w.E + 2 * (size_t)w.E + 48 + J + RNNT_RF * J + 4 * RNNT_NT + 8 * RNNT_RF;
    return f * 4 + 8 * RNNT_RF * 4 + RNNT_RF * 4;
  }
  size_t f = 4 * w.nl * H + (std::max<size_t>(w.E, H) + H) + 4 * H + P + J + RNNT_RF * J + 4 * RNNT_NT +
             8 * RNNT_RF;
  return f * 4 + 8 * RNNT_RF * 4 + RNNT_RF * 4;
}

}  // namespace cfm

using namespace cfm;

namespace {

struct Img {
  std::vector<char> bytes;
  std::vector<std::pair<size_t, const float**>> fix;
  void put(const std::vector<float>& v, const float** slot) {
    size_t off = (bytes.size() + 255) / 256 * 256;
    bytes.resize(off + (v.size() * 4 + 255) / 256 * 256);
    std::memcpy(bytes.data() + off, v.data(), v.size() * 4);
    fix.push_back({off, slot});
  }
};

// block-major slices of the grid path for h->grid_blocks workgroups (the ranges of rg_range)
int rnnt_grid_build(cfm_rnnt* h) {
  if (h->grid_mem) { (void)hipFree(h->grid_mem); h->grid_mem = nullptr; }
  const int G = h->w.kind != CFM_RNNT_PRED_RNN ? 0 : h->grid_blocks;
  h->gw = RnntGrid{};
  h->gw.G = G;
  if (G <= 0) return 0;
  const RnntDev& w = h->w;
  const int H = w.H;
  std::vector<float> img;
  std::vector<std::pair<size_t, const float4**>> fix;
  auto put = [&](const std::vector<float>& v, const float4** slot) {
    const size_t off = (img.size() + 63) / 64 * 64;
    img.resize(off + v.size());
    std::copy(v.begin(), v.end(), img.begin() + off);
    fix.push_back({off, slot});
  };
  auto range = [&](int M4, int p, int& g0, int& n) {
    g0 = (int)((long long)M4 * p / G);
    n = (int)((long long)M4 * (p + 1) / G) - g0;
  };
  // quad(k, g) -> 4 floats; slices [part][k][n]
  auto slices = [&](int K, int M4, auto quad) {
    std::vector<float> o((size_t)K * M4 * 4);
    size_t at = 0;
    for (int p = 0; p < G; ++p) {
      int g0, n;
      range(M4, p, g0, n);
      for (int k = 0; k < K; ++k)
        for (int j = 0; j < n; ++j) {
          quad(k, g0 + j, &o[at]);
          at += 4;
        }
    }
    return o;
  };
  for (int l = 0; l < w.nl; ++l) {
    const std::vector<float>& a = h->host_wg[l];
    const int K = (int)(a.size() / (4 * (size_t)H));
    put(slices(K, H, [&](int k, int u, float* q) {
          for (int gi = 0; gi < 4; ++gi) q[gi] = a[(size_t)k * 4 * H + gi * H + u];
        }), &h->gw.wg[l]);
    std::vector<float> bq(4 * (size_t)H);
    for (int u = 0; u < H; ++u)
      for (int gi = 0; gi < 4; ++gi) bq[4 * u + gi] = h->host_bg[l][gi * H + u];
    put(bq, &h->gw.bg[l]);
  }
  auto cols = [&](const std::vector<float>& m, int K, int M) {
    return slices(K, M / 4, [&](int k, int g, float* q) {
      for (int i = 0; i < 4; ++i) q[i] = m[(size_t)k * M + 4 * g + i];
    });
  };
  put(cols(h->host_wp, H, w.P), &h->gw.wp);
  put(cols(h->host_wo, w.J, w.Vp), &h->gw.wo);
  if (hipSetDevice(h->device) != hipSuccess || hipMalloc(&h->grid_mem, img.size() * 4) != hipSuccess ||
      hipMemcpy(h->grid_mem, img.data(), img.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    set_error(CFM_ERR_RUNTIME, std::string("rnnt grid weights upload: ") + hipGetErrorString(hipGetLastError()));
    return 1;
  }
  for (auto& f : fix) *f.second = reinterpret_cast<const float4*>((float*)h->grid_mem + f.first);
  return 0;
}

// floats of one utterance's grid workspace
size_t rnnt_grid_per_utt(const cfm_rnnt* h) {
  const RnntDev& w = h->w;
  const size_t G = std::max(h->grid_blocks, 1);
  return ((size_t)4 * w.nl * w.H + w.P + w.J + 4 * G * RNNT_RF + 63) / 64 * 64;
}

}  // namespace

extern "C" {

cfm_status cfm_rnnt_create(const cfm_rnnt_config* cfg, const cfm_tensor_view* weights, int32_t n, int32_t device,
                           cfm_rnnt** out) {
  return cfm_rnnt_create_ex(cfg, nullptr, weights, n, device, out);
}

cfm_status cfm_rnnt_create_ex(const cfm_rnnt_config* cfg, const cfm_rnnt_predictor_config* pcfg,
                              const cfm_tensor_view* weights, int32_t n, int32_t device, cfm_rnnt** out) {
  if (!cfg || !out || (!weights && n > 0)) return set_error(CFM_ERR_VALUE, "null argument");
  *out = nullptr;
  const int kind = pcfg ? pcfg->kind : CFM_RNNT_PRED_RNN;
  if (kind != CFM_RNNT_PRED_RNN && kind != CFM_RNNT_PRED_EMBEDDING && kind != CFM_RNNT_PRED_CONV)
    return set_error(CFM_ERR_VALUE, "predictor kind: rnn, embedding or conv");
  const bool sl = kind != CFM_RNNT_PRED_RNN;
  const int V = cfg->vocab, E = cfg->embed_size, H = sl ? 0 : cfg->hidden, nl = sl ? 0 : cfg->num_layers,
            P = cfg->pred_out, J = cfg->join_dim, Ee = cfg->enc_dim;
  if (V < 2 || (!sl && (nl < 1 || nl > RNNT_MAXL))) return set_error(CFM_ERR_ASSERT, "vocab >= 2 and 1 <= num_layers <= 4");
  for (int v : {E, sl ? E : H, P, J, Ee})
    if (v <= 0 || v % 4 || v > 1024) return set_error(CFM_ERR_ASSERT, "predictor / joint widths: multiples of 4, <= 1024");
  if (sl) {
    if (E != P) return set_error(CFM_ERR_ASSERT, "stateless predictors need embed_size == output_size");
    if (pcfg->history_size < 0 || pcfg->history_size > 8) return set_error(CFM_ERR_ASSERT, "history_size: 0 .. 8");
    if (kind == CFM_RNNT_PRED_EMBEDDING && pcfg->n_head < 1) return set_error(CFM_ERR_ASSERT, "n_head >= 1");
    if (pcfg->activation < CFM_RNNT_ACT_RELU || pcfg->activation > CFM_RNNT_ACT_GELU)
      return set_error(CFM_ERR_ASSERT, "predictor activation: relu, swish, tanh or gelu");
    if (!(pcfg->ln_eps > 0.f)) return set_error(CFM_ERR_ASSERT, "layer_norm_epsilon must be > 0");
  }
  if (Ee % 32) return set_error(CFM_ERR_ASSERT, "enc_output_size must be a multiple of 32");
  if (cfg->blank < 0 || cfg->blank >= V) return set_error(CFM_ERR_VALUE, "blank id out of range");
  std::map<std::string, std::pair<const float*, int64_t>> m;
  for (int i = 0; i < n; ++i) m[weights[i].name] = {weights[i].data, weights[i].numel};
  auto get = [&](const std::string& k, int64_t numel) -> const float* {
    auto it = m.find(k);
    if (it == m.end()) throw std::string("missing weight " + k);
    if (it->second.second != numel) throw std::string("weight " + k + ": wrong numel");
    return it->second.first;
  };
  auto transpose = [](const float* s, int rows, int cols, int cols_pad) {   // [rows][cols] -> [cols][pad rows]
    std::vector<float> t((size_t)cols * cols_pad, 0.f);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) t[(size_t)c * cols_pad + r] = s[(size_t)r * cols + c];
    return t;
  };
  auto h = std::make_unique<cfm_rnnt>();
  h->cfg = *cfg;
  if (sl) h->cfg.hidden = h->cfg.num_layers = 0;   // ignored for a stateless handle: no later reader sees the caller's
  h->device = device;
  Img img;
  RnntDev& w = h->w;
  w.V = V; w.Vp = (V + 3) / 4 * 4; w.E = E; w.H = H; w.nl = nl; w.P = P; w.J = J; w.blank = cfg->blank;
  try {
    const float* emb = get("predictor.embed.weight", (int64_t)V * E);
    img.put(std::vector<float>(emb, emb + (size_t)V * E), &w.embed);
    w.kind = kind;
    if (sl) {
      const int Kc = pcfg->history_size + 1;
      w.Kc = Kc; w.act = pcfg->activation; w.ln_eps = pcfg->ln_eps;
      std::vector<float> tap((size_t)Kc * E);
      if (kind == CFM_RNNT_PRED_EMBEDDING) {
        // the heads of pos_embed only ever appear summed: q_c[d] = sum_head weight[head, d * Kc + c], once here
        const int nh = pcfg->n_head;
        const float* pos = get("predictor.pos_embed.weight", (int64_t)nh * E * Kc);
        for (int c = 0; c < Kc; ++c)
          for (int d = 0; d < E; ++d) {
            double a = 0.0;
            for (int q = 0; q < nh; ++q) a += pos[((size_t)q * E + d) * Kc + c];
            tap[(size_t)c * E + d] = (float)a;
          }
        w.mix_div = (float)(nh * Kc);
        h->host_wf = transpose(get("predictor.ffn.weight", (int64_t)E * E), E, E, E);
        img.put(h->host_wf, &w.wf);
        const float* bf = get("predictor.ffn.bias", E);
        img.put(std::vector<float>(bf, bf + E), &w.bf);
      } else {
        const float* cw = get("predictor.conv.weight", (int64_t)E * Kc);
        for (int c = 0; c < Kc; ++c)
          for (int d = 0; d < E; ++d) tap[(size_t)c * E + d] = cw[(size_t)d * Kc + c];
        if (pcfg->conv_bias) {
          const float* cb = get("predictor.conv.bias", E);
          img.put(std::vector<float>(cb, cb + E), &w.cbias);
        }
      }
      img.put(tap, &w.tap);
      const float* ga = get("predictor.norm.weight", E);
      const float* be2 = get("predictor.norm.bias", E);
      img.put(std::vector<float>(ga, ga + E), &w.gamma);
      img.put(std::vector<float>(be2, be2 + E), &w.beta);
      // a non-linearity stands between the predictor and the joint's pred_ffn: it stays a separate [J, E] product
      const float* wpjm = get("joint.pred_ffn.weight", (int64_t)J * E);
      const float* bpj = get("joint.pred_ffn.bias", J);
      h->host_wp = transpose(wpjm, J, E, J);   // [E][J]
      img.put(h->host_wp, &w.wp);
      img.put(std::vector<float>(bpj, bpj + J), &w.bp);
    }
    for (int l = 0; l < nl; ++l) {
      const int in = l == 0 ? E : H;
      const std::string s = std::to_string(l);
      const float* wih = get("predictor.rnn.weight_ih_l" + s, (int64_t)4 * H * in);
      const float* whh = get("predictor.rnn.weight_hh_l" + s, (int64_t)4 * H * H);
      const float* bih = get("predictor.rnn.bias_ih_l" + s, 4 * H);
      const float* bhh = get("predictor.rnn.bias_hh_l" + s, 4 * H);
      std::vector<float> a = transpose(wih, 4 * H, in, 4 * H), bm = transpose(whh, 4 * H, H, 4 * H);
      a.insert(a.end(), bm.begin(), bm.end());   // [(in + H)][4H]
      img.put(a, &w.wg[l]);
      std::vector<float> bias(4 * H);
      for (int i = 0; i < 4 * H; ++i) bias[i] = bih[i] + bhh[i];
      img.put(bias, &w.bg[l]);
      h->host_wg.push_back(std::move(a));
      h->host_bg.push_back(std::move(bias));
    }
    if (!sl) {
      // projection (predictor.py:204) and the joint's pred_ffn (joint.py:86) are consecutive Linear
      // layers with nothing between them: composed once here (f64 products, f32 result) into one
      // [J, H] matrix, so an emission's predictor runs one matrix-vector product fewer (and the
      // multi-CU search one grid barrier fewer)
      const float* wpm = get("predictor.projection.weight", (int64_t)P * H);
      const float* bp = get("predictor.projection.bias", P);
      const float* wpjm = get("joint.pred_ffn.weight", (int64_t)J * P);
      const float* bpj = get("joint.pred_ffn.bias", J);
      std::vector<float> wc((size_t)J * H), bc(J);
      {
        std::vector<double> row(H);
        for (int j = 0; j < J; ++j) {
          std::fill(row.begin(), row.end(), 0.0);
          double b = bpj[j];
          for (int q = 0; q < P; ++q) {
            const double a = wpjm[(size_t)j * P + q];
            const float* src = wpm + (size_t)q * H;
            for (int k = 0; k < H; ++k) row[k] += a * src[k];
            b += a * bp[q];
          }
          for (int k = 0; k < H; ++k) wc[(size_t)j * H + k] = (float)row[k];
          bc[j] = (float)b;
        }
      }
      w.P = J;   // the composed product's width: pvec is the pred_ffn output
      h->host_wp = transpose(wc.data(), J, H, J);   // [H][J]
      img.put(h->host_wp, &w.wp);
      img.put(bc, &w.bp);
    }
    h->host_wo = transpose(get("joint.ffn_out.weight", (int64_t)V * J), V, J, w.Vp);
    img.put(h->host_wo, &w.wo);
    const float* bo = get("joint.ffn_out.bias", V);
    std::vector<float> bov(w.Vp, -std::numeric_limits<float>::infinity());
    std::copy(bo, bo + V, bov.begin());
    img.put(bov, &w.bo);
    const float* we = get("joint.enc_ffn.weight", (int64_t)J * Ee);
    img.put(std::vector<float>(we, we + (size_t)J * Ee), &h->we);
    const float* be = get("joint.enc_ffn.bias", J);
    img.put(std::vector<float>(be, be + J), &h->be);
  } catch (const std::string& e) {
    return set_error(CFM_ERR_VALUE, e);
  }
  if (rnnt_lds_bytes(w) > 160 * 1024) return set_error(CFM_ERR_ASSERT, "predictor / joint too wide for one workgroup's LDS");
  if (hipSetDevice(device) != hipSuccess || hipMalloc(&h->dev_mem, img.bytes.size()) != hipSuccess ||
      hipMemcpy(h->dev_mem, img.bytes.data(), img.bytes.size(), hipMemcpyHostToDevice) != hipSuccess)
    return set_error(CFM_ERR_RUNTIME, std::string("rnnt weights upload: ") + hipGetErrorString(hipGetLastError()));
  for (auto& f : img.fix) *f.second = reinterpret_cast<const float*>((char*)h->dev_mem + f.first);
  h->n_cu = cu_count();
  if (rnnt_grid_build(h.get())) return CFM_ERR_RUNTIME;
  *out = h.release();
  return CFM_OK;
}

void cfm_rnnt_destroy(cfm_rnnt* h) { delete h; }

// enc_proj rows, then the grid path's state (RG_MAXB utterances), barrier counters and error word
size_t cfm_rnnt_workspace_bytes(const cfm_rnnt* h, int32_t rows) {
  if (!h || rows <= 0) return 0;
  const size_t proj = ((size_t)rows * h->cfg.join_dim * sizeof(float) + 255) / 256 * 256;
  return proj + (size_t)RG_MAXB * rnnt_grid_per_utt(h) * 4 + (size_t)RG_MAXB * RG_MAXG * 8 + 256;
}

cfm_status cfm_rnnt_set_option(cfm_rnnt* h, const char* key, int64_t value) {
  if (!h || !key) return set_error(CFM_ERR_VALUE, "null argument");
  if (std::string(key) == "grid_blocks") {
    if (value < 0 || value > 256) return set_error(CFM_ERR_VALUE, "grid_blocks: 0 (off) .. 256");
    if (h->w.kind != CFM_RNNT_PRED_RNN) return CFM_OK;   // accepted, no effect: a stateless handle has no grid path
    h->grid_blocks = (int)value;
    if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      return set_error(CFM_ERR_RUNTIME, "rnnt: device sync");
    return rnnt_grid_build(h) ? CFM_ERR_RUNTIME : CFM_OK;
  }
  if (std::string(key) == "grid_lds") {
    h->grid_lds = value != 0;
    return CFM_OK;
  }
  if (std::string(key) == "grid_atomic") {
    h->grid_atomic = value != 0;
    return CFM_OK;
  }
  if (std::string(key) == "grid_force_error") {
    h->grid_force_error = value != 0;
    return CFM_OK;
  }
  if (std::string(key) == "lattice_dtype") {
    if (value != CFM_DTYPE_F32 && value != CFM_DTYPE_BF16)
      return set_error(CFM_ERR_VALUE, "lattice_dtype: CFM_DTYPE_F32 or CFM_DTYPE_BF16");
    h->lattice_dtype = (int)value;
    return CFM_OK;
  }
  return set_error(CFM_ERR_VALUE, std::string("unknown rnnt option ") + key);
}

int32_t cfm_rnnt_grid_blocks(const cfm_rnnt* h, int32_t B) {
  if (!h || B <= 0 || h->grid_blocks <= 0 || B > RG_MAXB || (int64_t)B * h->grid_blocks > h->n_cu) return 0;
  if (h->w.kind != CFM_RNNT_PRED_RNN) return 0;   // the multi-CU search is built for the LSTM predictor only
  const int G = h->grid_blocks;
  // the joint's per-workgroup candidates reuse the z block: <= 64 column groups per workgroup, J >= 128
  if ((h->w.Vp / 4 + G - 1) / G > 64 || h->w.J < 128) return 0;
  // rg_matvec gives every output column of a slice its own thread: the LSTM units (ceil(H / G)) and the
  // composed projection's column quads (ceil(P / 4 / G)) of one workgroup must fit in its RG_NT threads
  if ((h->w.H + G - 1) / G > RG_NT || (h->w.P / 4 + G - 1) / G > RG_NT) return 0;
  return G;
}

int32_t cfm_rnnt_error(const cfm_rnnt* h, const void* ws, int32_t rows) {
  if (!h || !ws || rows <= 0) return 0;
  const size_t at = cfm_rnnt_workspace_bytes(h, rows) - 256;
  int32_t e = 0;
  if (hipMemcpy(&e, (const char*)ws + at, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return e;
}

cfm_status cfm_rnnt_greedy(const cfm_rnnt* h, const float* enc, int32_t rows, const int32_t* row_start,
                           const int32_t* row_len, int32_t B, int32_t n_steps, int32_t* out, void* ws, size_t wsb,
                           cfm_stream stream) {
  return cfm_rnnt_greedy_ex(h, enc, rows, row_start, row_len, B, n_steps, out, ws, wsb, 0, stream);
}

cfm_status cfm_rnnt_greedy_ex(const cfm_rnnt* h, const float* enc, int32_t rows, const int32_t* row_start,
                              const int32_t* row_len, int32_t B, int32_t n_steps, int32_t* out, void* ws, size_t wsb,
                              int32_t flags, cfm_stream stream) {
  if (!h) return set_error(CFM_ERR_VALUE, "null handle");
  if (B < 0 || rows < 0 || n_steps < 1) return set_error(CFM_ERR_VALUE, "bad B / rows / n_steps");
  if (B == 0 || rows == 0) return CFM_OK;
  if (!enc || !row_start || !row_len || !out || !ws) return set_error(CFM_ERR_VALUE, "null argument");
  if (wsb < cfm_rnnt_workspace_bytes(h, rows)) return set_error(CFM_ERR_VALUE, "rnnt workspace too small");
  if (hipSetDevice(h->device) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipSetDevice");
  const hipStream_t st = (hipStream_t)stream;
  float* proj = (float*)ws;
  EpiArgs e;
  e.bias = h->be; e.out = proj; e.ldo = h->cfg.join_dim;
  int r = gemm<float>(EPI_STORE, ACT_NONE, enc, h->cfg.enc_dim, h->we, h->cfg.enc_dim, rows, h->cfg.join_dim,
                      h->cfg.enc_dim, e, st);
  if (r) return set_error(CFM_ERR_RUNTIME, std::string("rnnt enc_ffn gemm: ") + hipGetErrorString((hipError_t)r));
  const int G = (flags & CFM_RNNT_ONE_WORKGROUP) ? 0 : cfm_rnnt_grid_blocks(h, B);
  if (G > 0) {
    // grid path: zeroed state slots, counters and error word, then G workgroups per utterance
    const size_t proj_b = ((size_t)rows * h->cfg.join_dim * sizeof(float) + 255) / 256 * 256;
    const size_t per = rnnt_grid_per_utt(h);
    char* gbase = (char*)ws + proj_b;
    float* scratch = (float*)gbase;
    unsigned long long* bars = (unsigned long long*)(gbase + (size_t)RG_MAXB * per * 4);
    int* err = (int*)((char*)bars + (size_t)RG_MAXB * RG_MAXG * 8);
    if (hipMemsetAsync(scratch, 0, (size_t)B * per * 4, st) != hipSuccess ||
        hipMemsetAsync(bars, 0, (size_t)RG_MAXB * RG_MAXG * 8 + 256, st) != hipSuccess ||
        (h->grid_force_error && hipMemsetAsync(err, 1, 1, st) != hipSuccess))
      return set_error(CFM_ERR_RUNTIME, "rnnt: workspace memset");
    // the largest workgroup's weight slices (float4s): cached in LDS when they fit beside the work area
    const RnntDev& w = h->w;
    auto cdiv = [&](int a) { return (size_t)((a + G - 1) / G); };
    size_t slice4 = 0;
    for (int l = 0, in = w.E; l < w.nl; ++l, in = w.H) slice4 += (size_t)(in + w.H) * cdiv(w.H);
    slice4 += (size_t)w.H * cdiv(w.P / 4) + (size_t)w.J * cdiv(w.Vp / 4);   // what the kernel copies: wp, wo
    const size_t work = rnnt_grid_lds_bytes(w);
    const bool cache = h->grid_lds && work + slice4 * 16 <= 160 * 1024;
    const size_t glds = work + (cache ? slice4 * 16 : 0);
    // 0 = launched, 1 = the kernel cannot hold a workgroup on a CU at this LDS size (one-workgroup path instead),
    // -1 = error.  The grid barriers need all B * G workgroups resident at once: B * G <= CUs is checked by
    // cfm_rnnt_grid_blocks, one workgroup per CU by the occupancy query; a barrier that still times out (CUs
    // held by another stream's kernels) sets the error word and RNNTGreedy.greedy_packed reruns the search on
    // the one-workgroup kernel
    auto launch = [&](auto kern) -> int {
      if (glds > 64 * 1024 &&
          hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)glds) != hipSuccess)
        return -1;
      int per_cu = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, RG_NT, glds) != hipSuccess) return -1;
      if (per_cu < 1) return 1;
      hipLaunchKernelGGL(kern, dim3(B * G), dim3(RG_NT), glds, st, h->w, h->gw, scratch, (int)per, bars, err, proj,
                         row_start, row_len, n_steps, out);
      return 0;
    };
    const bool atom = h->grid_atomic != 0;
    const int okl = cache ? (atom ? launch(rnnt_grid_kernel<true, true>) : launch(rnnt_grid_kernel<true, false>))
                          : (atom ? launch(rnnt_grid_kernel<false, true>) : launch(rnnt_grid_kernel<false, false>));
    if (okl < 0) return set_error(CFM_ERR_RUNTIME, "rnnt: dynamic LDS attribute / occupancy query");
    if (okl == 0) {
      const hipError_t ge = hipGetLastError();
      if (ge != hipSuccess) return set_error(CFM_ERR_RUNTIME, std::string("rnnt_grid_kernel: ") + hipGetErrorString(ge));
      return CFM_OK;
    }
  }
  const size_t lds = rnnt_lds_bytes(h->w);
  const bool sl = h->w.kind != CFM_RNNT_PRED_RNN;
  const void* kern = sl ? (const void*)rnnt_greedy_kernel<true> : (const void*)rnnt_greedy_kernel<false>;
  if (lds > 64 * 1024 && hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return set_error(CFM_ERR_RUNTIME, "rnnt: dynamic LDS attribute");
  if (sl)
    hipLaunchKernelGGL(rnnt_greedy_kernel<true>, dim3(B), dim3(RNNT_NT), lds, st, h->w, proj, row_start, row_len,
                       n_steps, out);
  else
    hipLaunchKernelGGL(rnnt_greedy_kernel<false>, dim3(B), dim3(RNNT_NT), lds, st, h->w, proj, row_start, row_len,
                       n_steps, out);
  const hipError_t le = hipGetLastError();
  if (le != hipSuccess) return set_error(CFM_ERR_RUNTIME, std::string("rnnt_greedy_kernel: ") + hipGetErrorString(le));
  return CFM_OK;
}

}  // extern "C"
