// Full-sum transducer score of given hypotheses (the reference's Transducer._cal_transducer_score = -rnnt_loss, the
// third score of the modes rnnt_beam_attn_rescoring / ctc_beam_td_attn_rescoring, transducer/transducer.py:257-391)
// over the cfm_rnnt handle.  DESIGN §9g.
//
// Hypothesis i of utterance utt (T encoder rows) with U tokens has U + 1 predictor states p_0 .. p_U (p_u after
// [blank, y_1 .. y_u]) and T (U + 1) lattice nodes, node (t, u) at node0[i] + t (U + 1) + u.  The reference
// materialises joint(enc, pred) as [n_hyps, T, U + 1, V]; only two numbers per node are ever used:
//   b[t,u] = log_softmax(ffn_out(tanh(enc_ffn(x_t) + pred_ffn(p_u))))[blank],    k[t,u] = the same at y_{u+1}.
//
//   gemm<float>          enc_proj [rows, J] (enc_ffn with bias)
//   per step s <= max U  rl_step_kernel (state s's consumed token per hypothesis), the beam search's predictor step
//                        (rb_predictor: embedding, LSTM layers, composed projection + pred_ffn), rl_advance_kernel
//                        (pj -> pred_proj[first_state + s], the new LSTM state becomes the state)
//   (a stateless handle)  instead of those steps: rl_window_kernel (the id window of every state) and one pass of the
//                        beam search's stateless predictor (sl_predictor) over all n_states states -> pred_proj
//   rl_joint_kernel      one workgroup per tile of 32 or 64 consecutive nodes (tiles straddle hypotheses and end inside
//                        a lattice): z = tanh(e_t + p_u) is formed once into LDS and stays there for the whole sweep
//                        over V; ffn_out streams through LDS in tiles of 128 vocabulary rows x 32 (bf16: 64) columns of K (the
//                        next tile's global loads are in flight under the current tile's MFMAs).  ffn_out rows are
//                        the MFMA A operand and the nodes the B operand (32x32x2 f32, or 32x32x16 bf16 with f32
//                        accumulation), so a node's column sits on a lane and the vocabulary index in the 16
//                        accumulator registers: the online max / sum over V and the two picked logits are in-lane,
//                        plus one half-wave swap and a merge of the four waves (which split each V tile) at the end.
//                        Eight bytes per node leave the CU.
//   rl_alpha_kernel      one workgroup per hypothesis walks the anti-diagonals in f64 (beam.h's log_add), two diagonals
//                        in LDS (U + 1 <= 2048) or in the workspace; workgroup barriers only.
// No kernel waits for another workgroup.  Every index a kernel forms from a descriptor is clamped into its array, and
// a descriptor that does not fit its arrays sets the status word and gives td 0.
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

constexpr int RL_NT = 256;            // threads of a joint workgroup: four waves, each 32 rows of a V tile
constexpr int RL_VT = 128;            // vocabulary rows per tile
constexpr int RL_PADB = 16;           // row padding of the LDS images (bytes)
constexpr int RL_LDS_MAX = 160 * 1024;
constexpr int RL_ALPHA_LDS = 2048;    // U + 1 up to this keeps the two diagonals in LDS

struct RlJoint {
  const float *enc_proj, *pred_proj, *bias;   // [rows, J], [n_states, J], [V]
  const void* W;                              // ffn_out [V][J] f32, or its two bf16 images [2][V][J]
  const int32_t *tokens, *ustart, *desc;
  const int64_t* node0;
  float *b, *k;
  int64_t total;
  int rows, n_states, B, n_hyp, J, V, blank;
};

// the hypothesis of node n: the last i with node0[i] <= n
CFM_DEV int rl_find_hyp(const int64_t* __restrict__ node0, int n_hyp, int64_t n) {
  int lo = 0, hi = n_hyp - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (node0[mid] <= n) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <typename T> struct RlOp;
template <> struct RlOp<float> {
  // lane (r, h) holds k = 8 s + 4 h + e of its row: four 32x32x2 steps, step e pairing element e of both operands
  static CFM_DEV f32x16 mma(const float* a, const float* b, f32x16 acc) {
    const f32x4 av = *reinterpret_cast<const f32x4*>(a), bv = *reinterpret_cast<const f32x4*>(b);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], acc, 0, 0, 0);
    return acc;
  }
  static constexpr int KSTEP = 8;   // K per mma() call
  static constexpr int NW = 1;      // images of ffn_out whose products are summed
};
template <> struct RlOp<bf16> {
  static CFM_DEV f32x16 mma(const bf16* a, const bf16* b, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(a),
                                                   *reinterpret_cast<const bf16x8*>(b), acc, 0, 0, 0);
  }
  static constexpr int KSTEP = 16;
  // ffn_out as two bf16 terms, hi = bf16(w) and lo = bf16(w - hi), both multiplied with the same bf16 z: the weights'
  // rounding is a fixed error that does not average out along a lattice (one term alone moved a total by up to 0.14,
  // 0.10 of it from the weights), and the MFMA pipe has room for the second product
  static constexpr int NW = 2;
};

template <typename T, int NB, int KC> constexpr size_t rl_joint_lds(int J) {
  return (size_t)32 * NB * (J * sizeof(T) + RL_PADB) + (size_t)RlOp<T>::NW * RL_VT * (KC * sizeof(T) + RL_PADB) +
         (size_t)4 * 32 * NB * 16 + (size_t)32 * NB * 12;
}

// KC: the columns of K per staged ffn_out tile (a divisor of J)
template <typename T, int NB, int KC>
__global__ __launch_bounds__(RL_NT) void rl_joint_kernel(const RlJoint a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rl_smem[];
  constexpr int NN = 32 * NB;                       // nodes of this workgroup
  constexpr int KSTEP = RlOp<T>::KSTEP, NW = RlOp<T>::NW;
  constexpr int EPV = 16 / sizeof(T);               // elements per 16-byte vector
  constexpr int WS = KC + RL_PADB / sizeof(T);      // W tile row stride (elements)
  constexpr int VPR = KC / EPV;                     // vectors per staged row
  constexpr int NV = RL_VT * VPR / RL_NT;           // vectors per thread and tile
  const int J = a.J, V = a.V, ZS = J + RL_PADB / (int)sizeof(T);
  T* z = reinterpret_cast<T*>(rl_smem);                                 // [NN][ZS]
  T* wt = z + (size_t)NN * ZS;                                          // [NW][RL_VT][WS]
  float* red = reinterpret_cast<float*>(wt + (size_t)NW * RL_VT * WS);       // [4][NN][4]: m, s, blank logit, target logit
  int* s_row = reinterpret_cast<int*>(red + 4 * NN * 4);                // [NN] encoder row, state, target of a node
  int* s_state = s_row + NN;
  int* s_tgt = s_state + NN;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int64_t n_first = (int64_t)blockIdx.x * NN;

  if (tid < NN) {
    const int64_t n = min(n_first + tid, a.total - 1);   // a tile that ends past the lattice repeats the last node
    const int i = rl_find_hyp(a.node0, a.n_hyp, n);
    const int utt = min(max(a.desc[4 * i], 0), a.B - 1);
    const int st0 = a.desc[4 * i + 1], U1 = max(a.desc[4 * i + 2], 1);
    const int64_t local = max(n - a.node0[i], (int64_t)0);
    const int64_t t = local / U1;
    const int u = (int)(local - t * U1);
    s_row[tid] = (int)min(max((int64_t)a.ustart[utt] + t, (int64_t)0), (int64_t)a.rows - 1);
    const int st = min(max(st0 + u, 0), a.n_states - 1);
    s_state[tid] = st;
    s_tgt[tid] = (u + 1 < U1 && st + 1 < a.n_states) ? a.tokens[st + 1] : -1;
  }
  __syncthreads();
  // z = tanh(e_t + p_u), once per tile
  for (int q = tid; q < NN * (J >> 2); q += RL_NT) {
    const int nd = q / (J >> 2), j = (q - nd * (J >> 2)) << 2;
    const f32x4 e = *reinterpret_cast<const f32x4*>(a.enc_proj + (size_t)s_row[nd] * J + j);
    const f32x4 p = *reinterpret_cast<const f32x4*>(a.pred_proj + (size_t)s_state[nd] * J + j);
    T* o = z + (size_t)nd * ZS + j;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = from_f32<T>(tanhf(e[c] + p[c]));
  }
  int tgt[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) tgt[nb] = s_tgt[32 * nb + li];

  const int nkc = J / KC, nvt = (V + RL_VT - 1) / RL_VT, G = nkc * nvt;
  const T* W = reinterpret_cast<const T*>(a.W);
  const size_t image = (size_t)V * J;   // image wi of ffn_out at W + wi * image
  u32x4 pf[NW * NV];
  auto fetch = [&](int g) {
    const int v0 = (g / nkc) * RL_VT, kc = (g - (g / nkc) * nkc) * KC;
#pragma unroll
    for (int wi = 0; wi < NW; ++wi)
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const int idx = tid + RL_NT * q, row = idx / VPR, c = idx - row * VPR;
        pf[wi * NV + q] = v0 + row < V
                              ? *reinterpret_cast<const u32x4*>(W + wi * image + (size_t)(v0 + row) * J + kc + c * EPV)
                              : (u32x4){0u, 0u, 0u, 0u};   // padding rows: zero weights, bias -inf below
      }
  };
  float m[NB], s[NB], xb[NB], xk[NB];
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) { m[nb] = -INFINITY; s[nb] = 0.f; xb[nb] = -INFINITY; xk[nb] = -INFINITY; }
  fetch(0);
  for (int g = 0; g < G; ++g) {
    const int vt = g / nkc, kci = g - vt * nkc;
    __syncthreads();   // the previous tile's reads of wt are done (first round: z is complete)
#pragma unroll
    for (int wi = 0; wi < NW; ++wi)
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const int idx = tid + RL_NT * q, row = idx / VPR, c = idx - row * VPR;
        *reinterpret_cast<u32x4*>(wt + ((size_t)wi * RL_VT + row) * WS + c * EPV) = pf[wi * NV + q];
      }
    __syncthreads();
    if (g + 1 < G) fetch(g + 1);
    if (kci == 0) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    }
    const T* ap = wt + (size_t)(32 * w + li) * WS + (KSTEP / 2) * lh;
    const T* bp = z + (size_t)li * ZS + kci * KC + (KSTEP / 2) * lh;
#pragma unroll
    for (int ks = 0; ks < KC / KSTEP; ++ks)
#pragma unroll
      for (int wi = 0; wi < NW; ++wi)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          acc[nb] = RlOp<T>::mma(ap + (size_t)wi * RL_VT * WS + ks * KSTEP, bp + (size_t)32 * nb * ZS + ks * KSTEP,
                                 acc[nb]);
    if (kci == nkc - 1) {
      // this wave's 32 rows of the V tile: accumulator register r of lane (li, lh) is row 8 (r >> 2) + 4 lh + (r & 3)
      float bias[16];
      int rowv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        rowv[r] = vt * RL_VT + 32 * w + 8 * (r >> 2) + 4 * lh + (r & 3);
        bias[r] = rowv[r] < V ? a.bias[rowv[r]] : -INFINITY;
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        float x[16], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          x[r] = acc[nb][r] + bias[r];
          mx = fmaxf(mx, x[r]);
          if (rowv[r] == a.blank) xb[nb] = x[r];
          if (rowv[r] == tgt[nb]) xk[nb] = x[r];
        }
        if (mx > -INFINITY) {
          const float mn = fmaxf(m[nb], mx);
          float add = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) add += expf(x[r] - mn);
          s[nb] = s[nb] * expf(m[nb] - mn) + add;   // (m = -inf: s = 0 and exp(-inf) = 0)
          m[nb] = mn;
        }
      }
    }
  }
  // the two half-waves hold different rows of the same nodes
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const float om = __shfl_xor(m[nb], 32, 64), os = __shfl_xor(s[nb], 32, 64);
    const float ob = __shfl_xor(xb[nb], 32, 64), ok = __shfl_xor(xk[nb], 32, 64);
    const float mn = fmaxf(m[nb], om);
    float sn = 0.f;
    if (m[nb] > -INFINITY) sn += s[nb] * expf(m[nb] - mn);
    if (om > -INFINITY) sn += os * expf(om - mn);
    if (lh == 0) {
      float* o = red + ((size_t)w * NN + 32 * nb + li) * 4;
      o[0] = mn; o[1] = sn; o[2] = fmaxf(xb[nb], ob); o[3] = fmaxf(xk[nb], ok);
    }
  }
  __syncthreads();
  if (tid < NN && n_first + tid < a.total) {
    float mn = -INFINITY, vb = -INFINITY, vk = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* o = red + ((size_t)q * NN + tid) * 4;
      mn = fmaxf(mn, o[0]); vb = fmaxf(vb, o[2]); vk = fmaxf(vk, o[3]);
    }
    float sn = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* o = red + ((size_t)q * NN + tid) * 4;
      if (o[0] > -INFINITY) sn += o[1] * expf(o[0] - mn);
    }
    const float lse = logf(sn);
    a.b[n_first + tid] = (vb - mn) - lse;
    a.k[n_first + tid] = s_tgt[tid] >= 0 ? (vk - mn) - lse : 0.f;
  }
}

// ----------------------------------------------------------------------------- descriptors, predictor steps
// per hypothesis: T and U + 1 for the recursion (T = 0: not scored) and the status word for a descriptor outside its
// arrays (the joint kernel clamps, the recursion skips)
__global__ __launch_bounds__(64) void rl_check_kernel(const int32_t* __restrict__ desc, const int64_t* __restrict__ node0,
                                                      const int32_t* __restrict__ ulen, const int32_t* __restrict__ tokens,
                                                      int n_hyp, int B, int n_states, int max_u1, int V, int64_t total,
                                                      int32_t* __restrict__ hyp_t, int32_t* __restrict__ hyp_u1,
                                                      int32_t* __restrict__ err) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_hyp) return;
  const int utt = desc[4 * i], st0 = desc[4 * i + 1], U1 = desc[4 * i + 2];
  bool ok = utt >= 0 && utt < B && st0 >= 0 && U1 >= 1 && U1 <= max_u1 && U1 <= n_states - st0;
  int T = 0;
  if (ok) {
    T = ulen[utt];
    const int64_t n0 = node0[i];
    ok = T >= 1 && n0 >= 0 && node0[i + 1] - n0 == (int64_t)T * U1 && node0[i + 1] <= total;
    for (int u = 0; ok && u < U1; ++u) ok = tokens[st0 + u] >= 0 && tokens[st0 + u] < V;
  }
  if (!ok) err[0] = BEAM_ERR_RANGE;
  hyp_t[i] = ok ? T : 0;
  hyp_u1[i] = ok ? U1 : 1;
}

struct RlState {
  float *h[RNNT_MAXL], *c[RNNT_MAXL];        // the state rb_predictor reads: h part of xh[l][0] (row stride h_ld), c[l][0]
  const float *hn[RNNT_MAXL], *cn[RNNT_MAXL];
  int h_ld[RNNT_MAXL];
  int nl, H, J;
};

// state s's consumed token of every hypothesis (a hypothesis with fewer states repeats its last one: unused)
__global__ __launch_bounds__(64) void rl_step_kernel(const int32_t* __restrict__ desc, const int32_t* __restrict__ tokens,
                                                     int n_hyp, int n_states, int s, int32_t* __restrict__ tok) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_hyp) return;
  const int U1 = max(desc[4 * i + 2], 1);
  const int st = min(max(desc[4 * i + 1] + min(s, U1 - 1), 0), n_states - 1);
  tok[i] = tokens[st];
}

// pj of step s into pred_proj[first_state + s]; the state after the token becomes the state of the next step
__global__ __launch_bounds__(128) void rl_advance_kernel(const RlState a, const int32_t* __restrict__ desc, int n_states,
                                                         int s, const float* __restrict__ pj,
                                                         float* __restrict__ pred_proj) {
  const int i = blockIdx.x;
  const int st0 = desc[4 * i + 1], U1 = desc[4 * i + 2];
  if (s < U1 && st0 >= 0 && st0 + s < n_states)
    for (int j = threadIdx.x; j < a.J; j += 128) pred_proj[(size_t)(st0 + s) * a.J + j] = pj[(size_t)i * a.J + j];
  for (int l = 0; l < a.nl; ++l)
    for (int e = threadIdx.x; e < a.H; e += 128) {
      a.h[l][(size_t)i * a.h_ld[l] + e] = a.hn[l][(size_t)i * a.H + e];
      a.c[l][(size_t)i * a.H + e] = a.cn[l][(size_t)i * a.H + e];
    }
}

// A stateless handle: the id window of every state of every hypothesis, win [n_states][Kc] (oldest first, -1 = a zero
// vector).  State s of hypothesis i reads tokens[max(first_state, s - Kc + 1) .. s]: never the previous hypothesis'
// tokens in the packed array.  A state that no valid hypothesis owns keeps the all -1 window the caller set.
__global__ __launch_bounds__(64) void rl_window_kernel(const int32_t* __restrict__ desc, const int32_t* __restrict__ tokens,
                                                       const int32_t* __restrict__ hyp_t, int n_states, int max_u1, int Kc,
                                                       int V, int32_t* __restrict__ win) {
  const int i = blockIdx.x;
  if (hyp_t[i] <= 0) return;   // (rl_check_kernel: the descriptor is outside its arrays)
  const int st0 = desc[4 * i + 1], U1 = min(desc[4 * i + 2], max_u1);
  for (int e = threadIdx.x; e < U1 * Kc; e += 64) {
    const int u = e / Kc, c = e - u * Kc;
    const int p = u - (Kc - 1) + c;   // the position in the hypothesis' own states
    if (st0 + u >= n_states) continue;
    win[(size_t)(st0 + u) * Kc + c] = p >= 0 ? min(max(tokens[st0 + p], 0), V - 1) : -1;
  }
}

// ----------------------------------------------------------------------------- the recursion
// The two diagonals are addressed as (which, u): in LDS through the shared array itself, in the workspace through the
// global pointer -- never through one pointer that may be either (a generic pointer to LDS offset 0 minus one element
// leaves the LDS aperture before the instruction's offset brings it back).
template <bool IN_LDS>
CFM_DEV void rl_alpha_walk(double (*s_diag)[RL_ALPHA_LDS], double* __restrict__ g_diag, int max_u1,
                           const float* __restrict__ b, const float* __restrict__ k, int T, int U1, int* s_bad,
                           int32_t* __restrict__ err, double* __restrict__ td_i) {
  const int tid = threadIdx.x, U = U1 - 1;
  auto at = [&](int which, int u) -> double& {
    if constexpr (IN_LDS) return s_diag[which][u];
    else return g_diag[(size_t)which * max_u1 + u];
  };
  if (tid == 0) { at(0, 0) = 0.0; *s_bad = 0; }
  __syncthreads();
  bool bad = false;
  int prev = 0;
  for (int d = 1; d <= T - 1 + U; ++d) {
    const int ulo = max(0, d - (T - 1)), uhi = min(U, d), cur = prev ^ 1;
    for (int u = ulo + tid; u <= uhi; u += 256) {
      const int t = d - u;
      double x = NINF, y = NINF;
      if (t >= 1) x = at(prev, u) + (double)b[(int64_t)(t - 1) * U1 + u];
      if (u >= 1) y = at(prev, u - 1) + (double)k[(int64_t)t * U1 + u - 1];
      const double v = log_add(x, y);
      if (!(fabs(v) < INFINITY)) bad = true;
      at(cur, u) = v;
    }
    __syncthreads();
    prev = cur;
  }
  if (bad) *s_bad = 1;
  __syncthreads();
  if (tid == 0) {
    const double v = at(prev, U) + (double)b[(int64_t)(T - 1) * U1 + U];
    if (*s_bad || !(fabs(v) < INFINITY)) err[0] = BEAM_ERR_NAN;
    *td_i = v;
  }
}

__global__ __launch_bounds__(256) void rl_alpha_kernel(const float* __restrict__ b, const float* __restrict__ k,
                                                       const int32_t* __restrict__ hyp_t, const int32_t* __restrict__ hyp_u1,
                                                       const int64_t* __restrict__ node0, int max_u1, int64_t total,
                                                       double* __restrict__ spill, int32_t* __restrict__ err,
                                                       double* __restrict__ td) {
  __shared__ double s_diag[2][RL_ALPHA_LDS];
  __shared__ int s_bad;
  const int i = blockIdx.x, tid = threadIdx.x;
  const int T = hyp_t[i], U1 = hyp_u1[i];
  const int64_t base = node0[i];
  if (T < 1 || U1 < 1 || U1 > max_u1 || base < 0 || (int64_t)T * U1 > total - base) {   // (uniform over the workgroup)
    if (tid == 0) {
      if (T != 0) err[0] = BEAM_ERR_RANGE;   // T = 0: the descriptor check has already said so
      td[i] = 0.0;
    }
    return;
  }
  if (U1 <= RL_ALPHA_LDS)
    rl_alpha_walk<true>(s_diag, nullptr, max_u1, b + base, k + base, T, U1, &s_bad, err, td + i);
  else
    rl_alpha_walk<false>(s_diag, spill + (size_t)i * 2 * max_u1, max_u1, b + base, k + base, T, U1, &s_bad, err, td + i);
}

// ----------------------------------------------------------------------------- host side
namespace {

uint16_t rl_bf16(float f) {   // round to nearest even, as the device's (bf16) cast
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// ffn_out as two bf16 images [2][V][J] (hi, then lo = bf16(w - hi)), once per handle
int rl_weights16(cfm_rnnt* h) {
  std::lock_guard<std::mutex> lock(h->lat_mu);
  if (h->lat_mem) return 0;
  const RnntDev& w = h->w;
  const size_t image = (size_t)w.V * w.J;
  std::vector<uint16_t> img(2 * image);
  for (int k = 0; k < w.J; ++k)
    for (int v = 0; v < w.V; ++v) {
      const float x = h->host_wo[(size_t)k * w.Vp + v];
      const uint16_t hi = rl_bf16(x);
      const uint32_t hb = (uint32_t)hi << 16;
      float hf;
      std::memcpy(&hf, &hb, 4);
      img[(size_t)v * w.J + k] = hi;
      img[image + (size_t)v * w.J + k] = rl_bf16(x - hf);
    }
  void* mem = nullptr;
  if (hipMalloc(&mem, img.size() * 2) != hipSuccess) return 1;
  if (hipMemcpy(mem, img.data(), img.size() * 2, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(mem);
    return 1;
  }
  h->lat_mem = mem;
  return 0;
}

template <typename T, int NB, int KC> int rl_joint_launch(const RlJoint& a, hipStream_t st) {
  const size_t lds = rl_joint_lds<T, NB, KC>(a.J);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)rl_joint_kernel<T, NB, KC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
          hipSuccess)
    return (int)hipErrorInvalidValue;
  const int64_t tiles = (a.total + 32 * NB - 1) / (32 * NB);
  hipLaunchKernelGGL((rl_joint_kernel<T, NB, KC>), dim3((unsigned)tiles), dim3(RL_NT), lds, st, a);
  return (int)hipGetLastError();
}

// 64 nodes per workgroup where their z fits the LDS beside the ffn_out tile, else 32
template <typename T, int KC> int rl_joint_pick(const RlJoint& a, hipStream_t st) {
  if (rl_joint_lds<T, 2, KC>(a.J) <= (size_t)RL_LDS_MAX) return rl_joint_launch<T, 2, KC>(a, st);
  return rl_joint_launch<T, 1, KC>(a, st);
}

// the joint over the nodes; dtype as cfm_dtype
cfm_status rl_joint(cfm_rnnt* h, int dtype, RlJoint a, hipStream_t st) {
  const RnntDev& w = h->w;
  if (w.J % 32 != 0 || w.J > 1024 || w.V < 2) return set_error(CFM_ERR_ASSERT, "rnnt lattice: join_dim a multiple of 32 up to 1024");
  if (a.total > (int64_t)0x7fffffff * 32) return set_error(CFM_ERR_VALUE, "rnnt lattice: too many nodes for one call");
  a.J = w.J; a.V = w.V; a.blank = w.blank; a.bias = w.bo;
  if (dtype == CFM_DTYPE_F32) {
    a.W = h->bw_o;
    KCHK((rl_joint_pick<float, 32>(a, st)));
  } else {
    if (rl_weights16(h)) return set_error(CFM_ERR_RUNTIME, "rnnt lattice: weights upload");
    a.W = h->lat_mem;
    if (w.J % 64 == 0) KCHK((rl_joint_pick<bf16, 64>(a, st)));
    else KCHK((rl_joint_pick<bf16, 32>(a, st)));
  }
  return CFM_OK;
}

struct RlWS {
  RbWS rb;
  int32_t *hyp_t, *hyp_u1;
  float *pred_proj, *b, *k;
  double* spill;
  int32_t* win;       // a stateless handle: [n_states][Kc] id windows, the mixed vectors and the predictor outputs
  float *sx, *sy;     // [n_states][E]
};

bool rl_geom_ok(const cfm_rnnt* h, int rows, int n_hyp, int n_states, int max_u1, int64_t total) {
  return h && rows >= 1 && n_hyp >= 1 && n_hyp <= (1 << 20) && n_states >= n_hyp && max_u1 >= 1 && max_u1 <= n_states &&
         total >= n_hyp && total <= (int64_t)rows * n_states && total <= (int64_t)0x7fffffff * 32 &&
         rb_geom_ok(h, rows, n_hyp, 1);
}

RlWS rl_carve(const cfm_rnnt* h, void* base, int rows, int n_hyp, int n_states, int max_u1, int64_t total, size_t* bytes) {
  RlWS s;
  size_t t = 0;
  s.rb = rb_carve(h, base, rows, n_hyp, 1, &t);   // its error word is the first word of the workspace
  Carver c(base);
  c.off = t;
  s.hyp_t = c.take<int32_t>(n_hyp);
  s.hyp_u1 = c.take<int32_t>(n_hyp);
  s.pred_proj = c.take<float>((size_t)n_states * h->w.J);
  s.b = c.take<float>((size_t)total);
  s.k = c.take<float>((size_t)total);
  s.spill = c.take<double>(max_u1 > RL_ALPHA_LDS ? (size_t)n_hyp * 2 * max_u1 : 1);
  s.win = nullptr;
  s.sx = s.sy = nullptr;
  if (h->w.kind != CFM_RNNT_PRED_RNN) {
    s.win = c.take<int32_t>((size_t)n_states * h->w.Kc);
    s.sx = c.take<float>((size_t)n_states * h->w.E);
    s.sy = c.take<float>((size_t)n_states * h->w.E);
  }
  if (bytes) *bytes = c.off;
  return s;
}

}  // namespace
}  // namespace cfm

using namespace cfm;

extern "C" {

size_t cfm_rnnt_td_workspace_bytes(const cfm_rnnt* h, int32_t rows, int32_t n_hyp, int32_t n_states, int32_t max_u1,
                                   int64_t total_nodes) {
  if (!rl_geom_ok(h, rows, n_hyp, n_states, max_u1, total_nodes)) return 0;
  size_t t = 0;
  rl_carve(h, nullptr, rows, n_hyp, n_states, max_u1, total_nodes, &t);
  return t + 256;
}

cfm_status cfm_rnnt_td_score(cfm_rnnt* h, const float* enc, int32_t rows, const int32_t* row_start,
                             const int32_t* row_len, int32_t B, const int32_t* tokens, int32_t n_states,
                             const int32_t* desc, const int64_t* node0, int32_t n_hyp, int32_t max_u1,
                             int64_t total_nodes, int32_t dtype, double* td_out, void* ws, size_t wsb,
                             cfm_stream stream) {
  if (!h) return set_error(CFM_ERR_VALUE, "null handle");
  if (dtype != -1 && dtype != CFM_DTYPE_F32 && dtype != CFM_DTYPE_BF16)
    return set_error(CFM_ERR_VALUE, "rnnt td score: dtype f32, bf16 or -1 (the handle's lattice_dtype)");
  if (n_hyp == 0) return CFM_OK;
  if (B < 1 || !rl_geom_ok(h, rows, n_hyp, n_states, max_u1, total_nodes))
    return set_error(CFM_ERR_VALUE, "rnnt td score: bad rows / hypotheses / states / nodes");
  if (!rb_widths_ok(h))
    return set_error(CFM_ERR_ASSERT, "rnnt td score: embed_size, hidden_size and join_dim must be multiples of 32");
  if (!enc || !row_start || !row_len || !tokens || !desc || !node0 || !td_out || !ws)
    return set_error(CFM_ERR_VALUE, "null argument");
  if (wsb < cfm_rnnt_td_workspace_bytes(h, rows, n_hyp, n_states, max_u1, total_nodes))
    return set_error(CFM_ERR_VALUE, "rnnt td workspace too small");
  if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(enc)) & 15)
    return set_error(CFM_ERR_VALUE, "encoder rows / workspace must be 16-byte aligned");
  if (hipSetDevice(h->device) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipSetDevice");
  if (rb_weights(h)) return set_error(CFM_ERR_RUNTIME, "rnnt td score: weights upload");
  const hipStream_t st = (hipStream_t)stream;
  const RnntDev& w = h->w;
  const RlWS s = rl_carve(h, ws, rows, n_hyp, n_states, max_u1, total_nodes, nullptr);
  const RbWS& r = s.rb;
  if (hipMemsetAsync(r.err, 0, r.zero_bytes, st) != hipSuccess ||
      hipMemsetAsync((char*)ws + r.act_off, 0, r.act_bytes, st) != hipSuccess ||
      hipMemsetAsync(s.pred_proj, 0, (size_t)n_states * w.J * 4, st) != hipSuccess)
    return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
  // the utterances' validated row ranges.  rb_carve sized its per-utterance arrays for n_hyp >= the utterances that
  // have a hypothesis; a caller with more utterances than hypotheses passes only those (B <= n_hyp)
  if (B > n_hyp) return set_error(CFM_ERR_VALUE, "rnnt td score: more utterances than hypotheses");
  KCHK(rb_init(row_start, row_len, B, 1, rows, rows, w.blank, r, st));
  KCHK(rb_gemm(enc, h->cfg.enc_dim, h->we, h->be, rows, w.J, h->cfg.enc_dim, r.enc_proj, w.J, st));
  hipLaunchKernelGGL(rl_check_kernel, dim3((n_hyp + 63) / 64), dim3(64), 0, st, desc, node0, r.ulen, tokens, n_hyp, B,
                     n_states, max_u1, w.V, total_nodes, s.hyp_t, s.hyp_u1, r.err);
  KCHK((int)hipGetLastError());
  RlState ps{};
  ps.nl = w.nl; ps.H = w.H; ps.J = w.J;
  for (int l = 0; l < w.nl; ++l) {
    const int in = l == 0 ? w.E : w.H;
    ps.h[l] = r.xh[l][0] + in; ps.h_ld[l] = in + w.H;
    ps.c[l] = r.c[l][0]; ps.hn[l] = r.hn[l]; ps.cn[l] = r.cn[l];
  }
  const RbLive lv{nullptr, nullptr, nullptr, 1, 0};
  if (w.kind != CFM_RNNT_PRED_RNN) {
    // the predictor is a function of the last Kc ids: one pass over all n_states states, no sequential steps
    if (hipMemsetAsync(s.win, 0xff, (size_t)n_states * w.Kc * 4, st) != hipSuccess)
      return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
    hipLaunchKernelGGL(rl_window_kernel, dim3(n_hyp), dim3(64), 0, st, desc, tokens, s.hyp_t, n_states, max_u1, w.Kc, w.V,
                       s.win);
    KCHK((int)hipGetLastError());
    if (const cfm_status e = sl_predictor(h, lv, s.win, w.Kc, s.win + w.Kc - 1, w.Kc, n_states, nullptr, s.sx, s.sy,
                                          s.pred_proj, st))
      return e;
  }
  for (int step = 0; w.kind == CFM_RNNT_PRED_RNN && step < max_u1; ++step) {
    hipLaunchKernelGGL(rl_step_kernel, dim3((n_hyp + 63) / 64), dim3(64), 0, st, desc, tokens, n_hyp, n_states, step,
                       r.tok);
    KCHK((int)hipGetLastError());
    if (const cfm_status e = rb_predictor(h, r, lv, n_hyp, 0, st)) return e;
    hipLaunchKernelGGL(rl_advance_kernel, dim3(n_hyp), dim3(128), 0, st, ps, desc, n_states, step, r.pj, s.pred_proj);
    KCHK((int)hipGetLastError());
  }
  RlJoint a{};
  a.enc_proj = r.enc_proj; a.pred_proj = s.pred_proj; a.tokens = tokens; a.ustart = r.ustart; a.desc = desc;
  a.node0 = node0; a.b = s.b; a.k = s.k; a.total = total_nodes; a.rows = rows; a.n_states = n_states; a.B = B;
  a.n_hyp = n_hyp;
  if (const cfm_status e = rl_joint(h, dtype == -1 ? h->lattice_dtype : dtype, a, st)) return e;
  hipLaunchKernelGGL(rl_alpha_kernel, dim3(n_hyp), dim3(256), 0, st, s.b, s.k, s.hyp_t, s.hyp_u1, node0, max_u1,
                     total_nodes, s.spill, r.err, td_out);
  KCHK((int)hipGetLastError());
  return CFM_OK;
}

// ---- operator-level entry points (include/cfm_ops.h)
cfm_status cfm_op_rnnt_lattice(cfm_rnnt* h, int32_t dtype, const float* enc_proj, int32_t rows, const float* pred_proj,
                               int32_t n_states, const int32_t* tokens, const int32_t* row_start,
                               const int32_t* row_len, int32_t B, const int32_t* desc, const int64_t* node0,
                               int32_t n_hyp, int64_t total_nodes, float* b_out, float* k_out, cfm_stream stream) {
  if (!h) return set_error(CFM_ERR_VALUE, "null handle");
  if (dtype != CFM_DTYPE_F32 && dtype != CFM_DTYPE_BF16) return set_error(CFM_ERR_VALUE, "rnnt lattice: dtype f32 or bf16");
  if (rows < 1 || n_states < 1 || B < 1 || n_hyp < 1 || total_nodes < 1)
    return set_error(CFM_ERR_VALUE, "rnnt lattice: bad rows / states / hypotheses / nodes");
  if (!enc_proj || !pred_proj || !tokens || !row_start || !row_len || !desc || !node0 || !b_out || !k_out)
    return set_error(CFM_ERR_VALUE, "null argument");
  if ((reinterpret_cast<uintptr_t>(enc_proj) | reinterpret_cast<uintptr_t>(pred_proj)) & 15)
    return set_error(CFM_ERR_VALUE, "projections must be 16-byte aligned");
  if (hipSetDevice(h->device) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipSetDevice");
  if (rb_weights(h)) return set_error(CFM_ERR_RUNTIME, "rnnt lattice: weights upload");
  RlJoint a{};
  a.enc_proj = enc_proj; a.pred_proj = pred_proj; a.tokens = tokens; a.ustart = row_start; a.desc = desc;
  a.node0 = node0; a.b = b_out; a.k = k_out; a.total = total_nodes; a.rows = rows; a.n_states = n_states; a.B = B;
  a.n_hyp = n_hyp;
  return rl_joint(h, dtype, a, (hipStream_t)stream);
}

size_t cfm_op_rnnt_alpha_workspace_bytes(int32_t n_hyp, int32_t max_u1) {
  if (n_hyp < 1 || n_hyp > (1 << 20) || max_u1 < 1) return 0;
  return 256 + (max_u1 > RL_ALPHA_LDS ? align_up((size_t)n_hyp * 2 * max_u1 * 8) : 256);
}

cfm_status cfm_op_rnnt_alpha(const float* b, const float* k, const int32_t* hyp_t, const int32_t* hyp_u1,
                             const int64_t* node0, int32_t n_hyp, int32_t max_u1, int64_t total_nodes, double* td_out,
                             void* ws, size_t wsb, cfm_stream stream) {
  const size_t need = cfm_op_rnnt_alpha_workspace_bytes(n_hyp, max_u1);
  if (need == 0 || total_nodes < 1) return set_error(CFM_ERR_VALUE, "rnnt alpha: bad hypotheses / states / nodes");
  if (!b || !k || !hyp_t || !hyp_u1 || !node0 || !td_out || !ws) return set_error(CFM_ERR_VALUE, "null argument");
  if (wsb < need) return set_error(CFM_ERR_VALUE, "rnnt alpha workspace too small");
  if (reinterpret_cast<uintptr_t>(ws) & 15) return set_error(CFM_ERR_VALUE, "workspace must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(ws, 0, 256, st) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipMemsetAsync");
  hipLaunchKernelGGL(rl_alpha_kernel, dim3(n_hyp), dim3(256), 0, st, b, k, hyp_t, hyp_u1, node0, max_u1, total_nodes,
                     (double*)((char*)ws + 256), (int32_t*)ws, td_out);
  KCHK((int)hipGetLastError());
  return CFM_OK;
}

}  // extern "C"
