// CTC forced alignment (the consumer the reference runs as utils/model_utils.py:force_align ->
// torchaudio.functional.forced_align on the CPU) on device, semantics in DESIGN.md 9c:
//   ctc_align_trellis_kernel    Viterbi over the S = 2L + 1 states, one workgroup per utterance, alpha
//                               in f64, 2-bit backpointers;
//   ctc_align_backtrace_kernel  one wave per utterance walks the backpointers 64 frames at a time and
//                               writes frames, frame_logp, spans.
//
// Layout.  A thread owns runs of 16 consecutive states: one frame's backpointers of a run are one
// 32-bit word, trellis[t * runs + r], written with a plain store.  An alpha row holds a run as a slot
// of 18 doubles: [alpha(16r - 2), alpha(16r - 1) | alpha(16r) .. alpha(16r + 15)].  The two leading
// doubles repeat the previous run's last two states, so a thread reads its 18 inputs and writes its
// 16 outputs plus the next slot's two copies as 9 contiguous 16-byte accesses each; the 144-byte slot
// stride puts the 16 lanes of a ds_read_b128 group on 16 different 4-bank slots (36 i mod 64 is a
// permutation of the multiples of 4 for i = 0 .. 15).  Slot 0's copies are states -2 and -1: they stay
// -inf, which never wins a `>`.  The two rows (read one, write the other, one barrier per frame) live
// in LDS up to 8192 states (2 * 513 * 144 B = 144 KiB of the CU's 160), above that in the workspace.
//
// Runs that cannot be reached from the start (16r > 2t + 1) or cannot reach the end any more (their
// highest state is further than 2(T - 1 - t) + 1 from S - 1) are skipped: a state that can still reach
// the end reads only states that could at the frame before, so what the skipped runs leave behind is
// never read by a state on a surviving path, and unreached runs are -inf in both rows from the start.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/cfm.h"
#include "cfm_common.h"
#include "status.h"
#include "workspace.h"

namespace cfm {

constexpr int AL_NT = 512;             // threads of a trellis workgroup
constexpr int AL_SLOT = 18;            // doubles per run in an alpha row
constexpr int AL_LDS_STATES = 8192;    // alpha rows in LDS up to this many states
constexpr int AL_LDS_HEAD = 16;        // bytes of flags in front of the LDS rows
constexpr int AL_MAX_NRUN = 3;         // runs per thread held in registers (above: the generic strip loop)

struct AlignArgs {
  const float* lp;
  const int32_t *row_start, *row_len, *targets, *target_start, *target_len;
  const int64_t* ws_off;
  int32_t *frames, *spans, *status, *end_state;
  float* frame_logp;
  double* score;
  char* ws;
  size_t ws_bytes, header_bytes;
  int rows, V, blank, n_targets, lds_states, lds_bytes;
};

__host__ __device__ inline int64_t al_runs(int64_t L) { return (2 * L + 1 + 15) / 16; }
__host__ __device__ inline size_t al_trellis_bytes(int64_t T, int64_t runs) {
  return ((size_t)T * (size_t)runs * 4 + 255) / 256 * 256;
}
__host__ __device__ inline size_t al_row_bytes(int64_t runs) { return (size_t)(runs + 1) * AL_SLOT * 8; }
__host__ __device__ inline size_t al_region_bytes(int64_t T, int64_t L) {
  const int64_t runs = al_runs(L);
  return al_trellis_bytes(T, runs) + (2 * al_row_bytes(runs) + 255) / 256 * 256;
}

struct RunCtx {
  int lab[8];        // labels of the run's 8 odd states (blank where there is none: a safe index)
  uint32_t skip;     // bit j: odd state j may take the skip (its label differs from the one before)
  int nvalid;        // states of the run below S
};

CFM_DEV void load_run(const int32_t* __restrict__ y, int L, int S, int blank, int r, RunCtx& c) {
  const int q0 = 8 * r;
  int prev = (q0 >= 1 && q0 - 1 < L) ? y[q0 - 1] : -1;
  c.skip = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int q = q0 + j;
    const bool in = q < L;
    const int v = in ? y[q] : blank;
    if (in && q >= 1 && v != prev) c.skip |= 1u << j;
    c.lab[j] = v;
    prev = v;
  }
  const int left = S - 16 * r;
  c.nvalid = left < 16 ? left : 16;
}

CFM_DEV void load_em(const float* __restrict__ lpt, const RunCtx& c, float* em) {
#pragma unroll
  for (int j = 0; j < 8; ++j) em[j] = lpt[c.lab[j]];
}

// One frame of one run: k = 0; if (c1 > c[k]) k = 1; if (c2 > c[k]) k = 2 (stay, step, skip).
CFM_DEV uint32_t step_run(const double* prev, double* next, int r, const RunCtx& c, const float* em, float eb) {
  const double NEG = -INFINITY;
  double x[AL_SLOT], o[AL_SLOT];
  const double2* p2 = reinterpret_cast<const double2*>(prev + (size_t)r * AL_SLOT);
#pragma unroll
  for (int i = 0; i < AL_SLOT / 2; ++i) {
    const double2 v = p2[i];
    x[2 * i] = v.x;
    x[2 * i + 1] = v.y;
  }
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    double best = x[i + 2];
    uint32_t k = 0;
    if (x[i + 1] > best) { best = x[i + 1]; k = 1; }
    if ((i & 1) && ((c.skip >> (i >> 1)) & 1u) && x[i] > best) { best = x[i]; k = 2; }
    const float e = (i & 1) ? em[i >> 1] : eb;
    double v = best == NEG ? NEG : best + (double)e;
    if (i >= c.nvalid) { v = NEG; k = 0; }
    o[i] = v;
    w |= k << (2 * i);
  }
  o[16] = o[14];
  o[17] = o[15];
  double2* q2 = reinterpret_cast<double2*>(next + (size_t)r * AL_SLOT + 2);
#pragma unroll
  for (int i = 0; i < AL_SLOT / 2; ++i) q2[i] = make_double2(o[2 * i], o[2 * i + 1]);
  return w;
}

CFM_DEV bool run_active(int r, int t, int T, int S) {
  if (16 * r > 2 * t + 1) return false;
  int top = 16 * r + 15;
  if (top > S - 1) top = S - 1;
  return (S - 1 - top) <= 2 * (T - 1 - t) + 1;
}

CFM_DEV size_t al_idx(int s) { return (size_t)(s >> 4) * AL_SLOT + 2 + (s & 15); }

// NRUN > 0: a thread's runs tid + k * AL_NT, k < NRUN, with their labels in registers and the emissions
// of the next D frames in flight (a ring of D register sets, the frame loop unrolled by D so that no
// set is ever copied: a set is consumed and refilled for frame t + D at once, and the gathers of a fresh
// log-prob row have D frames to arrive); NRUN == 0: any number of strips, labels and emissions fetched
// per frame.
template <int NRUN>
CFM_DEV void trellis_body(const AlignArgs& a, int b, double* row0, double* row1, const float* __restrict__ lp,
                          const int32_t* __restrict__ y, int T, int L, int S, int runs, uint32_t* __restrict__ bpw) {
  const int tid = threadIdx.x;
  const double NEG = -INFINITY;
  const int V = a.V, blank = a.blank;
  constexpr int NR = NRUN > 0 ? NRUN : 1;
  constexpr int D = NRUN == 1 ? 4 : (NRUN == 2 ? 2 : 1);
  RunCtx c[NR];
  float em[D][NR][8];
  float eb[D];
  // both rows -inf (every slot and the one after the last run)
  for (int i = tid; i < (runs + 1) * AL_SLOT; i += AL_NT) {
    row0[i] = NEG;
    row1[i] = NEG;
  }
  if constexpr (NRUN > 0) {
#pragma unroll
    for (int k = 0; k < NRUN; ++k) {
      const int r = tid + k * AL_NT;
      if (r < runs) load_run(y, L, S, blank, r, c[k]);
    }
  }
  __syncthreads();
  if (tid == 0) {
    row0[al_idx(0)] = (double)lp[blank];
    if (L >= 1) row0[al_idx(1)] = (double)lp[y[0]];
  }
  auto fetch = [&](int t, int d) {       // frame t's emissions into set d
    const float* lpt = lp + (size_t)t * V;
    eb[d] = lpt[blank];
#pragma unroll
    for (int k = 0; k < NR; ++k)
      if (tid + k * AL_NT < runs) load_em(lpt, c[k], em[d][k]);
  };
  if constexpr (NRUN > 0) {
#pragma unroll
    for (int d = 0; d < D; ++d)
      if (1 + d < T) fetch(1 + d, d);
  }
  __syncthreads();
  for (int t0 = 1; t0 < T; t0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int t = t0 + d;
      if (t >= T) break;
      const double* prev = (t & 1) ? row0 : row1;
      double* next = (t & 1) ? row1 : row0;
      uint32_t* bpt = bpw + (size_t)t * (size_t)runs;
      if constexpr (NRUN > 0) {
#pragma unroll
        for (int k = 0; k < NRUN; ++k) {
          const int r = tid + k * AL_NT;
          if (r < runs && run_active(r, t, T, S)) bpt[r] = step_run(prev, next, r, c[k], em[d][k], eb[d]);
        }
        if (t + D < T) fetch(t + D, d);
      } else {
        const float* lpt = lp + (size_t)t * V;
        const float ebc = lpt[blank];
        for (int r = tid; r < runs; r += AL_NT) {
          if (!run_active(r, t, T, S)) continue;
          load_run(y, L, S, blank, r, c[0]);
          load_em(lpt, c[0], em[0][0]);
          bpt[r] = step_run(prev, next, r, c[0], em[0][0], ebc);
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    const double* fin = ((T - 1) & 1) ? row1 : row0;
    int e = S - 1;
    double sc = fin[al_idx(S - 1)];
    if (S > 1) {
      const double s2 = fin[al_idx(S - 2)];
      if (s2 > sc) { sc = s2; e = S - 2; }
    }
    if (!(sc - sc == 0.0)) {          // NaN or infinite
      a.status[b] = 4;
    } else {
      a.status[b] = 0;
      a.score[b] = sc;
      a.end_state[b] = e;
    }
  }
}

template <int NRUN>
__global__ __launch_bounds__(AL_NT) void ctc_align_trellis_kernel(AlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* flags = reinterpret_cast<int*>(smem);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t r0 = a.row_start[b], T64 = a.row_len[b], ts = a.target_start[b], L64 = a.target_len[b];
  int st = 0;
  if (r0 < 0 || T64 < 0 || r0 + T64 > a.rows || ts < 0 || L64 < 0 || ts + L64 > a.n_targets) st = 2;
  const int64_t off = a.ws_off[b];
  if (!st && (off < (int64_t)a.header_bytes || (off & 255) != 0 || (size_t)off > a.ws_bytes ||
              al_region_bytes(T64, L64) > a.ws_bytes - (size_t)off))
    st = 5;
  const int T = (int)T64, L = (int)L64, S = 2 * L + 1, runs = (int)al_runs(L64);
  if (!st && NRUN > 0 && runs > NRUN * AL_NT) st = 5;   // device lengths differ from the host's
  if (st) {
    if (tid == 0) a.status[b] = st;
    return;
  }
  const int32_t* y = a.targets + ts;
  if (tid == 0) flags[0] = flags[1] = 0;
  __syncthreads();
  int bad = 0, rep = 0;
  for (int q = tid; q < L; q += AL_NT) {
    const int v = y[q];
    if (v < 0 || v >= a.V || v == a.blank) bad = 1;
    if (q >= 1 && v == y[q - 1]) ++rep;
  }
  if (bad) atomicOr(&flags[0], 1);
  if (rep) atomicAdd(&flags[1], rep);
  __syncthreads();
  bad = flags[0];
  rep = flags[1];
  if (bad || T64 < L64 + rep) {
    if (tid == 0) a.status[b] = bad ? 3 : 1;
    return;
  }
  if (T == 0) {        // then L == 0: the empty alignment
    if (tid == 0) {
      a.status[b] = 0;
      a.score[b] = 0.0;
      a.end_state[b] = 0;
    }
    return;
  }
  char* reg = a.ws + off;
  uint32_t* bpw = reinterpret_cast<uint32_t*>(reg);
  const float* lp = a.lp + (size_t)r0 * a.V;
  const size_t rb = al_row_bytes(runs);
  if (S <= a.lds_states && (size_t)AL_LDS_HEAD + 2 * rb <= (size_t)a.lds_bytes) {
    double* row0 = reinterpret_cast<double*>(smem + AL_LDS_HEAD);
    trellis_body<NRUN>(a, b, row0, row0 + (size_t)(runs + 1) * AL_SLOT, lp, y, T, L, S, runs, bpw);
  } else {
    double* row0 = reinterpret_cast<double*>(reg + al_trellis_bytes(T, runs));
    trellis_body<NRUN>(a, b, row0, row0 + (size_t)(runs + 1) * AL_SLOT, lp, y, T, L, S, runs, bpw);
  }
}

// One wave per utterance.  The state falls by at most 2 per frame, so the 64 rows below the current
// one need only the 9 words that end at the current state's: every lane fetches its row's 9 into LDS
// at once, lane 0 walks them, then the lanes write their rows.
__global__ __launch_bounds__(64) void ctc_align_backtrace_kernel(AlignArgs a) {
  __shared__ uint32_t win[64][9];
  __shared__ int sarr[66];          // [0]: the state one row above the batch; [1 + i]: row t0 - i; [1 + n]: below
  const int b = blockIdx.x, lane = threadIdx.x;
  if (a.status[b] != 0) return;
  const int T = a.row_len[b];
  if (T <= 0) return;
  const int L = a.target_len[b], S = 2 * L + 1, runs = (int)al_runs(L);
  const int64_t r0 = a.row_start[b], ts = a.target_start[b];
  const int32_t* y = a.targets + ts;
  const uint32_t* bpw = reinterpret_cast<const uint32_t*>(a.ws + a.ws_off[b]);
  int s0 = a.end_state[b];
  s0 = s0 < 0 ? 0 : (s0 > S - 1 ? S - 1 : s0);
  int above = -1;
  for (int t0 = T - 1; t0 >= 0; t0 -= 64) {
    const int n = t0 + 1 < 64 ? t0 + 1 : 64;
    const int w_lo = (s0 >> 4) - 8;
    const int row = t0 - lane;
    if (lane < n) {
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const int w = w_lo + j;
        win[lane][j] = (row >= 1 && w >= 0 && w < runs) ? bpw[(size_t)row * (size_t)runs + w] : 0u;
      }
    }
    __syncthreads();
    if (lane == 0) {
      int s = s0;
      sarr[0] = above;
      for (int i = 0; i < n; ++i) {
        sarr[1 + i] = s;
        if (t0 - i >= 1) {
          int j = (s >> 4) - w_lo;
          j = j < 0 ? 0 : (j > 8 ? 8 : j);
          int k = (int)((win[i][j] >> (2 * (s & 15))) & 3u);
          if (k == 3) k = 0;
          s -= k;
          if (s < 0) s = 0;
        }
      }
      sarr[1 + n] = s;
    }
    __syncthreads();
    if (lane < n) {
      const int s = sarr[1 + lane], up = sarr[lane], dn = sarr[2 + lane];
      const int lab = (s & 1) ? y[s >> 1] : a.blank;
      const size_t gr = (size_t)(r0 + row);
      a.frames[gr] = lab;
      if (a.frame_logp) a.frame_logp[gr] = a.lp[gr * (size_t)a.V + lab];
      if ((s & 1) && a.spans) {
        int32_t* sp = a.spans + 2 * (size_t)(ts + (s >> 1));
        if (row == 0 || dn != s) sp[0] = row;
        if (up != s) sp[1] = row;
      }
    }
    const int nabove = sarr[n], ns0 = sarr[1 + n];
    __syncthreads();
    above = nabove;
    s0 = ns0;
  }
}

}  // namespace cfm

using namespace cfm;

// header: end state per utterance | per utterance, at ws_offset[b]: trellis words [row_len, runs],
// then the two alpha rows of the workspace path
size_t cfm_ctc_align_plan(const int32_t* row_len_host, const int32_t* target_len_host, int32_t B,
                          int64_t* ws_offset_host_out) {
  if (B < 0 || (B > 0 && (!row_len_host || !target_len_host))) return 0;
  size_t at = align_up((size_t)(B > 0 ? B : 1) * 4);
  for (int b = 0; b < B; ++b) {
    const int64_t T = row_len_host[b] > 0 ? row_len_host[b] : 0, L = target_len_host[b] > 0 ? target_len_host[b] : 0;
    if (ws_offset_host_out) ws_offset_host_out[b] = (int64_t)at;
    at += al_region_bytes(T, L);
  }
  return at;
}

cfm_status cfm_ctc_align(const float* logp, int32_t rows, int32_t V, const int32_t* row_start, const int32_t* row_len,
                         int32_t B, int32_t blank_id, const int32_t* targets, int32_t n_targets,
                         const int32_t* target_start, const int32_t* target_len, const int64_t* ws_offset,
                         const int32_t* row_len_host, const int32_t* target_len_host, int32_t* frames,
                         float* frame_logp, int32_t* spans, double* score, int32_t* status, int32_t lds_max_states,
                         int32_t flags, void* ws, size_t wsb, cfm_stream stream) {
  if (B < 0 || rows < 0 || n_targets < 0) return set_error(CFM_ERR_VALUE, "bad rows / B / n_targets");
  if (V < 1 || blank_id < 0 || blank_id >= V) return set_error(CFM_ERR_VALUE, "blank_id outside [0, V)");
  if (rows > (1 << 30) || n_targets > (1 << 29)) return set_error(CFM_ERR_VALUE, "rows / n_targets too large");
  if (B == 0) return CFM_OK;
  if ((rows > 0 && (!logp || !frames)) || (n_targets > 0 && !targets) || !row_start || !row_len || !target_start ||
      !target_len || !ws_offset || !row_len_host || !target_len_host || !score || !status || !ws)
    return set_error(CFM_ERR_VALUE, "null argument");
  if (wsb < cfm_ctc_align_plan(row_len_host, target_len_host, B, nullptr))
    return set_error(CFM_ERR_VALUE, "alignment workspace too small");
  int64_t max_runs = 1;
  for (int b = 0; b < B; ++b) {
    const int64_t r = al_runs(target_len_host[b] > 0 ? target_len_host[b] : 0);
    if (r > max_runs) max_runs = r;
  }
  AlignArgs a{};
  a.lp = logp; a.row_start = row_start; a.row_len = row_len; a.targets = targets; a.target_start = target_start;
  a.target_len = target_len; a.ws_off = ws_offset; a.frames = frames; a.spans = spans; a.status = status;
  a.end_state = (int32_t*)ws; a.frame_logp = frame_logp; a.score = score; a.ws = (char*)ws; a.ws_bytes = wsb;
  a.header_bytes = align_up((size_t)B * 4); a.rows = rows; a.V = V; a.blank = blank_id; a.n_targets = n_targets;
  a.lds_states = lds_max_states < 0 || lds_max_states > AL_LDS_STATES ? AL_LDS_STATES : lds_max_states;
  const int64_t lds_runs = std::min<int64_t>(max_runs, (a.lds_states + 15) / 16);
  a.lds_bytes = AL_LDS_HEAD + (a.lds_states > 0 ? (int)(2 * al_row_bytes(lds_runs)) : 0);
  const int64_t strips = (max_runs + AL_NT - 1) / AL_NT;
  const int nrun = (flags & CFM_ALIGN_GENERIC_STRIPS) || strips > AL_MAX_NRUN ? 0 : (int)std::max<int64_t>(strips, 1);
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto kern) -> hipError_t {
    if (a.lds_bytes > 64 * 1024) {
      const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(B), dim3(AL_NT), (size_t)a.lds_bytes, st, a);
    return hipGetLastError();
  };
  hipError_t e = nrun == 1 ? launch(ctc_align_trellis_kernel<1>)
               : nrun == 2 ? launch(ctc_align_trellis_kernel<2>)
               : nrun == 3 ? launch(ctc_align_trellis_kernel<3>)
                           : launch(ctc_align_trellis_kernel<0>);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(ctc_align_backtrace_kernel, dim3(B), dim3(64), 0, st, a);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return set_error(CFM_ERR_RUNTIME, std::string("ctc align: ") + hipGetErrorString(e));
  return CFM_OK;
}
