// Classification consumer (model: classification checkpoints): masked mean pool over time of the encoder
// output + the per-task linear heads with argmax / softmax, the reference's
// SpeechClassificationModel._average_pooling and classify (modules/classification_model.py:174-200,
// 232-281), on packed rows: utterance b = rows [row_start[b], row_start[b] + row_len[b]) of enc [rows, d].
//
// Three stream-ordered launches, no allocation, no host synchronisation, no floating-point atomics:
//   cls_scan_kernel    slab_off[b] = exclusive prefix sum of ceil(row_len[b] / CLS_SLAB)   (one workgroup)
//   cls_slab_kernel    workgroup j = slab (j - slab_off[u]) of utterance u (binary search in slab_off):
//                      column sums of its <= CLS_SLAB rows -> partial[j][d]
//   cls_finish_kernel  workgroup b: sum of its partials in slab order, / (row_len + 1e-10f) -> pooled;
//                      then logits = W . pooled + bias, per task argmax (lowest index on ties) and
//                      1 / sum exp(l - max)
// The slab grid is ceil(rows / CLS_SLAB) + B workgroups, an upper bound of the slab count of
// non-overlapping regions that the host knows without reading the length arrays; workgroups past the
// last slab exit.  Work is spread by rows, not by utterance, so one long utterance next to many short
// ones covers the device like a uniform batch.
//
// Summation order (fixed by d and the constants below alone, so a call is reproducible bit for bit):
// thread (g, c) of a 256-thread workgroup owns float4 column c and rows g, g + G, ... of the slab
// (G = 256 / (d / 4) row groups), added in ascending order; the G row-group sums are added in order
// g = 0 .. G - 1; the finish kernel adds the partials the same way.  Longest chain of f32 additions
// through one element: ceil(CLS_SLAB / G) + (G - 1) + ceil(P / G) + (G - 1), P = ceil(row_len / CLS_SLAB).
//
// Regions are clamped to [0, rows) on the device, so a bad length array cannot make a kernel read
// outside enc; rows outside every region are never loaded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cfm.h"
#include "cfm_common.h"
#include "status.h"
#include "workspace.h"

namespace cfm {

constexpr int CLS_SLAB = 64;        // rows per slab
constexpr int CLS_THREADS = 256;
constexpr int CLS_UNROLL = 8;       // independent 16-byte row loads in flight per thread
constexpr int CLS_MAX_TASKS = 16;
constexpr int CLS_MAX_CLASSES = 1024;
constexpr int CLS_MAX_TOTAL = 4096;

struct ClsHeads {
  const float* w;       // [sum_classes, d]
  const float* bias;    // [sum_classes]
  int n_tasks;          // 0: pooling only
  int off[CLS_MAX_TASKS + 1];
};

__device__ __forceinline__ void cls_region(const int* row_start, const int* row_len, int b, int rows, int& start,
                                           int& len) {
  int s = row_start[b], n = row_len[b];
  if (s < 0 || s > rows || n < 0) n = 0;
  if (n > rows - s) n = rows - s;
  start = s;
  len = n;
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// slab_off[0 .. B]: exclusive prefix sum of the utterances' slab counts, capped at `cap` slabs
__global__ __launch_bounds__(CLS_THREADS) void cls_scan_kernel(const int* __restrict__ row_start,
                                                               const int* __restrict__ row_len, int B, int rows,
                                                               int cap, int* __restrict__ slab_off) {
  __shared__ int part[CLS_THREADS];
  const int tid = threadIdx.x;
  const int per = (B + CLS_THREADS - 1) / CLS_THREADS;
  const int b0 = min(tid * per, B), b1 = min(b0 + per, B);
  int sum = 0;
  for (int b = b0; b < b1; ++b) {
    int s, n;
    cls_region(row_start, row_len, b, rows, s, n);
    sum += (n + CLS_SLAB - 1) / CLS_SLAB;
  }
  part[tid] = sum;
  __syncthreads();
  int base = 0;
  for (int t = 0; t < tid; ++t) base += part[t];
  for (int b = b0; b < b1; ++b) {
    int s, n;
    cls_region(row_start, row_len, b, rows, s, n);
    slab_off[b] = min(base, cap);
    base += (n + CLS_SLAB - 1) / CLS_SLAB;
  }
  if (tid == CLS_THREADS - 1) slab_off[B] = min(base, cap);
}

// column sums of rows r0, r0 + step, ... (< r0 + n * step) of src, ascending, CLS_UNROLL loads in flight
__device__ __forceinline__ float4 cls_column_sum(const float4* __restrict__ src, size_t stride, int first, int n,
                                                 int step) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int i = first;
  for (; i + (CLS_UNROLL - 1) * step < n; i += CLS_UNROLL * step) {
    float4 v[CLS_UNROLL];
#pragma unroll
    for (int u = 0; u < CLS_UNROLL; ++u) v[u] = src[(size_t)(i + u * step) * stride];
#pragma unroll
    for (int u = 0; u < CLS_UNROLL; ++u) acc = add4(acc, v[u]);
  }
  for (; i < n; i += step) acc = add4(acc, src[(size_t)i * stride]);
  return acc;
}

// the G row-group sums of column c, added in order g = 0 .. G - 1 (called by all threads; result valid for g == 0)
__device__ __forceinline__ float4 cls_group_sum(float4* sm, float4 acc, int g, int c, int G, int cols, bool active) {
  if (active) sm[g * cols + c] = acc;
  __syncthreads();
  float4 tot = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active && g == 0) {
    tot = sm[c];
    for (int k = 1; k < G; ++k) tot = add4(tot, sm[k * cols + c]);
  }
  return tot;
}

__global__ __launch_bounds__(CLS_THREADS) void cls_slab_kernel(const float* __restrict__ enc, int rows, int d,
                                                               const int* __restrict__ row_start,
                                                               const int* __restrict__ row_len, int B,
                                                               const int* __restrict__ slab_off,
                                                               float* __restrict__ partial) {
  __shared__ float4 sm[CLS_THREADS];
  const int j = blockIdx.x;
  if (j >= slab_off[B]) return;   // uniform: past the last slab
  int lo = 0, hi = B - 1;         // last u with slab_off[u] <= j (utterances without rows share an offset)
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (slab_off[mid] <= j) lo = mid; else hi = mid - 1;
  }
  const int u = lo;
  int start, len;
  cls_region(row_start, row_len, u, rows, start, len);
  const int s = j - slab_off[u];
  const int r0 = s * CLS_SLAB;
  const int n = min(CLS_SLAB, len - r0);   // >= 1 for a slab below slab_off[u + 1]
  const int cols = d >> 2;
  const int G = max(1, CLS_THREADS / cols);
  const int tid = threadIdx.x;
  const int g = tid / cols, c = tid - g * cols;
  const bool active = g < G;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active && n > 0)
    acc = cls_column_sum(reinterpret_cast<const float4*>(enc + (size_t)(start + r0) * d) + c, (size_t)cols, g, n, G);
  float4 tot = cls_group_sum(sm, acc, g, c, G, cols, active);
  if (active && g == 0) reinterpret_cast<float4*>(partial + (size_t)j * d)[c] = tot;
}

__global__ __launch_bounds__(CLS_THREADS) void cls_finish_kernel(int rows, int d, const int* __restrict__ row_start,
                                                                 const int* __restrict__ row_len,
                                                                 const int* __restrict__ slab_off,
                                                                 const float* __restrict__ partial, ClsHeads hd,
                                                                 float* __restrict__ pooled_out,
                                                                 float* __restrict__ logits_out,
                                                                 int* __restrict__ pred_out,
                                                                 float* __restrict__ prob_out) {
  __shared__ float4 sm[CLS_THREADS];
  __shared__ float4 pooled[CLS_THREADS];          // d <= 1024 floats
  __shared__ float logit[CLS_MAX_TOTAL];
  const int b = blockIdx.x;
  int start, len;
  cls_region(row_start, row_len, b, rows, start, len);
  const int p0 = slab_off[b];
  const int P = slab_off[b + 1] - p0;
  const int cols = d >> 2;
  const int G = max(1, CLS_THREADS / cols);
  const int tid = threadIdx.x;
  const int g = tid / cols, c = tid - g * cols;
  const bool active = g < G;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active && P > 0)
    acc = cls_column_sum(reinterpret_cast<const float4*>(partial + (size_t)p0 * d) + c, (size_t)cols, g, P, G);
  float4 tot = cls_group_sum(sm, acc, g, c, G, cols, active);
  if (active && g == 0) {
    const float den = (float)len + 1e-10f;   // classification_model.py:198
    tot = make_float4(tot.x / den, tot.y / den, tot.z / den, tot.w / den);
    pooled[c] = tot;
    if (pooled_out) reinterpret_cast<float4*>(pooled_out + (size_t)b * d)[c] = tot;
  }
  if (hd.n_tasks == 0) return;
  __syncthreads();
  const int S = hd.off[hd.n_tasks];
  const int wave = tid >> 6, lane = tid & 63;
  const float4* w4 = reinterpret_cast<const float4*>(hd.w);
  for (int k = wave; k < S; k += CLS_THREADS / 64) {
    float a = 0.f;
    for (int i = lane; i < cols; i += 64) {
      const float4 w = w4[(size_t)k * cols + i];
      const float4 p = pooled[i];
      a = fmaf(w.x, p.x, a);
      a = fmaf(w.y, p.y, a);
      a = fmaf(w.z, p.z, a);
      a = fmaf(w.w, p.w, a);
    }
    a = wave_sum(a) + hd.bias[k];
    if (lane == 0) {
      logit[k] = a;
      if (logits_out) logits_out[(size_t)b * S + k] = a;
    }
  }
  __syncthreads();
  for (int t = wave; t < hd.n_tasks; t += CLS_THREADS / 64) {
    const int o = hd.off[t], nc = hd.off[t + 1] - o;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int k = lane; k < nc; k += 64) {
      const float v = logit[o + k];
      if (v > best) { best = v; idx = k; }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const float ob = __shfl_xor(best, s, 64);
      const int oi = __shfl_xor(idx, s, 64);
      if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if (idx == 0x7fffffff) { idx = 0; best = logit[o]; }   // no finite-or-larger logit at all
    float e = 0.f;
    for (int k = lane; k < nc; k += 64) e += expf(logit[o + k] - best);
    e = wave_sum(e);
    if (lane == 0) {
      pred_out[(size_t)b * hd.n_tasks + t] = idx;
      prob_out[(size_t)b * hd.n_tasks + t] = 1.0f / e;   // exp(0) / sum exp(l - max)
    }
  }
}

static int cls_slab_cap(int rows, int B) { return (rows + CLS_SLAB - 1) / CLS_SLAB + B; }

static cfm_status cls_run(const float* enc, int rows, int d, const int* row_start, const int* row_len, int B,
                          const ClsHeads& hd, float* pooled, float* logits, int* pred, float* prob, void* ws, size_t wsb,
                          hipStream_t st) {
  if (rows < 0 || B < 0) return set_error(CFM_ERR_VALUE, "bad rows / B");
  if (d < 4 || d % 4 || d > 1024) return set_error(CFM_ERR_VALUE, "pooling width: a multiple of 4, 4 .. 1024");
  if (B == 0) return CFM_OK;
  if ((rows > 0 && !enc) || !row_start || !row_len || !ws) return set_error(CFM_ERR_VALUE, "null argument");
  if (hd.n_tasks == 0 && !pooled) return set_error(CFM_ERR_VALUE, "null argument");
  if (hd.n_tasks > 0 && (!pred || !prob)) return set_error(CFM_ERR_VALUE, "null argument");
  if (wsb < cfm_cls_pool_workspace_bytes(rows, d, B)) return set_error(CFM_ERR_VALUE, "classification workspace too small");
  if ((reinterpret_cast<uintptr_t>(enc) | reinterpret_cast<uintptr_t>(pooled) | reinterpret_cast<uintptr_t>(ws)) & 15)
    return set_error(CFM_ERR_VALUE, "enc / pooled / workspace must be 16-byte aligned");
  const int cap = cls_slab_cap(rows, B);
  int* slab_off = static_cast<int*>(ws);
  float* partial = reinterpret_cast<float*>(static_cast<char*>(ws) + align_up((size_t)(B + 1) * 4));
  hipLaunchKernelGGL(cls_scan_kernel, dim3(1), dim3(CLS_THREADS), 0, st, row_start, row_len, B, rows, cap, slab_off);
  hipLaunchKernelGGL(cls_slab_kernel, dim3(cap), dim3(CLS_THREADS), 0, st, enc, rows, d, row_start, row_len, B, slab_off,
                     partial);
  hipLaunchKernelGGL(cls_finish_kernel, dim3(B), dim3(CLS_THREADS), 0, st, rows, d, row_start, row_len, slab_off, partial,
                     hd, pooled, logits, pred, prob);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(CFM_ERR_RUNTIME, std::string("classification kernels: ") + hipGetErrorString(e));
  return CFM_OK;
}

}  // namespace cfm

struct cfm_cls {
  int device = 0;
  int d = 0;
  void* dev_mem = nullptr;
  cfm::ClsHeads hd{};
  ~cfm_cls() {
    (void)hipSetDevice(device);
    if (dev_mem) (void)hipFree(dev_mem);
  }
};

using namespace cfm;

extern "C" {

cfm_status cfm_cls_create(const cfm_cls_config* cfg, const cfm_tensor_view* weights, int32_t n, int32_t device,
                          cfm_cls** out) {
  if (!cfg || !out || !weights) return set_error(CFM_ERR_VALUE, "null argument");
  const int d = cfg->enc_dim, T = cfg->n_tasks;
  if (T < 1 || T > CLS_MAX_TASKS) return set_error(CFM_ERR_VALUE, "classification: 1 .. 16 tasks");
  if (d < 4 || d % 4 || d > 1024) return set_error(CFM_ERR_VALUE, "classification: enc_dim a multiple of 4, 4 .. 1024");
  auto h = std::make_unique<cfm_cls>();
  h->device = device;
  h->d = d;
  h->hd.n_tasks = T;
  int S = 0;
  for (int t = 0; t < T; ++t) {
    const int nc = cfg->num_classes[t];
    if (nc < 1 || nc > CLS_MAX_CLASSES) return set_error(CFM_ERR_VALUE, "classification: 1 .. 1024 classes per task");
    h->hd.off[t] = S;
    S += nc;
  }
  h->hd.off[T] = S;
  if (S > CLS_MAX_TOTAL) return set_error(CFM_ERR_VALUE, "classification: at most 4096 classes in total");
  if (n != 2 * T) return set_error(CFM_ERR_VALUE, "classification: expected a weight and a bias per task, in task order");
  const size_t w_elems = (size_t)S * d;
  std::vector<float> img(w_elems + S);
  for (int t = 0; t < T; ++t) {
    const cfm_tensor_view& w = weights[2 * t];
    const cfm_tensor_view& bv = weights[2 * t + 1];
    const int nc = cfg->num_classes[t];
    const std::string wn = w.name ? w.name : "?", bn = bv.name ? bv.name : "?";
    if (!w.data || w.numel != (int64_t)nc * d)
      return set_error(CFM_ERR_VALUE, "weight " + wn + ": expected " + std::to_string(nc) + " x " + std::to_string(d));
    if (!bv.data || bv.numel != nc) return set_error(CFM_ERR_VALUE, "weight " + bn + ": expected " + std::to_string(nc));
    std::copy(w.data, w.data + (size_t)nc * d, img.begin() + (size_t)h->hd.off[t] * d);
    std::copy(bv.data, bv.data + nc, img.begin() + w_elems + h->hd.off[t]);
  }
  if (hipSetDevice(device) != hipSuccess || hipMalloc(&h->dev_mem, img.size() * 4) != hipSuccess ||
      hipMemcpy(h->dev_mem, img.data(), img.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
    return set_error(CFM_ERR_RUNTIME, std::string("classification weights upload: ") + hipGetErrorString(hipGetLastError()));
  h->hd.w = static_cast<const float*>(h->dev_mem);
  h->hd.bias = h->hd.w + w_elems;
  *out = h.release();
  return CFM_OK;
}

void cfm_cls_destroy(cfm_cls* h) { delete h; }

size_t cfm_cls_pool_workspace_bytes(int32_t rows, int32_t d, int32_t B) {
  if (rows < 0 || B < 0 || d < 0) return 0;
  return align_up((size_t)(B + 1) * 4) + align_up((size_t)cls_slab_cap(rows, B) * d * 4);
}

size_t cfm_cls_workspace_bytes(const cfm_cls* h, int32_t rows, int32_t B) {
  return h ? cfm_cls_pool_workspace_bytes(rows, h->d, B) : 0;
}

cfm_status cfm_cls_pool(const float* enc, int32_t rows, int32_t d, const int32_t* row_start, const int32_t* row_len,
                        int32_t B, float* pooled, void* ws, size_t wsb, cfm_stream stream) {
  ClsHeads none{};
  return cls_run(enc, rows, d, row_start, row_len, B, none, pooled, nullptr, nullptr, nullptr, ws, wsb,
                 static_cast<hipStream_t>(stream));
}

cfm_status cfm_cls_classify(const cfm_cls* h, const float* enc, int32_t rows, const int32_t* row_start,
                            const int32_t* row_len, int32_t B, float* pooled, float* logits, int32_t* pred, float* prob,
                            void* ws, size_t wsb, cfm_stream stream) {
  if (!h) return set_error(CFM_ERR_VALUE, "null handle");
  if (hipSetDevice(h->device) != hipSuccess) return set_error(CFM_ERR_RUNTIME, "hipSetDevice");
  return cls_run(enc, rows, h->d, row_start, row_len, B, h->hd, pooled, logits, pred, prob, ws, wsb,
                 static_cast<hipStream_t>(stream));
}

}  // extern "C"
