// The attention decoder handle (cfm_aed) shared by its two consumers: the n-best rescoring of aed.hip and the
// step-by-step beam search of attdec.hip.  One handle, one copy of the weights on the device, and one decoder block:
// aed_decoder_blocks is the launch sequence of both, each consumer supplying its two attentions.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/cfm.h"
#include "cfm_common.h"
#include "cfm_kernels.h"
#include "status.h"
#include "workspace.h"

namespace cfm {

constexpr int AED_MAX_POS = 5000;   // PositionalEncoding max_len (embedding.py:22)

// LayerNorm of f32 rows of any width (the launcher of norm.hip takes 128 / 256 / 512): one wave per row, mean, then
// the mean of squared deviations, as ln_row does
template <typename T>
__global__ __launch_bounds__(256) void aed_ln_kernel(const float* __restrict__ x, int M, int d, const float* __restrict__ w,
                                                     const float* __restrict__ b, float eps, T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xp = x + (size_t)row * d;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += xp[c];
  const float mean = wave_sum(s) / d;
  float q = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float t = xp[c] - mean;
    q += t * t;
  }
  const float rstd = rsqrtf(wave_sum(q) / d + eps);
  for (int c = lane; c < d; c += 64) out[(size_t)row * d + c] = from_f32<T>((xp[c] - mean) * rstd * w[c] + b[c]);
}

template <typename T>
static int aed_layernorm(float* x, int M, int d, const float* w, const float* b, float eps, T* out, hipStream_t st) {
  if (M <= 0) return 0;
  if (d == 128 || d == 256 || d == 512) return layernorm<T>(x, ResidAdd<T>(), M, d, w, b, eps, out, nullptr, st);
  hipLaunchKernelGGL((aed_ln_kernel<T>), dim3((M + 3) / 4), dim3(256), 0, st, x, M, d, w, b, eps, out);
  CFM_CHECK_LAUNCH();
  return 0;
}

struct AedLayerW {
  void *wq_s, *wkv_s, *wo_s, *wq_c, *wkv_c, *wo_c, *w1, *w2;   // T matrices [N][K]
  float *bq_s, *bkv_s, *bo_s, *bq_c, *bkv_c, *bo_c, *b1, *b2;
  float *n1w, *n1b, *n2w, *n2b, *n3w, *n3b;
};
struct AedDecoderW {
  bool present = false;
  float* embed = nullptr;   // [V, d] f32
  float *an_w = nullptr, *an_b = nullptr, *out_b = nullptr;
  void* out_w = nullptr;    // [V, d] T
  std::vector<AedLayerW> layers;
};

// The decoder blocks of D and its after_norm on M rows (decoder_layer.py:67-149, normalize_before, dropout off):
// x [M, d] f32 is the residual stream, h, q, ao [M, d] and hid [M, ff] are T scratch; on return h = after_norm(x).
// Per block   LN1 -> Q GEMM -> self(l, L, h) -> out GEMM (+= x)
//             LN2 -> Q GEMM -> cross(l, L, q) -> out GEMM (+= x);  LN3 -> w_1 + ReLU GEMM -> w_2 GEMM (+= x)
// self projects K|V from h to where the consumer keeps them and attends q over them into ao; cross attends q over
// the memory's K|V of block l into ao.  Both return 0 or a hipError_t, as this does.
template <typename T, class SelfFn, class CrossFn>
static int aed_decoder_blocks(const AedDecoderW& D, const cfm_aed_config& cfg, int M, float* x, T* h, T* q, T* ao, T* hid,
                              SelfFn&& self, CrossFn&& cross, hipStream_t st) {
  const int d = cfg.d, ff = cfg.ff;
#define AED_TRY(X) do { if (const int _r = (X)) return _r; } while (0)
  int l = 0;
  for (const AedLayerW& L : D.layers) {
    // x += SelfAttn(LN1(x))
    AED_TRY(aed_layernorm<T>(x, M, d, L.n1w, L.n1b, cfg.eps, h, st));
    { EpiArgs e; e.bias = L.bq_s; e.out = q; e.ldo = d;
      AED_TRY(gemm<T>(EPI_STORE, ACT_NONE, h, d, (const T*)L.wq_s, d, M, d, d, e, st)); }
    AED_TRY(self(l, L, (const T*)h));
    { EpiArgs e; e.bias = L.bo_s; e.x = x; e.ldx = d;
      AED_TRY(gemm<T>(EPI_RESID, ACT_NONE, ao, d, (const T*)L.wo_s, d, M, d, d, e, st)); }
    // x += SrcAttn(LN2(x), memory)
    AED_TRY(aed_layernorm<T>(x, M, d, L.n2w, L.n2b, cfg.eps, h, st));
    { EpiArgs e; e.bias = L.bq_c; e.out = q; e.ldo = d;
      AED_TRY(gemm<T>(EPI_STORE, ACT_NONE, h, d, (const T*)L.wq_c, d, M, d, d, e, st)); }
    AED_TRY(cross(l, L, (const T*)q));
    { EpiArgs e; e.bias = L.bo_c; e.x = x; e.ldx = d;
      AED_TRY(gemm<T>(EPI_RESID, ACT_NONE, ao, d, (const T*)L.wo_c, d, M, d, d, e, st)); }
    // x += W2 ReLU(W1 LN3(x))
    AED_TRY(aed_layernorm<T>(x, M, d, L.n3w, L.n3b, cfg.eps, h, st));
    { EpiArgs e; e.bias = L.b1; e.out = hid; e.ldo = ff;
      AED_TRY(gemm<T>(EPI_STORE, ACT_RELU, h, d, (const T*)L.w1, d, M, ff, d, e, st)); }
    { EpiArgs e; e.bias = L.b2; e.x = x; e.ldx = d;
      AED_TRY(gemm<T>(EPI_RESID, ACT_NONE, hid, ff, (const T*)L.w2, ff, M, d, ff, e, st)); }
    ++l;
  }
  AED_TRY(aed_layernorm<T>(x, M, d, D.an_w, D.an_b, cfg.eps, h, st));
#undef AED_TRY
  return 0;
}

// K|V [rows, 2 d] of a block's cross-attention over the memory rows
template <typename T>
static int aed_memory_kv(const AedLayerW& L, const T* memT, int rows, int d, T* kv, hipStream_t st) {
  EpiArgs e; e.bias = L.bkv_c; e.out = kv; e.ldo = 2 * d;
  return gemm<T>(EPI_STORE, ACT_NONE, memT, d, (const T*)L.wkv_c, d, rows, 2 * d, d, e, st);
}

// the f32 memory rows as T: themselves, or converted into buf
template <typename T>
static int aed_memory_rows(const float* mem, int rows, int d, T* buf, hipStream_t st, const T** out) {
  if constexpr (sizeof(T) == 4) {
    *out = mem;
    return 0;
  } else {
    *out = buf;
    return att_cache_in<T>(mem, rows, d, buf, st);
  }
}

}  // namespace cfm

struct cfm_aed {
  cfm_aed_config cfg{};
  int device = 0;
  void* dev_mem = nullptr;
  float* pe = nullptr;   // [AED_MAX_POS, d] f32
  cfm::AedDecoderW dec[2];
  virtual ~cfm_aed() {
    if (dev_mem) { (void)hipSetDevice(device); (void)hipFree(dev_mem); }
  }
  virtual size_t ws_bytes(int tokens, int mem_rows) const = 0;
  virtual cfm_status score(const float* mem, int mem_rows, const int32_t* utt_start, const int32_t* utt_len, int B,
                           const int32_t* tokens, int n_tok, const int32_t* hyp_start, const int32_t* hyp_len,
                           const int32_t* hyp_utt, int n_hyps, int dirs, float* out_l2r, float* out_r2l, void* ws,
                           size_t wsb, hipStream_t st) const = 0;
};
