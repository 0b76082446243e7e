// The attention decoder handle (cfm_aed) shared by its two consumers: the n-best rescoring of aed.hip and the
// step-by-step beam search of attdec.hip.  One handle, one copy of the weights on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/cfm.h"
#include "cfm_common.h"
#include "cfm_kernels.h"
#include "status.h"

namespace cfm {

constexpr int AED_MAX_POS = 5000;   // PositionalEncoding max_len (embedding.py:22)

#define AED_KCHK(x)                                                                           \
  do {                                                                                        \
    int _e = (x);                                                                             \
    if (_e) return set_error(CFM_ERR_RUNTIME, std::string(#x ": ") + hipGetErrorString((hipError_t)_e)); \
  } while (0)

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

static inline size_t aed_align(size_t x) { return (x + 255) / 256 * 256; }

struct AedCarver {
  char* base;
  size_t off = 0;
  explicit AedCarver(void* b) : base((char*)b) {}
  template <typename U> U* take(size_t n) {
    U* p = (U*)(base ? base + off : nullptr);
    off += aed_align(n * sizeof(U));
    return p;
  }
};

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
