// The cfm_rnnt handle (csrc/rnnt.hip creates it): the predictor / joint weights on the device, shared by the greedy
// search (rnnt.hip) and the prefix beam search (rnnt_beam.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "../../include/cfm.h"

namespace cfm {

constexpr int RNNT_MAXL = 4;   // LSTM layers

struct RnntDev {
  const float* embed;                     // [V, E]
  const float* wg[RNNT_MAXL];             // [(in_l + H), 4H]: W_ih^T rows then W_hh^T rows
  const float* bg[RNNT_MAXL];             // [4H] b_ih + b_hh
  const float *wp, *bp;                   // [H, J], [J]: projection and pred_ffn composed (P = J)
  const float *wo, *bo;                   // [J, Vp] (zero-padded columns), [Vp] (padding -inf)
  int V, Vp, E, H, nl, P, J, blank;
  // the stateless predictors (kind != CFM_RNNT_PRED_RNN: H = nl = 0, P = E, wp / bp = pred_ffn [E, J], [J])
  int kind, Kc, act;                      // Kc = history_size + 1 ids of context
  float ln_eps, mix_div;                  // embedding: n_head * Kc
  const float* tap;                       // [Kc, E]: embedding q_c (pos_embed heads summed), conv the taps conv.weight[:, 0, c]
  const float* cbias;                     // [E] conv.bias or null
  const float *wf, *bf;                   // embedding: ffn [E, E] transposed, [E]
  const float *gamma, *beta;              // norm [E]
};

// the stateless predictors' activation (CFM_RNNT_ACT_*; gelu is torch's default erf form)
__device__ __forceinline__ float rnnt_act(int act, float v) {
  switch (act) {
    case CFM_RNNT_ACT_RELU: return v > 0.f ? v : 0.f;
    case CFM_RNNT_ACT_SWISH: return v / (1.f + expf(-v));
    case CFM_RNNT_ACT_TANH: return tanhf(v);
    default: return 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
  }
}

struct RnntGrid {
  const float4* wg[RNNT_MAXL];  // per layer, block-major [K_l][n_b] slices of gate quads (i, f, g, o of a unit)
  const float4* bg[RNNT_MAXL];  // [H] gate-quad biases (b_ih + b_hh)
  const float4 *wp, *wo;        // block-major slices of the composed projection + pred_ffn and ffn_out columns
  int G;
};

}  // namespace cfm

struct cfm_rnnt {
  cfm_rnnt_config cfg;
  int device = 0;
  void* dev_mem = nullptr;
  cfm::RnntDev w{};
  const float *we = nullptr, *be = nullptr;   // enc_ffn [J, Eenc] (torch layout), [J]
  // the grid path's block-major slices (built for grid_blocks workgroups per utterance)
  int grid_blocks = 32;                       // 0: always one workgroup per utterance
  int grid_lds = 1;                           // cache the grid path's weight slices in LDS when they fit
  int grid_atomic = 1;                        // exchanged vectors by agent-scope atomics, no cache-wide fences
  int grid_force_error = 0;                   // test hook: the grid search starts with its error word set
  int n_cu = 0;
  void* grid_mem = nullptr;
  cfm::RnntGrid gw{};
  std::vector<std::vector<float>> host_wg;    // [(in_l + H)][4H] transposed gate weights per layer
  std::vector<std::vector<float>> host_bg;    // [4H]
  std::vector<float> host_wp, host_wo;   // [H][J] (projection + pred_ffn composed), [J][Vp]
  // the beam search's GEMM operands in nn.Linear layout [N][K] (rnnt_beam.hip builds them on its first call, under
  // beam_mu, from the host copies above): per layer [4H][in_l + H], composed projection [J][H], ffn_out [V][J]
  std::mutex beam_mu;
  void* beam_mem = nullptr;
  const float* bw_g[cfm::RNNT_MAXL] = {};
  const float *bw_p = nullptr, *bw_o = nullptr;
  const float* bw_f = nullptr;                // stateless embedding predictor: ffn [E][E] (torch layout)
  std::vector<float> host_wf;                 // its transposed image [E][E]
  // the lattice kernel's bf16 operand (rnnt_lattice.hip builds it on its first bf16 call, under lat_mu, from host_wo):
  // ffn_out as two bf16 images [2][V][J], hi and lo = bf16(w - hi); the f32 kernel reads bw_o
  std::mutex lat_mu;
  void* lat_mem = nullptr;
  int lattice_dtype = CFM_DTYPE_F32;          // "lattice_dtype": operands of cfm_rnnt_td_score's joint (f32 or bf16)
  ~cfm_rnnt() {
    (void)hipSetDevice(device);
    if (dev_mem) (void)hipFree(dev_mem);
    if (grid_mem) (void)hipFree(grid_mem);
    if (beam_mem) (void)hipFree(beam_mem);
    if (lat_mem) (void)hipFree(lat_mem);
  }
};
