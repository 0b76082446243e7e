// Dispatch of the K = 512 weight-stationary GEMM (gemm_wst_impl.h) to its epilogue families, each
// instantiated in its own translation unit (gemm_wst_store / _silu / _qkv / _dw2.hip).
#include "gemm_wst_impl.h"

namespace cfm {

int wst_launch_store(int act, const bf16* A, int lda, const bf16* W, int ldw, int M, int N, const EpiArgs& ep,
                     hipStream_t st);
int wst_launch_silu(int act, const bf16* A, int lda, const bf16* W, int ldw, int M, int N, const EpiArgs& ep,
                    hipStream_t st);
int wst_launch_qkv_glu(int epi, int act, const bf16* A, int lda, const bf16* W, int ldw, int M, int N,
                       const EpiArgs& ep, hipStream_t st);
int wst_launch_dw2(const bf16* A, int lda, const bf16* W, int ldw, int M, int N, const EpiArgs& ep, hipStream_t st);

// -1 = not eligible (caller uses the 256 x 256 kernel)
int gemm_bf16_wst(int epi, int act, const bf16* A, int lda, const bf16* W, int ldw, int M, int N, int K,
                  const EpiArgs& ep, hipStream_t st) {
  if (!gemm_wst_eligible(epi, act, lda, ldw, M, N, K, ep)) return -1;   // cfm_kernels.h
  switch (epi) {
    case EPI_STORE:
      if (act == ACT_SILU || act == ACT_SILU_L2E) return wst_launch_silu(act, A, lda, W, ldw, M, N, ep, st);
      return wst_launch_store(act, A, lda, W, ldw, M, N, ep, st);
    case EPI_QKV: return wst_launch_qkv_glu(EPI_QKV, ACT_NONE, A, lda, W, ldw, M, N, ep, st);
    case EPI_GLU:
      return wst_launch_qkv_glu(EPI_GLU, act, A, lda, W, ldw, M, N, ep, st);
    case EPI_DW2:   // front-end pw1 + ReLU + dw2 (N = 512, dw2 taps / bias / geometry in ep; bf16 or f16)
      return wst_launch_dw2(A, lda, W, ldw, M, N, ep, st);
  }
  return -1;
}

}  // namespace cfm
