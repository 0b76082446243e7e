// The 32-key MFMA tile of the decoder's attention kernels (bf16 / f16, head dim DK 64 / 128): seg_attn_mfma_kernel
// (aed.hip) and attdec_cross_mfma_kernel (attdec.hip) compute it the same way; an edit to one belongs in the other.
//
// Transposed: S^T = K . Q^T (keys on the MFMA row axis, the wave's 16 queries on the lanes' column axis), so a query's
// scores sit in one lane column (softmax reductions: 8 registers and two shuffles) and the probabilities are the B
// operand of O^T = V^T . P^T as they stand.  Their key order is a fixed permutation, contraction index
// 8 gq + e <-> key 16 (e / 4) + 4 gq + (e % 4) (gq = lane >> 4, e = 0 .. 7), which the V^T fragment read has to match:
// two 4-key reads at keys 4 gq and 16 + 4 gq of row (16 j + (lane & 15)).  The K rows and V^T of a tile are staged
// through LDS once for the workgroup: ks [32][KP], vt [DK][VP].
#pragma once

namespace cfm {

template <int DK>
struct AttnTile {
  static constexpr int KS = DK / 32;   // 32-deep steps of Q . K^T
  static constexpr int NJ = DK / 16;   // 16-dim tiles of the output
  static constexpr int KP = DK + 8;    // K pitch in elements (144 / 272 B: conflict-free 16-row fragment reads)
  static constexpr int VP = 40;        // V^T pitch in elements (80 B: 8-B aligned 4-key reads)
  static constexpr int CH = DK / 8;    // 16-B chunks per row
};

}  // namespace cfm
