// Chunked relative-position multi-head self-attention over the overlapping-chunk
// KV stream (the "OCT" of attention.py:459-473).
//
// Reference: ChunkAttentionWithRelativeRightContext.forward_parallel_chunk
// (attention.py:420-505) with rel_shift (242-266) and forward_attention
// (104-150); the padded `forward` (268-418) uses the same kernel with other
// descriptors.  For block b (<= 64 queries of one head h):
//
//   s(i, j) = ((q_i + u_h) . k_j + (q_i + v_h) . P[P_BASE - i + j]) / sqrt(64)
//   keys j outside [KEY_LO, KEY_HI) are -inf, softmax in f32, out_i = sum_j p_ij v_j,
//   rows i >= Q_VALID are fully masked (reference: NaN -> 0) and written as 0.
//
// The rel_shift is never materialised: per 64-key tile each wave computes the
// 16 x 80 band Qv . P^T that its 16 query rows need (P rows P_BASE-i0-15+j0 ..
// +79), parks it in LDS and reads it back along the skewed diagonal.  Keys run
// in 64-key tiles with an online softmax; tiles entirely outside [KEY_LO,KEY_HI)
// are skipped (their probabilities are exactly 0 in the reference).  V^T tiles
// are staged in LDS (144/272-B pitch: conflict-free 16-row fragment reads).
#include <cstdlib>
#include "cfm_common.h"
#include "cfm_kernels.h"

namespace cfm {

template <typename T, int DK> struct AttnLds {
  static constexpr int VT_PITCH = 64 * sizeof(T) + 16;   // bytes per dim row of V^T (64 keys)
  static constexpr int P_PITCH = 64 * sizeof(T) + 16;    // bytes per query row of probabilities
  static constexpr int BD_PITCH = 85;                    // floats per row of the bd band
  static constexpr int VT_BYTES = DK * VT_PITCH;
  static constexpr int P_BYTES = 16 * P_PITCH;           // per wave
  static constexpr int BD_BYTES = 16 * BD_PITCH * 4;     // per wave
  static constexpr int TOTAL = VT_BYTES + 4 * (P_BYTES + BD_BYTES);
};

// DK = head dim (64: 8-head d=512 / 2-head d=128; 128: the 4-head d=512 recipes,
// examples/asr/rnnt/conf/chunkformer-rnnt-large-vie.yaml:5-6).  KV stream rows are
// [H][K dk | V dk]; P / pos_u / pos_v per head at h * DK.
template <typename T, int DK>
__global__ __launch_bounds__(256) void chunk_attention_kernel(
    const T* __restrict__ Q, const T* __restrict__ KV, int kv_rows, const T* __restrict__ P, int p_rows,
    const float* __restrict__ pos_u, const float* __restrict__ pos_v, const int32_t* __restrict__ desc, int H,
    T* __restrict__ out, int p_ld) {
  using LY = AttnLds<T, DK>;
  using FT = typename Frag<T>::type;
  constexpr int NS = DK / 32;   // 32-deep contraction sub-steps over the head dim
  constexpr int NO = DK / 16;   // 16-wide output n-blocks
  __shared__ __attribute__((aligned(16))) char smem[LY::TOTAL];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int h = blockIdx.y;
  const int32_t* D = desc + (size_t)blockIdx.x * AD_INTS;
  const int q_row0 = D[AD_Q_ROW0], nq = D[AD_NQ], kv_row0 = D[AD_KV_ROW0];
  const int key_lo = D[AD_KEY_LO], key_hi = D[AD_KEY_HI], p_base = D[AD_P_BASE], q_valid = D[AD_Q_VALID];
  const int d = H * DK;
  const int i0 = w * 16;

  char* vt = smem;
  char* pb = smem + LY::VT_BYTES + w * (LY::P_BYTES + LY::BD_BYTES);
  float* bd = reinterpret_cast<float*>(pb + LY::P_BYTES);

  // ---- query fragments (row i0 + fr), with u / v biases, NS 32-deep sub-steps over dk
  FT qu[NS], qv[NS];
  {
    const int qi = min(i0 + fr, nq - 1);
    const T* qp = Q + (size_t)(q_row0 + qi) * d + h * DK;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const FT raw = ld8<T>(qp + s * 32 + 8 * g);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int dd = s * 32 + 8 * g + e;
        const float qf = to_f32(raw[e]);
        qu[s][e] = from_f32<T>(qf + pos_u[h * DK + dd]);
        qv[s][e] = from_f32<T>(qf + pos_v[h * DK + dd]);
      }
    }
  }

  f32x4 O[NO];
  float m_r[4], l_r[4];
#pragma unroll
  for (int n = 0; n < NO; ++n) O[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_r[r] = -INFINITY; l_r[r] = 0.f; }

  const float scale = 1.0f / sqrtf((float)DK);
  for (int j0 = key_lo; j0 < key_hi; j0 += 64) {
    // ---- stage V^T of keys j0 .. j0+63 (each thread: one key, DK/4 dims)
    {
      constexpr int DQ = DK / 4;
      const int key = tid >> 2, dq = (tid & 3) * DQ;
      const int row = min(max(kv_row0 + j0 + key, 0), kv_rows - 1);
      const T* vp = KV + (size_t)row * (2 * d) + h * 2 * DK + DK + dq;
#pragma unroll
      for (int c8 = 0; c8 < DQ / 8; ++c8) {
        const FT v0 = ld8<T>(vp + 8 * c8);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          *reinterpret_cast<T*>(vt + (dq + 8 * c8 + e) * LY::VT_PITCH + key * sizeof(T)) = v0[e];
      }
    }
    // ---- ac = (q+u) K^T  (4 key sub-tiles of 16)
    f32x4 S[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int row = min(max(kv_row0 + j0 + n * 16 + fr, 0), kv_rows - 1);
      const T* kp = KV + (size_t)row * (2 * d) + h * 2 * DK;
      f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NS; ++s) a = mma16(qu[s], ld8<T>(kp + s * 32 + 8 * g), a);
      S[n] = a;
    }
    // ---- bd band = (q+v) P^T over rel-pos rows kb .. kb+79
    const int kb = p_base - i0 - 15 + j0;
#pragma unroll
    for (int n = 0; n < 5; ++n) {
      const int prow = min(max(kb + n * 16 + fr, 0), p_rows - 1);
      const T* pp = P + (size_t)prow * p_ld + h * DK;
      f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NS; ++s) a = mma16(qv[s], ld8<T>(pp + s * 32 + 8 * g), a);
#pragma unroll
      for (int r = 0; r < 4; ++r) bd[(4 * g + r) * LY::BD_PITCH + n * 16 + fr] = a[r];
    }
    __syncthreads();
    // ---- scores, mask, online softmax
    float mt[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * g + r;
      float mx = -INFINITY;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int jj = n * 16 + fr;
        float sv = (S[n][r] + bd[row * LY::BD_PITCH + jj + 15 - row]) * scale;
        if (j0 + jj >= key_hi) sv = -INFINITY;
        S[n][r] = sv;
        mx = fmaxf(mx, sv);
      }
      mt[r] = group16_max(mx);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mn = fmaxf(m_r[r], mt[r]);
      const float alpha = __expf(m_r[r] - mn);
      m_r[r] = mn;
      float rs = 0.f;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const float p = __expf(S[n][r] - mn);
        S[n][r] = p;
        rs += p;
      }
      l_r[r] = l_r[r] * alpha + group16_sum(rs);
#pragma unroll
      for (int n = 0; n < NO; ++n) O[n][r] *= alpha;
    }
    // ---- probabilities -> LDS (row-major [query][key]) -> A fragments
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<T*>(pb + (4 * g + r) * LY::P_PITCH + (n * 16 + fr) * sizeof(T)) = from_f32<T>(S[n][r]);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const FT pa = *reinterpret_cast<const FT*>(pb + fr * LY::P_PITCH + (s * 32 + 8 * g) * sizeof(T));
#pragma unroll
      for (int n = 0; n < NO; ++n) {
        const FT vb = *reinterpret_cast<const FT*>(vt + (n * 16 + fr) * LY::VT_PITCH + (s * 32 + 8 * g) * sizeof(T));
        O[n] = mma16(pa, vb, O[n]);
      }
    }
    __syncthreads();
  }

  // ---- normalise and store (head-merged layout [row][h*DK + dim])
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * g + r;
    if (i >= nq) continue;
    const bool live = (i < q_valid) && (l_r[r] > 0.f);
    const float inv = live ? 1.f / l_r[r] : 0.f;
    T* op = out + (size_t)(q_row0 + i) * d + h * DK;
#pragma unroll
    for (int n = 0; n < NO; ++n) op[n * 16 + fr] = from_f32<T>(O[n][r] * inv);
  }
}

template <typename T>
int chunk_attention(const T* q, const T* kv, int kv_rows, const T* P, int p_rows, const float* pos_u,
                    const float* pos_v, const int32_t* desc, int nblk, int H, int dk, T* out, hipStream_t st,
                    int p_ld) {
  if (nblk <= 0) return 0;
  if (p_ld <= 0) p_ld = H * dk;
  if (dk == 64)
    hipLaunchKernelGGL((chunk_attention_kernel<T, 64>), dim3(nblk, H), dim3(256), 0, st, q, kv, kv_rows, P, p_rows,
                       pos_u, pos_v, desc, H, out, p_ld);
  else if (dk == 128)
    hipLaunchKernelGGL((chunk_attention_kernel<T, 128>), dim3(nblk, H), dim3(256), 0, st, q, kv, kv_rows, P, p_rows,
                       pos_u, pos_v, desc, H, out, p_ld);
  else
    return (int)hipErrorInvalidValue;
  CFM_CHECK_LAUNCH();
  return 0;
}

template int chunk_attention<float>(const float*, const float*, int, const float*, int, const float*, const float*,
                                    const int32_t*, int, int, int, float*, hipStream_t, int);
template int chunk_attention<bf16>(const bf16*, const bf16*, int, const bf16*, int, const float*, const float*,
                                   const int32_t*, int, int, int, bf16*, hipStream_t, int);
template int chunk_attention<f16>(const f16*, const f16*, int, const f16*, int, const float*, const float*,
                                   const int32_t*, int, int, int, f16*, hipStream_t, int);



// =====================================================================================
// Fast path (bf16, masked batch): one block = one head x a run of NCH consecutive chunks.
//
// The packed chunk stream makes consecutive chunks' key windows overlap by W - C rows, so a
// block slides along the stream: K and V^T live in an LDS ring of 384 rows (the window of
// the current chunk plus the next chunk's C new rows, register-prefetched during compute),
// and the head's relative-position rows P (<= 383) are staged once per block.  Per wave (16
// queries) everything is computed TRANSPOSED (keys / P rows on the MFMA row axis, queries
// on lanes): S^T = K . (q+u)^T, band^T = P . (q+v)^T, then O^T = V^T . P^T uses the score
// registers directly as the B operand (their key order is a fixed permutation, matched by
// the V^T fragment), so probabilities never round-trip through LDS.  The rel_shift skew is
// a per-wave bf16 scratch write + diagonal read (reference: matrix_bd is bf16 under autocast).
// Softmax is exact (not online): all <= 320 scores of a query stay in registers.
// =====================================================================================
namespace {
constexpr int RING = 384;                       // ring rows (>= W + C)
constexpr int NCH = 8;                          // chunks per block
constexpr int KR_BYTES = RING * 128;            // K ring [384][64] bf16, 16-B chunks swizzled
constexpr int P_BYTES_ = RING * 128;            // P rows [384][64] bf16, swizzled
constexpr int VT_PITCH_B = (RING + 8) * 2;      // V^T [64 dims][384 (+8)] bf16
constexpr int VT_BYTES_ = 64 * VT_PITCH_B;
// bf16 per query row of the skew scratch (48-wide band, rows unsheared): a multiple of 4 (aligned ds_write_b64);
// 52 = 4 mod 8: the 16-lane write groups hit 32 distinct banks
constexpr int RD_PITCH = 52;
constexpr int SCR_ELEMS = 16 * RD_PITCH + 8;
constexpr int SCR_BYTES = (SCR_ELEMS * 2 + 15) / 16 * 16;   // per wave
constexpr int RING_LDS = KR_BYTES + P_BYTES_ + VT_BYTES_ + 8 * SCR_BYTES + 512;
}  // namespace

typedef unsigned u32x2_a __attribute__((ext_vector_type(2)));
CFM_DEV unsigned pack_bf16x2_a(float a, float b) {
  typedef bf16 b2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, (b2){(bf16)a, (bf16)b});
}
template <typename E>
CFM_DEV unsigned pack_e2(float a, float b) {
  typedef E e2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, (e2){(E)a, (E)b});
}
CFM_DEV int sw128(int row, int ch) { return row * 128 + ((ch ^ ((row >> 1) & 7)) << 4); }
// the two halves of an 8-wave block are SIMD partners running the same program (MI355X_MICROARCH.md,
// "Two waves per SIMD" item 4: a static priority for the arbitration loser): the second-dispatched half
// (waves 4-7) runs at s_setprio 1 (ring attention 4.82 -> 4.74 ms/step)
CFM_DEV void attn_static_prio(int half) {
  if (half) __builtin_amdgcn_s_setprio(1);
}

// rel_shift of one 32-key half (hh) of a 64-key tile through the wave's bf16 scratch (attention.py:242-266, the
// reference's pad / reshape trick): b[0..2] = band^T subtiles 2hh .. 2hh+2 (P rows kb0 + 16(2hh+pt) + 4g + rr,
// query fr); the result is the band of (query fr, keys j0 + 32hh + 16st2 + 4g .. +3) = band column
// 16st2 + 4g + rr + 15 - fr.  The rows are written unsheared (one aligned ds_write_b64 per subtile) and sheared
// on the read (ds_read2_b32 + ds_read_b32 per 4 values); the round-5 layout (sheared 2-B writes, pitch 49 / 48)
// spent a quarter of the kernel's LDS cycles in 2-way bank conflicts (PMC SQ_LDS_BANK_CONFLICT 25% of
// SQ_LDS_IDX_ACTIVE; a model of the banking: the b16 writes and the pitch-48 b64 reads are 2-way, pitch-52
// b64 writes conflict-free, the read-side shear's dword reads 2-way): 112 -> 72 LDS cycles per wave and tile.
// Query row fr lives in row slot skew_slot(fr) of the pitch-52 scratch.  With rows in query
// order the reads' first dwords (2 q(fr) + (15 - fr) / 2 for slot q(fr) in 8-B units) and those 2 banks on (g odd)
// collide pairwise in the 32-lane groups; a permutation whose slots keep q mod 16 distinct (the writes stay
// conflict-free) and make those 32 dwords distinct mod 32 removes the reads' conflicts: 72 -> 60 cycles per wave
// and tile in the model (the permutation is one solution of that search; any slot order keeps the layout valid)
CFM_DEV int skew_slot(int fr) {
  return (int)((0x9f35c268b17de4a0ull >> (4 * fr)) & 15u);
}
// The round trip is split in an issue and a finish, so the second half's trip through the scratch is in flight
// while the first half's score MFMAs run (the wait names their results, which pins them between the reads'
// issue and the wait)
struct SkewRd {
  u32x2_a d01[2];
  unsigned d2[2], sh[2];
};
template <typename E>
CFM_DEV void skew_issue(unsigned scr_base, int fr, int g, const f32x4* b, SkewRd& r) {
  const int srow = skew_slot(fr) * RD_PITCH;
#pragma unroll
  for (int pt = 0; pt < 3; ++pt) {
    const unsigned lo = pack_e2<E>(b[pt][0], b[pt][1]), hi = pack_e2<E>(b[pt][2], b[pt][3]);
    const unsigned waddr = scr_base + 2u * (unsigned)(srow + 16 * pt + 4 * g);
    asm volatile("ds_write_b64 %0, %1" ::"v"(waddr), "v"((u32x2_a){lo, hi}) : "memory");
  }
#pragma unroll
  for (int st2 = 0; st2 < 2; ++st2) {
    const unsigned ra = scr_base + 2u * (unsigned)(srow + 15 - fr + 16 * st2 + 4 * g);
    const unsigned al = ra & ~3u;
    r.sh[st2] = (ra & 2u) << 3;
    asm volatile("ds_read2_b32 %0, %1 offset0:0 offset1:1" : "=v"(r.d01[st2]) : "v"(al) : "memory");
    asm volatile("ds_read_b32 %0, %1 offset:8" : "=v"(r.d2[st2]) : "v"(al) : "memory");
  }
}
// bf16: the values straight into the f32 C operand -- v_perm_b32 puts an element's two bytes in the high half and
// zeros below (one VALU op per value instead of the funnel shift plus the bf16 -> f32 shift / mask); the byte
// offset sh / 8 is a lane constant (the parity of 15 - fr), so are the selectors
CFM_DEV void skew_finish_c(const SkewRd& r, f32x4 (&c)[2]) {
  const unsigned o = r.sh[0] >> 3;
  const unsigned s0 = 0x0c0cu | (o << 16) | ((o + 1) << 24);
  const unsigned s1 = s0 + 0x02020000u, s2 = s0 + 0x04040000u;
#pragma unroll
  for (int st2 = 0; st2 < 2; ++st2) {
    c[st2][0] = __builtin_bit_cast(float, __builtin_amdgcn_perm(r.d01[st2].y, r.d01[st2].x, s0));
    c[st2][1] = __builtin_bit_cast(float, __builtin_amdgcn_perm(r.d01[st2].y, r.d01[st2].x, s1));
    c[st2][2] = __builtin_bit_cast(float, __builtin_amdgcn_perm(r.d01[st2].y, r.d01[st2].x, s2));
    c[st2][3] = __builtin_bit_cast(float, __builtin_amdgcn_perm(r.d2[st2], r.d01[st2].y, s1));
  }
}
template <typename E>
CFM_DEV void skew_finish(const SkewRd& r, E (&bd)[2][4]) {
  typedef E ex4 __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int st2 = 0; st2 < 2; ++st2) {
    const ex4 v = __builtin_bit_cast(ex4, (u32x2_a){__builtin_amdgcn_alignbit(r.d01[st2].y, r.d01[st2].x, r.sh[st2]),
                                                   __builtin_amdgcn_alignbit(r.d2[st2], r.d01[st2].y, r.sh[st2])});
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) bd[st2][rr] = v[rr];
  }
}

// DG: the timing / A-B hooks of `diag` are compiled in (the production instantiation has none of their
// uniform branches inside the tile loop, which would cut it into basic blocks the scheduler cannot
// interleave across); NTI = W / 64 when W is whole 64-key tiles (1..5), else 0; V4 = next-pair staging in row
// quads (8-B V^T stores, half the store instructions; the launcher: W % 4 == 0), else in row pairs: the staged
// rows start at flat row c0 C + (cp - c0) C + W + C + 4k = W (mod 4), and a quad must not straddle the ring
// wrap (RING % 4 == 0) nor split an 8-B V^T store
template <bool DG, int NTI, typename E = bf16, bool V4 = true>
__global__ __launch_bounds__(512, 1) void chunk_attention_ring_kernel(
    const E* __restrict__ Q, const E* __restrict__ KV, int kv_rows, const E* __restrict__ P, int p_rows,
    const float* __restrict__ pos_u, const float* __restrict__ pos_v, const int32_t* __restrict__ desc, int n_chunks,
    int H, int C, int W, E* __restrict__ out, int diag_arg, int nch, int p_ld) {
  typedef E ex8 __attribute__((ext_vector_type(8)));   // bf16x8 / f16x8 fragments
  const int diag = DG ? diag_arg : 0;
  const bool reuse_band = (diag & 15) != 5;   // diag 5: recompute band subtile 0 of every tile (A/B)
  __shared__ __attribute__((aligned(16))) char smem[RING_LDS];
  char* kr = smem;
  char* pl = smem + KR_BYTES;
  char* vt = pl + P_BYTES_;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  // waves 0-3 work on chunk c, waves 4-7 on chunk c+1 (both windows live in the ring: W + C <= RING)
  const int half = __builtin_amdgcn_readfirstlane(w) >> 2, wq = w & 3;
  E* scr = reinterpret_cast<E*>(vt + VT_BYTES_ + w * SCR_BYTES);
  const unsigned scr_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)scr;
  float* uv = reinterpret_cast<float*>(vt + VT_BYTES_ + 8 * SCR_BYTES);   // [2][64]: pos_bias_u / v of head h
  const int h = blockIdx.y;
  const int d = H * 64;
  // balanced runs: block x of gridDim.x takes chunks [x n / gx, (x + 1) n / gx) of its head (nch unused)
  const int c0 = (int)((long long)blockIdx.x * n_chunks / gridDim.x),
            c1 = (int)((long long)(blockIdx.x + 1) * n_chunks / gridDim.x);
  if (c0 >= c1) return;

  // ---- zero the K / V^T rings (rows past a window's end are read as masked keys: p = 0 must not meet NaN)
  for (int idx = tid; idx < (KR_BYTES + P_BYTES_ + VT_BYTES_) / 16; idx += 512)
    reinterpret_cast<u32x4*>(smem)[idx] = (u32x4){0u, 0u, 0u, 0u};
  if (tid < 128) uv[tid] = (tid < 64 ? pos_u : pos_v)[h * 64 + (tid & 63)];
  __syncthreads();
  // ---- stage P rows and the first pair's windows (rows [kv0, kv0 + W + C))
  for (int idx = tid; idx < p_rows * 8; idx += 512) {
    const int r = idx >> 3, ch = idx & 7;
    *reinterpret_cast<u32x4*>(pl + sw128(r, ch)) = *reinterpret_cast<const u32x4*>(P + (size_t)r * p_ld + h * 64 + ch * 8);
  }
  // staging unit = two consecutive (even-aligned) flat rows x one 16-B chunk of K and V: the K halves
  // go to the swizzled K ring, the V halves are interleaved into 8 bf16x2 words of V^T (conflict-free:
  // the 64 lanes of a wave take 64 consecutive row pairs of one chunk)
  typedef E ex2_ __attribute__((ext_vector_type(2)));
  auto stage_pair = [&](int frow, int ch, const u32x4& k0, const u32x4& v0, const u32x4& k1, const u32x4& v1) {
    const int rr = frow % RING;   // even; rr + 1 < RING
    *reinterpret_cast<u32x4*>(kr + sw128(rr, ch)) = k0;
    *reinterpret_cast<u32x4*>(kr + sw128(rr + 1, ch)) = k1;
    const ex8 a = __builtin_bit_cast(ex8, v0), b = __builtin_bit_cast(ex8, v1);
#pragma unroll
    for (int e = 0; e < 8; ++e) *reinterpret_cast<ex2_*>(vt + (ch * 8 + e) * VT_PITCH_B + rr * 2) = (ex2_){a[e], b[e]};
  };
  // V4: four consecutive rows (frow % 4 == 0) x one 16-B chunk: each V^T dim row gets one 8-B store
  auto stage_quad = [&](int frow, int ch, const u32x4 (&k)[4], const u32x4 (&v)[4]) {
    const int rr = frow % RING;   // multiple of 4; rr + 3 < RING
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(kr + sw128(rr + i, ch)) = k[i];
    typedef E ex4_ __attribute__((ext_vector_type(4)));
    const ex8 a = __builtin_bit_cast(ex8, v[0]), b = __builtin_bit_cast(ex8, v[1]), c_ = __builtin_bit_cast(ex8, v[2]),
              d_ = __builtin_bit_cast(ex8, v[3]);
#pragma unroll
    for (int e = 0; e < 8; ++e) *reinterpret_cast<ex4_*>(vt + (ch * 8 + e) * VT_PITCH_B + rr * 2) = (ex4_){a[e], b[e], c_[e], d_[e]};
  };
  auto load_pair = [&](int frow, int ch, u32x4& k0, u32x4& v0, u32x4& k1, u32x4& v1) {
    const E* s0 = KV + (size_t)min(frow, kv_rows - 1) * (2 * d) + h * 128 + ch * 8;
    const E* s1 = KV + (size_t)min(frow + 1, kv_rows - 1) * (2 * d) + h * 128 + ch * 8;
    k0 = *reinterpret_cast<const u32x4*>(s0);
    v0 = *reinterpret_cast<const u32x4*>(s0 + 64);
    k1 = *reinterpret_cast<const u32x4*>(s1);
    v1 = *reinterpret_cast<const u32x4*>(s1 + 64);
  };
  const int kvb = desc[(size_t)c0 * AD_INTS + AD_KV_ROW0];   // chunk c's window starts at kvb + (c - c0) * C
  {
    const int npairs = (W + (c0 + 1 < c1 ? C : 0)) / 2;
    for (int idx = tid; idx < npairs * 8; idx += 512) {
      const int pr = idx % npairs, ch = idx / npairs;
      u32x4 k0, v0, k1, v1;
      load_pair(kvb + 2 * pr, ch, k0, v0, k1, v1);
      stage_pair(kvb + 2 * pr, ch, k0, v0, k1, v1);
    }
  }
  __syncthreads();

  const int i0 = wq * 16;
  attn_static_prio(half);
  // masked-batch descriptors (planner.cpp, C <= 64: one query block per chunk): chunk c's queries
  // are rows c*C.., its window starts at flat KV row c*C, P_BASE = C-1, every query row valid;
  // only the key range [lo, hi) varies.  Q fragments and the key range of the wave's NEXT chunk
  // are loaded one pair ahead, so no iteration waits on a dependent global load.
  const int p_base = C - 1, q_valid = C;
  auto load_q = [&](int c, ex8 (&qr)[2]) {
    const E* qp = Q + ((size_t)c * C + i0 + fr) * d + h * 64;
    qr[0] = *reinterpret_cast<const ex8*>(qp + 8 * g);
    qr[1] = *reinterpret_cast<const ex8*>(qp + 32 + 8 * g);
  };
  ex8 qraw[2], qnext[2];
  int klo_n = 0, khi_n = 0;
  {
    const int c = c0 + half;
    if (c < c1 && i0 < C) load_q(c, qnext);
    const int cc = min(c, c1 - 1);
    klo_n = desc[(size_t)cc * AD_INTS + AD_KEY_LO];
    khi_n = desc[(size_t)cc * AD_INTS + AD_KEY_HI];
  }
  // the output rows of a query group: O^T / l as E, dims 16nt + 4g .. of query row op
  auto store_out = [&](const f32x4 (&O)[4], float inv, E* op) {
    // dim pairs (16 nt .. +15, 16 (nt+1) ..): one permlane16 swap per packed dword leaves lane g with
    // 8 contiguous dims, so each query row leaves as two 64-B pieces (2 x 16-B stores per lane)
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const unsigned x0 = pack_e2<E>(O[2 * pr][0] * inv, O[2 * pr][1] * inv), x1 = pack_e2<E>(O[2 * pr][2] * inv, O[2 * pr][3] * inv);
      const unsigned y0 = pack_e2<E>(O[2 * pr + 1][0] * inv, O[2 * pr + 1][1] * inv),
                     y1 = pack_e2<E>(O[2 * pr + 1][2] * inv, O[2 * pr + 1][3] * inv);
      const auto r0 = __builtin_amdgcn_permlane16_swap(x0, y0, false, false);
      const auto r1 = __builtin_amdgcn_permlane16_swap(x1, y1, false, false);
      *reinterpret_cast<u32x4*>(op + 32 * pr + 16 * (g & 1) + 8 * (g >> 1)) = (u32x4){r0[0], r1[0], r0[1], r1[1]};
    }
  };
  for (int cp = c0; cp < c1; cp += 2) {
    const int kvp = kvb + (cp - c0) * C;
    const int c = cp + half;
    const bool active = c < c1 && i0 < C && (diag & 15) != 1;
    qraw[0] = qnext[0];
    qraw[1] = qnext[1];
    const int key_lo = klo_n, key_hi = khi_n;
    {
      const int cn = c + 2;
      if (cn < c1 && i0 < C) load_q(cn, qnext);
      const int cc = min(cn, c1 - 1);
      klo_n = desc[(size_t)cc * AD_INTS + AD_KEY_LO];
      khi_n = desc[(size_t)cc * AD_INTS + AD_KEY_HI];
    }
    // ---- prefetch the next pair's 2C new window rows [kvp + W + C, kvp + W + 3C) into registers
    // diag 6 / 7 (timing only, wrong results): no next-pair staging / and no barriers between pairs
    const int n_new = (diag & 15) >= 6 ? 0 : max(0, min(2 * C, (min(cp + 4, c1) - (cp + 2)) * C));
    const int pf_pairs = n_new / 2;
    u32x4 pk0[2], pv0[2], pk1[2], pv1[2];
    int pf_row[2], pf_ch[2];
    if constexpr (V4) {
      // quads: 2C / 4 <= 32 row quads x 8 chunks <= 256 items, one per thread of the first half
      const int pf_quads = n_new / 4;
      pf_row[0] = pf_row[1] = -1;
      if (pf_quads > 0 && tid < pf_quads * 8) {
        pf_ch[0] = tid / pf_quads;
        pf_row[0] = kvp + W + C + 4 * (tid % pf_quads);
        load_pair(pf_row[0], pf_ch[0], pk0[0], pv0[0], pk1[0], pv1[0]);
        load_pair(pf_row[0] + 2, pf_ch[0], pk0[1], pv0[1], pk1[1], pv1[1]);
      }
    } else {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = tid + 512 * q;
      pf_row[q] = -1;
      if (pf_pairs > 0 && idx < pf_pairs * 8) {
        pf_ch[q] = idx / pf_pairs;
        pf_row[q] = kvp + W + C + 2 * (idx % pf_pairs);
        load_pair(pf_row[q], pf_ch[q], pk0[q], pv0[q], pk1[q], pv1[q]);
      }
    }
    }
    if (active) {
      const int q_row0 = c * C;
      // Addresses split into a wave-uniform part and a lane constant: the window start rb, every
      // tile / subtile start and the band's P row base kb0 are multiples of 16 (C % 16 == 0), so a
      // 16-row subtile never straddles the ring wrap and the 16-B chunk swizzle of row base+fr is
      // (fr >> 1) & 7 for every subtile.  Out-of-range band rows (edge chunks only) read finite
      // LDS bytes whose products land in skew positions no valid (query, key) pair reads.
      const int rb = __builtin_amdgcn_readfirstlane((c * C) % RING);   // ring row of window key 0
      auto ring16 = [&](int j) { const int r = rb + j; return r >= RING ? r - RING : r; };   // j % 16 == 0
      const int key8 = (fr >> 1) & 7;
      const int frag_lane[2] = {fr * 128 + ((g ^ key8) << 4), fr * 128 + (((4 + g) ^ key8) << 4)};
      const int vt_lane = fr * VT_PITCH_B + 8 * g;
      // ---- query fragments (B operands): lane (fr, g) = query i0+fr, dims 32s + 8g .. +7
      ex8 qu[2], qv[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const f32x4 u0 = *reinterpret_cast<const f32x4*>(uv + s * 32 + 8 * g);
        const f32x4 u1 = *reinterpret_cast<const f32x4*>(uv + s * 32 + 8 * g + 4);
        const f32x4 v0_ = *reinterpret_cast<const f32x4*>(uv + 64 + s * 32 + 8 * g);
        const f32x4 v1_ = *reinterpret_cast<const f32x4*>(uv + 64 + s * 32 + 8 * g + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          // the 1/sqrt(dk) = 2^-3 scale is folded into both operands: exact in E and in the f32
          // accumulation, so (qu.k + bd) * 0.125 is reproduced bit for bit
          const float qf = (float)qraw[s][e];
          qu[s][e] = (E)((qf + (e < 4 ? u0[e] : u1[e - 4])) * 0.125f);
          qv[s][e] = (E)((qf + (e < 4 ? v0_[e] : v1_[e - 4])) * 0.125f);
        }
      }
      // interior chunks of a window that is whole 64-key tiles (key_lo = 0, key_hi = W = 64 NTI): no
      // per-score mask and no tile test -- the tile loop is one straight-line block; every other chunk
      // (utterance edges, W % 64 != 0) runs the masked copy (tiles from key_lo & ~15, skipped past key_hi)
      const bool whole = NTI > 0 && __builtin_amdgcn_readfirstlane(key_lo == 0 && key_hi == W) != 0;
      auto body = [&](auto MASKc) {
        constexpr bool MASK = decltype(MASKc)::value;
        constexpr int NTT = MASK ? 5 : (NTI > 0 ? NTI : 1);
        const int jb = MASK ? (key_lo & ~15) : 0;
        f32x4 S[NTT][4];
        f32x4 band_next = (f32x4){0.f, 0.f, 0.f, 0.f};
        float mx = -INFINITY;
        auto load_kf = [&](int t, ex8 (&kf)[4][2]) {
#pragma unroll
          for (int st = 0; st < 4; ++st) {
            const char* kb_ = kr + ring16(jb + 64 * t + 16 * st) * 128;
#pragma unroll
            for (int s = 0; s < 2; ++s) kf[st][s] = *reinterpret_cast<const ex8*>(kb_ + frag_lane[s]);
          }
        };
#pragma unroll
        for (int t = 0; t < NTT; ++t) {
          const int j0 = jb + 64 * t;
          if (MASK && j0 >= key_hi) {
#pragma unroll
            for (int st = 0; st < 4; ++st) S[t][st] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            continue;
          }
          // the band first: its skewed values (E, through the per-wave scratch) become the C
          // operand of the score MFMAs, so S = K.(q+u) + band costs no VALU add
          ex8 kf[4][2], pf[5][2];
          const int kb0 = p_base - i0 - 15 + j0;
          // band subtile 0 of tile t is subtile 4 of tile t - 1 (P rows kb0 .. kb0 + 15, 64 rows on):
          // carried in registers (tiles past key_hi are skipped only at the end, so tile t - 1 ran)
          const bool carry = t > 0 && reuse_band;
#pragma unroll
          for (int pt = 0; pt < 5; ++pt) {
            if (pt == 0 && carry) continue;
            const char* pb_ = pl + (kb0 + 16 * pt) * 128;
#pragma unroll
            for (int s = 0; s < 2; ++s) pf[pt][s] = *reinterpret_cast<const ex8*>(pb_ + frag_lane[s]);
          }
          load_kf(t, kf);
          // band^T[P row kb0 + 16pt + 4g + rr][query fr], pt = 0..4 (80 rows for 64 keys + 15 skew); the
          // two 32-key halves use subtiles 0-2 and 2-4 -> scratch[query][band pos] (16 x 48 E per wave)
          f32x4 band[5];
          // subtiles 3-4 (half 1 only) are computed while half 0's round trip is in flight
#pragma unroll
          for (int pt = 0; pt < 3; ++pt) {
            if (pt == 0 && carry) {
              band[0] = band_next;
              continue;
            }
            f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 2; ++s) a = mma16(pf[pt][s], qv[s], a);
            band[pt] = a;
          }
          SkewRd r0, r1;
          skew_issue<E>(scr_base, fr, g, band, r0);
          asm volatile("" : "+v"(qv[0]), "+v"(qv[1]));   // the MFMAs below read qv after the issue
#pragma unroll
          for (int pt = 3; pt < 5; ++pt) {
            f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 2; ++s) a = mma16(pf[pt][s], qv[s], a);
            band[pt] = a;
          }
          band_next = band[4];
          asm volatile("s_waitcnt lgkmcnt(0)"
                       : "+v"(r0.d01[0]), "+v"(r0.d01[1]), "+v"(r0.d2[0]), "+v"(r0.d2[1]), "+v"(band[3]), "+v"(band[4])::"memory");
          // the band as the f32 C operand of half hh's score MFMAs
          auto finish = [&](const SkewRd& r, f32x4 (&c)[2]) {
            if constexpr (std::is_same<E, bf16>::value) {
              skew_finish_c(r, c);
            } else {
              E bdv[2][4];
              skew_finish<E>(r, bdv);
#pragma unroll
              for (int st2 = 0; st2 < 2; ++st2)
                c[st2] = (f32x4){(float)bdv[st2][0], (float)bdv[st2][1], (float)bdv[st2][2], (float)bdv[st2][3]};
            }
          };
          // S^T[key 16st + 4g + rr][query fr] = band + K.(q+u)
          auto scores = [&](int hh, const f32x4 (&c)[2]) {
#pragma unroll
            for (int st2 = 0; st2 < 2; ++st2) {
              f32x4 a = c[st2];
#pragma unroll
              for (int s = 0; s < 2; ++s) a = mma16(kf[2 * hh + st2][s], qu[s], a);
              S[t][2 * hh + st2] = a;
            }
          };
          f32x4 c0[2], c1[2];
          finish(r0, c0);
          skew_issue<E>(scr_base, fr, g, band + 2, r1);   // the half-0 reads are complete: the rows may be reused
          scores(0, c0);
          asm volatile("s_waitcnt lgkmcnt(0)"
                       : "+v"(r1.d01[0]), "+v"(r1.d01[1]), "+v"(r1.d2[0]), "+v"(r1.d2[1]), "+v"(S[t][0]), "+v"(S[t][1])::"memory");
          finish(r1, c1);
          scores(1, c1);
          if constexpr (MASK) {
#pragma unroll
            for (int st = 0; st < 4; ++st)
#pragma unroll
              for (int rr = 0; rr < 4; ++rr) {
                const int j = j0 + 16 * st + 4 * g + rr;
                float sv = S[t][st][rr];
                if (j < key_lo || j >= key_hi) sv = -INFINITY;
                S[t][st][rr] = sv;
                mx = fmaxf(mx, sv);
              }
          } else {
#pragma unroll
            for (int st = 0; st < 4; ++st)
#pragma unroll
              for (int rr = 0; rr < 4; ++rr) mx = fmaxf(mx, S[t][st][rr]);
          }
        }
        // ---- exact softmax per query (lanes fr, fr+16, fr+32, fr+48 share a query)
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        if (mx == -INFINITY) mx = 0.f;   // fully masked query: every p = 0, output 0 (reference: NaN -> 0)
        const float mxl = mx * 1.4426950408889634f;
#pragma unroll
        for (int t = 0; t < NTT; ++t)
#pragma unroll
          for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) S[t][st][rr] = __builtin_amdgcn_exp2f(fmaf(S[t][st][rr], 1.4426950408889634f, -mxl));
        // ---- O^T[dim 16nt + 4g + rr][query fr] = sum_keys V^T . P^T (key order permuted, same for both);
        // the softmax denominator as a fifth MFMA against a constant "ones" row (row 0 of an A
        // fragment held in registers): l = sum over keys of the E p the numerator uses, and no
        // VALU add per score
        f32x4 O[4], Ol = (f32x4){0.f, 0.f, 0.f, 0.f};
        const E one_or_zero = (E)(fr == 0 ? 1.f : 0.f);
        const ex8 ones = (ex8){one_or_zero, one_or_zero, one_or_zero, one_or_zero,
                                     one_or_zero, one_or_zero, one_or_zero, one_or_zero};
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) O[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NTT; ++t) {
          const int j0 = jb + 64 * t;
          if ((MASK && j0 >= key_hi) || (diag & 15) == 3) continue;
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            ex8 pb;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              pb[rr] = (E)S[t][2 * s][rr];
              pb[4 + rr] = (E)S[t][2 * s + 1][rr];
            }
            const char* va_ = vt + vt_lane + ring16(j0 + 32 * s) * 2;
            const char* vb_ = vt + vt_lane + ring16(j0 + 32 * s + 16) * 2;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
              typedef E ex4 __attribute__((ext_vector_type(4)));
              const ex4 lo = *reinterpret_cast<const ex4*>(va_ + 16 * nt * VT_PITCH_B);
              const ex4 hi = *reinterpret_cast<const ex4*>(vb_ + 16 * nt * VT_PITCH_B);
              const ex8 va = (ex8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
              O[nt] = mma16(va, pb, O[nt]);
            }
            Ol = mma16(ones, pb, Ol);
          }
        }
        // row 0 of Ol^T (query fr) sits in register 0 of lane fr (g = 0)
        const float l = __shfl(Ol[0], fr, 64);
        const int qi = i0 + fr;
        const bool live = qi < q_valid && l > 0.f;
        const float inv = live ? 1.f / l : 0.f;
        E* op = out + (size_t)(q_row0 + qi) * d + h * 64;
        store_out(O, inv, op);
      };
      if (whole) body(std::false_type{});
      else body(std::true_type{});
    }
    // ---- the prefetched rows replace the first 2C rows of this pair's windows (no longer needed)
    if ((diag & 15) != 7) __syncthreads();
    if constexpr (V4) {
      if (pf_row[0] >= 0) {
        const u32x4 kq[4] = {pk0[0], pk1[0], pk0[1], pk1[1]}, vq[4] = {pv0[0], pv1[0], pv0[1], pv1[1]};
        stage_quad(pf_row[0], pf_ch[0], kq, vq);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (pf_row[q] >= 0) stage_pair(pf_row[q], pf_ch[q], pk0[q], pv0[q], pk1[q], pv1[q]);
    }
    if ((diag & 15) != 7) __syncthreads();
  }
}

// returns -1 when the shape is not eligible for the ring kernel
template <typename E>
int chunk_attention_masked_ring(const E* q, const E* kv, int kv_rows, const E* P, int p_rows,
                                const float* pos_u, const float* pos_v, const int32_t* desc, int n_chunks, int H,
                                int C, int W, E* out, hipStream_t st, int diag, int p_ld, int min_chunks) {
  if (p_ld <= 0) p_ld = H * 64;
  // W <= 320: a query's scores are 5 tiles of 64 keys held in registers (exact softmax)
  if (C <= 0 || C > 64 || (C % 16) || (W & 1) || W > 320 || W + C > RING || p_rows > RING || n_chunks <= 0) return -1;
  // one block per CU (LDS-bound), each sweeping a long run of chunks of one head: one prologue
  // (P rows + first window) per block instead of one per 8 chunks
  const int n_cu = cu_count();
  // one block per CU (CUs / H runs per head), each a balanced run of >= 2 chunks: a small launch (an
  // endless_decode segment at tbd 1800: 199 chunks) still fills every CU (was: runs of >= NCH chunks,
  // rounded to pairs -- 200 blocks on 256 CUs there)
  const int gx = max(1, min(n_cu / max(H, 1), n_chunks / max(2, min_chunks)));
  const int nch = (n_chunks + gx - 1) / gx;
  const dim3 grid(gx, H);
#define RING_L(DG_, NT_)                                                                                             \
  hipLaunchKernelGGL((chunk_attention_ring_kernel<DG_, NT_, E, true>), grid, dim3(512), 0, st, q, kv, kv_rows, P, p_rows, pos_u, \
                     pos_v, desc, n_chunks, H, C, W, out, diag, nch, p_ld)
#define RING_P(DG_)                                                                                                   \
  hipLaunchKernelGGL((chunk_attention_ring_kernel<DG_, 0, E, false>), grid, dim3(512), 0, st, q, kv, kv_rows, P, p_rows, \
                     pos_u, pos_v, desc, n_chunks, H, C, W, out, diag, nch, p_ld)
  const int nti = W % 64 == 0 ? W / 64 : 0;
  if (W % 4) {   // W % 4 == 2 (never whole 64-key tiles): pair staging
    if (diag) RING_P(true);
    else RING_P(false);
  }
  else if (diag) {
    if (nti == 5) RING_L(true, 5);
    else RING_L(true, 0);
  }
  else if (nti == 5) RING_L(false, 5);
  else if (nti == 4) RING_L(false, 4);
  else if (nti == 3) RING_L(false, 3);
  else if (nti == 2) RING_L(false, 2);
  else if (nti == 1) RING_L(false, 1);
  else RING_L(false, 0);
#undef RING_L
#undef RING_P
  CFM_CHECK_LAUNCH();
  return 0;
}
int chunk_attention_masked_bf16(const bf16* q, const bf16* kv, int kv_rows, const bf16* P, int p_rows,
                                const float* pos_u, const float* pos_v, const int32_t* desc, int n_chunks, int H,
                                int C, int W, bf16* out, hipStream_t st, int diag, int p_ld, int min_chunks) {
  return chunk_attention_masked_ring<bf16>(q, kv, kv_rows, P, p_rows, pos_u, pos_v, desc, n_chunks, H, C, W, out, st,
                                           diag, p_ld, min_chunks);
}
int chunk_attention_masked_f16(const f16* q, const f16* kv, int kv_rows, const f16* P, int p_rows,
                               const float* pos_u, const float* pos_v, const int32_t* desc, int n_chunks, int H,
                               int C, int W, f16* out, hipStream_t st, int diag, int p_ld, int min_chunks) {
  return chunk_attention_masked_ring<f16>(q, kv, kv_rows, P, p_rows, pos_u, pos_v, desc, n_chunks, H, C, W, out, st,
                                          diag, p_ld, min_chunks);
}


// =====================================================================================
// Dense path (bf16, dk 64, full attention: forward_encoder with chunk_size -1, BASELINE configs[4];
// any padded plan without left context): one 512-thread block = one utterance x one head (8 waves, two
// per SIMD), every key of the utterance (T' <= 384) staged in LDS for all 8 waves instead of each wave
// reloading K and P fragments from global memory per 64-key tile (chunk_attention_kernel).  Round 6: the
// block runs the utterance's query pairs (two 64-query descriptors, one per half of the block) as passes
// over ONE prologue -- the relative-position rows of every pass (64 NT + 127 + 128 per further pair) by
// LDS-DMA, the K and V rows into registers, where they stay for all passes -- instead of one block (and
// one HBM-bound prologue of 160 KB) per pair; per pass:
//   K rows (swizzled) from the registers into the K / V^T region;
//   scores:  the ring kernel's compute -- S^T = K.(q+u)^T, band^T = P.(q+v)^T skewed through a bf16
//            scratch (skew_issue / skew_finish_c), exact softmax with all <= 384 scores of a query in registers;
//   V^T from the registers over the dead K region, then O^T = V^T.P^T with the score registers as
//            the B operand.
// LDS: max(K 48 KiB, V^T 49 KiB) + P 96 KiB + 8 skew scratches = 159 KiB.
// =====================================================================================
namespace {
constexpr int FA_KEYS = 384;                        // keys staged (T' <= 384: utterances <= 30.8 s)
constexpr int FA_NT = FA_KEYS / 64;                 // key tiles
constexpr int FA_PROWS = 64 * FA_NT + 128;          // P rows staged (64 NT + 127, rounded)
constexpr int FA_K_BYTES = FA_KEYS * 128;
constexpr int FA_VT_PITCH = (FA_KEYS + 8) * 2;
constexpr int FA_VT_BYTES = 64 * FA_VT_PITCH;
constexpr int FA_KV_BYTES = FA_VT_BYTES > FA_K_BYTES ? FA_VT_BYTES : FA_K_BYTES;
constexpr int FA_MAXPAIR = (FA_NT + 1) / 2;                      // query pairs of a T' <= 384 utterance
constexpr int FA_PROWS_ALL = FA_PROWS + 128 * (FA_MAXPAIR - 1);   // P rows of every pass (768)
constexpr int FA_P_BYTES = FA_PROWS_ALL * 128;
constexpr int FA_LDS = FA_KV_BYTES + FA_P_BYTES + 8 * SCR_BYTES + 512;
static_assert(FA_LDS <= 163840, "full-attention LDS");
static_assert(RING_LDS <= 163840, "ring-attention LDS");
}  // namespace

__global__ __launch_bounds__(512, 1) void full_attention_bf16_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ KV, int kv_rows, const bf16* __restrict__ P, int p_rows,
    const float* __restrict__ pos_u, const float* __restrict__ pos_v, const int32_t* __restrict__ desc, int H,
    int nd, bf16* __restrict__ out, int p_ld) {
  __shared__ __attribute__((aligned(16))) char smem[FA_LDS];
  char* kr = smem;   // K in phase 1, V^T in phase 2
  char* vt = smem;
  char* pl = smem + FA_KV_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int half = __builtin_amdgcn_readfirstlane(w) >> 2, wq = w & 3;
  bf16* scr = reinterpret_cast<bf16*>(pl + FA_P_BYTES + w * SCR_BYTES);
  const unsigned scr_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)scr;
  float* uv = reinterpret_cast<float*>(pl + FA_P_BYTES + 8 * SCR_BYTES);
  // XCD-aware order: the dispatcher deals consecutive workgroups round-robin to the 8 XCDs, so the
  // hardware index is remapped (bijectively) to give each XCD a contiguous run of (head, utterance)
  // items: the utterances of one head -- which stage the same P rows -- share that XCD's L2
  const int nutt = gridDim.x;
  const int T = nutt * gridDim.y, b = blockIdx.y * nutt + blockIdx.x, xcd = b & 7, q8 = T >> 3, r8 = T & 7;
  const int item = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b >> 3);
  const int h = item / nutt, u = item - h * nutt, d = H * 64;
  const int npair = (nd + 1) >> 1;
  const int32_t* Du = desc + (size_t)u * nd * AD_INTS;
  const int kv_row0 = Du[AD_KV_ROW0], key_hi = Du[AD_KEY_HI];   // shared by the utterance's descriptors
  // P_BASE of descriptor k is T' - 1 - 64 k (planner.cpp): the last pair's rows start lowest
  const int pb0 = Du[(size_t)(2 * (npair - 1)) * AD_INTS + AD_P_BASE] - 127;   // P row of LDS row 0

  // ---- prologue: the P rows pb0 .. of every pass straight into LDS by LDS-DMA (wave w, instruction i
  // fills rows 8 (8 i + w) .. +7 lane-linearly, the row's 16-B chunk swizzle applied on the source
  // address; rows outside [0, p_rows) are clamped: they reach masked scores only), then every global
  // load of the thread (K and V, kept in registers for all passes)
  const int p_iters = (FA_PROWS + 128 * (npair - 1)) / 64;
  for (int i = 0; i < p_iters; ++i) {
    const int r = 8 * (8 * i + w) + (lane >> 3), ch = (lane & 7) ^ ((r >> 1) & 7);
    const int prow = min(max(pb0 + r, 0), p_rows - 1);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(P + (size_t)prow * p_ld + h * 64 + ch * 8),
                                     (__attribute__((address_space(3))) void*)(pl + 8 * (8 * i + w) * 128), 16, 0, 0);
  }
  if (tid < 128) uv[tid] = (tid < 64 ? pos_u : pos_v)[h * 64 + (tid & 63)];
  constexpr int KIT = FA_KEYS * 8 / 512, VIT = (FA_KEYS / 2) * 8 / 512;
  static_assert(FA_KEYS * 8 % 512 == 0 && FA_PROWS % 64 == 0 && (FA_KEYS / 2) * 8 % 512 == 0, "staging");
  static_assert(FA_LDS <= 163840, "full-attention LDS");
  u32x4 sk[KIT], sv0[VIT], sv1[VIT];
  const u32x4 z4 = (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
  for (int it = 0; it < VIT; ++it) {   // V rows: two keys x one 16-B chunk (zero past key_hi: p = 0 x finite)
    const int idx = tid + 512 * it, pr = idx % (FA_KEYS / 2), ch = idx / (FA_KEYS / 2), j = 2 * pr;
    sv0[it] = j < key_hi ? *reinterpret_cast<const u32x4*>(KV + (size_t)min(kv_row0 + j, kv_rows - 1) * (2 * d) +
                                                            h * 128 + 64 + ch * 8)
                         : z4;
    sv1[it] = j + 1 < key_hi ? *reinterpret_cast<const u32x4*>(KV + (size_t)min(kv_row0 + j + 1, kv_rows - 1) * (2 * d) +
                                                                h * 128 + 64 + ch * 8)
                             : z4;
  }
#pragma unroll
  for (int it = 0; it < KIT; ++it) {   // K rows: one 16-B chunk (8 lanes per row: conflict-free stores)
    const int idx = tid + 512 * it, j = idx >> 3, ch = idx & 7;
    sk[it] = j < key_hi ? *reinterpret_cast<const u32x4*>(KV + (size_t)min(kv_row0 + j, kv_rows - 1) * (2 * d) +
                                                           h * 128 + ch * 8)
                        : z4;
  }

  const int i0 = wq * 16;
  attn_static_prio(half);
  // the block's key tiles (one utterance: uniform), as a compile-time count: the tile loops are
  // straight-line code without per-tile skip branches; only the last tile can need the key mask
  const int ntv = __builtin_amdgcn_readfirstlane((key_hi + 63) >> 6);
  auto body = [&](auto NTVc) {
    constexpr int NTV = decltype(NTVc)::value;
    const int key8 = (fr >> 1) & 7;
    const int frag_lane[2] = {fr * 128 + ((g ^ key8) << 4), fr * 128 + (((4 + g) ^ key8) << 4)};
    for (int pr2 = 0; pr2 < npair; ++pr2) {
    const int dix = u * nd + 2 * pr2 + half;
    const bool has = 2 * pr2 + half < nd;
    const int32_t* D = desc + (size_t)(has ? dix : u * nd + 2 * pr2) * AD_INTS;
    const int q_row0 = D[AD_Q_ROW0], nq = D[AD_NQ], p_base = D[AD_P_BASE], q_valid = D[AD_Q_VALID];
    const bool active = has && i0 < nq;
    // K rows into the K / V^T region (the previous pass's P.V reads of it are behind the pass-end barrier)
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int idx = tid + 512 * it;
      *reinterpret_cast<u32x4*>(kr + sw128(idx >> 3, idx & 7)) = sk[it];
    }
    if (pr2 == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the P rows (LDS-DMA) have landed
    __syncthreads();
    f32x4 S[NTV][4];
    float l = 0.f;
    if (active) {
      bf16x8 qraw[2];
      {
        const bf16* qp = Q + ((size_t)q_row0 + min(i0 + fr, nq - 1)) * d + h * 64;
        qraw[0] = *reinterpret_cast<const bf16x8*>(qp + 8 * g);
        qraw[1] = *reinterpret_cast<const bf16x8*>(qp + 32 + 8 * g);
      }
      bf16x8 qu[2], qv[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const f32x4 u0 = *reinterpret_cast<const f32x4*>(uv + s * 32 + 8 * g);
        const f32x4 u1 = *reinterpret_cast<const f32x4*>(uv + s * 32 + 8 * g + 4);
        const f32x4 v0_ = *reinterpret_cast<const f32x4*>(uv + 64 + s * 32 + 8 * g);
        const f32x4 v1_ = *reinterpret_cast<const f32x4*>(uv + 64 + s * 32 + 8 * g + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float qf = (float)qraw[s][e];   // 1/sqrt(64) = 2^-3 folded in: exact in bf16 and f32
          qu[s][e] = (bf16)((qf + (e < 4 ? u0[e] : u1[e - 4])) * 0.125f);
          qv[s][e] = (bf16)((qf + (e < 4 ? v0_[e] : v1_[e - 4])) * 0.125f);
        }
      }
      f32x4 band_next = (f32x4){0.f, 0.f, 0.f, 0.f};
      float mx = -INFINITY;
      // band rows kb0 = p_base - i0 - 15 + j0 .. +79 -> LDS row kb0 - pb0
      const int lbase = p_base - i0 - 15 - pb0;
#pragma unroll
      for (int t = 0; t < NTV; ++t) {
        const int j0 = 64 * t;
        // the band first; its skewed values are the C operand of the score MFMAs (no VALU add)
        f32x4 band[5];
        const bool tmask = t == NTV - 1 && j0 + 64 > key_hi;   // only the last valid tile can be partial
        auto band_pt = [&](int pt) {
          f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < 2; ++s)
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                *reinterpret_cast<const bf16x8*>(pl + (lbase + j0 + 16 * pt) * 128 + frag_lane[s]), qv[s], a, 0, 0, 0);
          band[pt] = a;
        };
        // S^T[key 16st + 4g + rr][query fr] = band + K.(q+u), masked past key_hi
        auto score_st = [&](int st, const f32x4& c, const bf16x8 (&kf)[2]) {
          f32x4 a = c;
#pragma unroll
          for (int s = 0; s < 2; ++s) a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[s], qu[s], a, 0, 0, 0);
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            float sv = a[rr];
            if (tmask && j0 + 16 * st + 4 * g + rr >= key_hi) sv = -INFINITY;
            S[t][st][rr] = sv;
            mx = fmaxf(mx, sv);
          }
        };
        auto kfrag = [&](int st, bf16x8 (&kf)[2]) {
#pragma unroll
          for (int s = 0; s < 2; ++s) kf[s] = *reinterpret_cast<const bf16x8*>(kr + (j0 + 16 * st) * 128 + frag_lane[s]);
        };
#pragma unroll
        for (int pt = 0; pt < 5; ++pt) {
          if (pt == 0 && t > 0) band[0] = band_next;   // subtile 0 of this tile is subtile 4 of the previous one
          else band_pt(pt);
        }
        band_next = band[4];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          f32x4 c[2];
          SkewRd r;   // the band straight into the C operand (v_perm_b32)
          skew_issue<bf16>(scr_base, fr, g, band + 2 * hh, r);
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r.d01[0]), "+v"(r.d01[1]), "+v"(r.d2[0]), "+v"(r.d2[1])::"memory");
          skew_finish_c(r, c);
#pragma unroll
          for (int st2 = 0; st2 < 2; ++st2) {
            bf16x8 kf[2];
            kfrag(2 * hh + st2, kf);
            score_st(2 * hh + st2, c[st2], kf);
          }
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      if (mx == -INFINITY) mx = 0.f;   // no valid key: every p = 0, output 0
      const float mxl = mx * 1.4426950408889634f;
#pragma unroll
      for (int t = 0; t < NTV; ++t)
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const float p = __builtin_amdgcn_exp2f(fmaf(S[t][st][rr], 1.4426950408889634f, -mxl));
            S[t][st][rr] = p;
            l += p;
          }
      l += __shfl_xor(l, 16, 64);
      l += __shfl_xor(l, 32, 64);
    }
    // ---- phase 2: V^T over the K region (every wave is past its K reads)
    __syncthreads();
    typedef bf16 bf16x2_ __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
      const int idx = tid + 512 * it, pr = idx % (FA_KEYS / 2), ch = idx / (FA_KEYS / 2), j = 2 * pr;
      const bf16x8 a = __builtin_bit_cast(bf16x8, sv0[it]), b = __builtin_bit_cast(bf16x8, sv1[it]);
#pragma unroll
      for (int e = 0; e < 8; ++e) *reinterpret_cast<bf16x2_*>(vt + (ch * 8 + e) * FA_VT_PITCH + j * 2) = (bf16x2_){a[e], b[e]};
    }
    __syncthreads();
    if (active) {
    const int vt_lane = fr * FA_VT_PITCH + 8 * g;
    f32x4 O[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) O[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NTV; ++t) {
      const int j0 = 64 * t;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 pb;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          pb[rr] = (bf16)S[t][2 * s][rr];
          pb[4 + rr] = (bf16)S[t][2 * s + 1][rr];
        }
        const char* va_ = vt + vt_lane + (j0 + 32 * s) * 2;
        const char* vb_ = vt + vt_lane + (j0 + 32 * s + 16) * 2;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));
          const bf16x4 lo = *reinterpret_cast<const bf16x4*>(va_ + 16 * nt * FA_VT_PITCH);
          const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vb_ + 16 * nt * FA_VT_PITCH);
          const bf16x8 va = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          O[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, O[nt], 0, 0, 0);
        }
      }
    }
    const int qi = i0 + fr;
    const bool live = qi < q_valid && l > 0.f;
    const float inv = live ? 1.f / l : 0.f;
    bf16* op = out + ((size_t)q_row0 + qi) * d + h * 64;
    // as the ring kernel: 16-B stores after permlane16 swaps (every lane takes part in the swaps)
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const unsigned x0 = pack_bf16x2_a(O[2 * pr][0] * inv, O[2 * pr][1] * inv), x1 = pack_bf16x2_a(O[2 * pr][2] * inv, O[2 * pr][3] * inv);
      const unsigned y0 = pack_bf16x2_a(O[2 * pr + 1][0] * inv, O[2 * pr + 1][1] * inv),
                     y1 = pack_bf16x2_a(O[2 * pr + 1][2] * inv, O[2 * pr + 1][3] * inv);
      const auto r0 = __builtin_amdgcn_permlane16_swap(x0, y0, false, false);
      const auto r1 = __builtin_amdgcn_permlane16_swap(x1, y1, false, false);
      if (qi < nq) *reinterpret_cast<u32x4*>(op + 32 * pr + 16 * (g & 1) + 8 * (g >> 1)) = (u32x4){r0[0], r1[0], r0[1], r1[1]};
    }
    }   // active
    __syncthreads();   // every wave is past its V^T reads before the next pass writes K there
    }   // passes
  };
  switch (ntv) {
    case 0:   // (no key: tile 0 fully masked, output 0)
    case 1: body(std::integral_constant<int, 1>{}); break;
    case 2: body(std::integral_constant<int, 2>{}); break;
    case 3: body(std::integral_constant<int, 3>{}); break;
    case 4: body(std::integral_constant<int, 4>{}); break;
    case 5: body(std::integral_constant<int, 5>{}); break;
    default: body(std::integral_constant<int, FA_NT>{}); break;
  }
}

// -1 when not eligible (T' > 384, dk != 64): the caller uses chunk_attention_kernel.  `nd` = the
// plan's 64-query descriptors per utterance (consecutive), `nutt` utterances.
int full_attention_bf16(const bf16* q, const bf16* kv, int kv_rows, const bf16* P, int p_rows, const float* pos_u,
                        const float* pos_v, const int32_t* desc, int nutt, int nd, int H, int dk, int t_keys,
                        bf16* out, hipStream_t st, int p_ld) {
  if (nutt <= 0 || nd <= 0) return 0;
  if (dk != 64 || t_keys > FA_KEYS || t_keys <= 0) return -1;
  if (p_ld <= 0) p_ld = H * 64;
  if ((nd + 1) / 2 > FA_MAXPAIR) return -1;
  hipLaunchKernelGGL(full_attention_bf16_kernel, dim3(nutt, H), dim3(512), 0, st, q, kv, kv_rows, P,
                     p_rows, pos_u, pos_v, desc, H, nd, out, p_ld);
  CFM_CHECK_LAUNCH();
  return 0;
}

}  // namespace cfm
