/*
 * cfm_ops.h — operator-level entry points of libcfm.so (tests and integrators).
 *
 * These expose single kernels of the encoder path on caller-owned device
 * buffers, stream-ordered, no allocation.  They are not part of the
 * reference's surface; the parity tests use them to check one kernel at a time
 * against a torch fp32 reference of the same op.
 */
#ifndef CFM_OPS_H
#define CFM_OPS_H
#include "cfm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* epilogue kinds / activations of the projection GEMM C = A . W^T (A [M,K], W [N,K]) */
typedef enum { CFM_EPI_STORE = 0, CFM_EPI_STORE_F32 = 1, CFM_EPI_RESID = 2, CFM_EPI_QKV = 3, CFM_EPI_GLU = 4 } cfm_epi;
typedef enum { CFM_ACT_NONE = 0, CFM_ACT_RELU = 1, CFM_ACT_SILU = 2 } cfm_act;

/* dtype selects the operand type of A / W / T outputs (CFM_DTYPE_F32 or CFM_DTYPE_BF16).
 *   STORE:     out_T[(m+row_off)*ldo + n] = act(acc + bias)
 *   STORE_F32: out_f32[(m+row_off)*ldo + n] = alpha*(acc + bias)
 *   RESID:     x[m*ldx + n] += alpha*(acc + bias)*rowmask[m]
 *   QKV:       n < d -> out_T[m*d + n]; else out2_T[(m+row_off)*2d + head*128 + {0,64} + dim]
 *   GLU:       W rows interleaved [a16 | gate16]: out_T[(m+row_off)*ldo + ch] = a*sigmoid(gate)
 * variant (A/B testing): bit 0 forces the 128x128 kernel; bits 8-15 select a timing diagnostic of
 * the bf16 kernels (1 no MFMA, 2 no DMA in the loop, 3 no epilogue, 5 no stores; 0 = normal; only
 * in a library built with -DCFM_GEMM_DIAG); bits 16-17 the bf16 store policy (2 = nt); bits 18-20 the
 * K = 512 weight-stationary kernel (0 = model default, 1 = on, 2 = on at any M, 7 = off); bit 21 the QKV head dim
 * (0 = 64, 1 = 128: the K | V stream column of K / V column cc is (cc / dk) * 2 dk + {0, dk} + cc % dk); bits 22-23
 * the 256 x 256 kernel's column-group width ("col_group": tiles ordered group, row, column; 0 = all columns); bits
 * 24-27 a field f: the 256 x 256 kernel only from 4^f tiles of 256 x 256 on (f = 0: always; f = 15: never).
 * act: 0 none, 1 ReLU, 2 SiLU, 3 SiLU of a -log2(e)-prescaled input (STORE: a / (1 + 2^a); GLU: the gate half is
 * prescaled, out = a / (1 + 2^gate)).  GLU needs a bias and N % 32 == 0, QKV N == 3 d and d % dk == 0.
 * Kernels: f32 runs on 128 x 128 tiles (K % 32 == 0, lda, ldw % 4 == 0).  bf16 / f16 (K % 64 == 0, lda, ldw % 8 == 0)
 * run the weight-stationary kernel (K == 512, N % 256 == 0, N <= 8192, STORE / QKV / GLU, from 128 row tiles of 64 on,
 * GLU from 512), else the 256 x 256 kernel (N % 256 == 0), else 128 x 128 tiles.  The two big kernels store 16 B per
 * lane and take a call only if every pitch they write keeps that aligned -- ldo % 8 == 0 for 16-bit outputs, ldo % 4
 * == 0 / ldx % 4 == 0 for f32 outputs, out / out2 / x 16-B aligned (QKV: d % 64 == 0) -- otherwise the call runs on
 * 128 x 128 tiles, whose stores are scalar.  A call no kernel takes launches nothing and returns CFM_ERR_RUNTIME. */
cfm_status cfm_op_gemm(int32_t dtype, int32_t epi, int32_t act, const void* A, int32_t lda, const void* W, int32_t ldw,
                       int32_t M, int32_t N, int32_t K, const float* bias, float alpha, void* out, int32_t ldo,
                       int32_t row_off, void* out2, int32_t d, float* x, int32_t ldx, const uint8_t* rowmask,
                       int32_t variant, cfm_stream stream);
/* The kernel the call above would launch, decided by the same host predicates as the launch itself; touches no
 * device.  Buffers are taken as 16-B aligned (and d = N / 3 for QKV).  0 = none (an empty problem or an error). */
typedef enum { CFM_GEMM_NONE = 0, CFM_GEMM_128 = 1, CFM_GEMM_256 = 2, CFM_GEMM_WST = 3 } cfm_gemm_route;
int32_t cfm_op_gemm_route(int32_t dtype, int32_t epi, int32_t act, int32_t lda, int32_t ldw, int32_t M, int32_t N,
                          int32_t K, int32_t has_bias, int32_t ldo, int32_t ldx, int32_t variant);

/* One attention kernel on caller-owned buffers (csrc/attention.hip, attention128.hip).  `kernel` names the
 * kernel and nothing else runs in its place: when the selected kernel does not take the configuration
 * (dtype, dk, C, W, p_rows, T') the call launches nothing, leaves `out` untouched and returns CFM_ERR_ASSERT
 * with a message naming the kernel; a HIP failure is CFM_ERR_RUNTIME.
 *   q [rows][H*dk], out [rows][H*dk], kv [kv_rows][H][K dk | V dk] (dtype elements); P [p_rows] rows of stride
 *   p_ld (0 = H*dk), head h at column h*dk; pos_u / pos_v [H*dk] f32; desc [n_desc][8] int32 on the device:
 *   (Q_ROW0, NQ, KV_ROW0, KEY_LO, KEY_HI, P_BASE, Q_VALID, 0).  For descriptor b, head h, i < NQ, j in [KEY_LO, KEY_HI):
 *     s(i,j) = ((q_i + u).K[KV_ROW0 + j] + (q_i + v).P[P_BASE - i + j]) / sqrt(dk),  out_i = softmax_j(s) . V;
 *   rows i >= Q_VALID and rows without keys are written as 0.
 * GENERIC: any descriptors, f32 / bf16 / f16, dk 64 or 128.
 * RING:    bf16 / f16, dk 64; the descriptors of a masked-batch plan with one block per chunk (chunk c: Q_ROW0 =
 *          KV_ROW0 = c*C, NQ = Q_VALID = C, P_BASE = C-1), W = L + C + R; min_chunks = shortest run of chunks per
 *          block (the model's "attn_min_chunks"; >= 2).
 * A128:    bf16, dk 128, the same descriptors at C = 64; vt = V^T scratch [H*128][vt_ld] (vt_ld >= kv_rows,
 *          a multiple of 8), filled here by the transpose kernel before the attention kernel, as the model does.
 * DENSE:   bf16, dk 64; a full-attention padded plan: nutt utterances x nd consecutive 64-query descriptors
 *          (n_desc = nutt * nd), t_keys = T' <= 384. */
typedef enum { CFM_ATTN_GENERIC = 0, CFM_ATTN_RING = 1, CFM_ATTN_A128 = 2, CFM_ATTN_DENSE = 3 } cfm_attn_kernel;
cfm_status cfm_op_attention(int32_t dtype, int32_t kernel, const void* q, const void* kv, int32_t kv_rows, const void* P,
                            int32_t p_rows, int32_t p_ld, const float* pos_u, const float* pos_v, const int32_t* desc,
                            int32_t n_desc, int32_t H, int32_t dk, int32_t C, int32_t W, void* out, int32_t min_chunks,
                            void* vt, int32_t vt_ld, int32_t nutt, int32_t nd, int32_t t_keys, cfm_stream stream);

/* One LayerNorm kernel on caller-owned buffers (csrc/norm.hip).  `kind` names the kernel and nothing else runs in
 * its place: a d the kernels do not take (not 128 / 256 / 512) launches nothing, leaves x and out untouched and
 * returns CFM_ERR_ASSERT naming the kernel; an argument combination outside the contract below is CFM_ERR_VALUE.
 *   x [M][d] f32, read and written; y, y2 [M][d] dtype elements or null; ymask, ymask2, rowmask [M] bytes (0 / 1) or
 *   null (= all 1); w1, b1, w2, b2 [d] f32.  Per row r, in f32 and in this order:
 *     v = x_r;  if y: v = fmaf(alpha * ymask[r], y_r, v);  if y2 (needs y): v = fmaf(alpha2 * ymask2[r], y2_r, v)
 *     LN(v; w, b) = (v - mean(v)) * rsqrt(mean((v - mean(v))^2) + eps) * w + b     (biased variance)
 *   LN  (ln_kernel):      with y and not defer: x_r = v; with defer: x is left unwritten (the next LayerNorm
 *                         re-applies the branch as its first term).  out_r = LN(v; w1, b1) as dtype, or a zero row
 *                         where rowmask[r] == 0.  w2 / b2 are unused.
 *   LN2 (ln2_kernel):     x_r = t = LN(v; w1, b1) (f32);  out_r = (w2 ? LN(t; w2, b2) : t) as dtype.
 *   LN2_F32 (ln2_kernel): the same with out [M][d] f32.  defer and rowmask belong to LN alone. */
typedef enum { CFM_LN = 0, CFM_LN2 = 1, CFM_LN2_F32 = 2 } cfm_ln_kind;
cfm_status cfm_op_layernorm(int32_t dtype, int32_t kind, float* x, int32_t M, int32_t d, const void* y, float alpha,
                            const uint8_t* ymask, const void* y2, float alpha2, const uint8_t* ymask2, int32_t defer,
                            const float* w1, const float* b1, const float* w2, const float* b2, float eps, void* out,
                            const uint8_t* rowmask, cfm_stream stream);

/* The conv module's middle kernel (csrc/conv_module.hip, conv_dw_ln_silu<T>) on caller-owned buffers: depthwise conv
 * k = 15 + bias, LayerNorm over the channels, SiLU.  dtype selects the kernel together with d: f32 the per-tap kernel,
 * bf16 / f16 the dot2 whole-chunk kernel at d = 128 / 256 and the dot2 half-chunk kernel at d = 512; another d
 * launches nothing, leaves out untouched and returns CFM_ERR_ASSERT naming the kernels.
 *   glu, out: rows of d dtype elements; wdw_t [15][d] f32 tap-major; bdw, lnw, lnb [d] f32;
 *   desc [nblk][8] int32 on the device: (OUT_ROW0, NOUT <= 64, SRC_ROW0, J_LO, J_HI, -, -, -).  For block b, i < NOUT:
 *     a_c = bdw_c + sum over t < 15 with J_LO <= i + t < J_HI of wdw_t[t][c] * glu[SRC_ROW0 + i + t][c]
 *     out[OUT_ROW0 + i] = silu(LN(a; lnw, lnb, eps))
 *   glu rows of columns outside [J_LO, J_HI) are never read (SRC_ROW0 and J_LO may be negative); the 16-bit kernels
 *   run the conv on taps rounded to dtype.  Rows no block covers are not written. */
cfm_status cfm_op_conv_module(int32_t dtype, const void* glu, const int32_t* desc, int32_t nblk, int32_t d,
                              const float* wdw_t, const float* bdw, const float* lnw, const float* lnb, float eps,
                              void* out, cfm_stream stream);

/* The relative-position table kernel (csrc/misc.hip, pos_table_kernel): out [p_rows][d] dtype elements, row k at
 * distance p = anchor - k: out[k][2i] = sin(p * div_i), out[k][2i + 1] = cos(p * div_i), div_i = exp(2i * -(ln 1e4 / d)),
 * the angle |p| * div_i formed in f32.  d must be even (CFM_ERR_ASSERT otherwise, nothing launched). */
cfm_status cfm_op_pos_table(int32_t dtype, int32_t d, int32_t p_rows, int32_t anchor, void* out, cfm_stream stream);

/* One front-end conv0 + ReLU + dw1 kernel (csrc/frontend.hip) on a model's own weights (w0, b0, w1, b1, the packed
 * MFMA operands and CMVN of `m`; the element type is the model's compute dtype).  `kernel` names the kernel and
 * nothing else runs in its place -- in particular VALU on a bf16 model runs the VALU kernel, which the model's own
 * "fe_conv" 0 does not: a (dtype, d) the selected kernel does not take launches nothing, leaves out untouched and
 * returns CFM_ERR_ASSERT naming the kernel.
 *   VALU:     fe_conv0_dw_kernel, any dtype: f32 arithmetic throughout, out rounded to the dtype.
 *   MFMA_POS: fe_conv0_dw_mfma_kernel (position-stationary; "fe_conv" 1), bf16 / f16, d % 64 == 0: the input after
 *             CMVN, w0 and b0 rounded to the dtype, conv0 accumulated in f32, ReLU and dw1 (w1, b1) in f32.
 *   MFMA_CH:  fe_conv0_dw_mfma2_kernel (channel-stationary; "fe_conv" 2 + k: about k + 1 chunks of 256 dw1 positions
 *             per workgroup), bf16 / f16, d % 64 == 0: as MFMA_POS, and conv0's ReLU output and w1 rounded to the
 *             dtype as well (dw1 on MFMA; b1 f32).  k is ignored by the other kernels.
 *   meta [nwin][8] int32 on the device, the plan's window records: window n reads W feature rows of 80 f32 from
 *   feats + meta[n][0] * 80 (packed mode, tab null) or from tab[meta[n][6]] + meta[n][7] * step * 80 (table mode:
 *   tab = device array of per-utterance row pointers); rows at or past meta[n][1] (NVALID) are zero padding and are
 *   never read.  CMVN, (x - mean) * istd, is applied after the padding when use_cmvn (padding rows become
 *   -mean * istd); with use_cmvn 0 it is skipped even if the model has CMVN.
 *   out [nwin][T2][19][d], T1 = (W - 3) / 2 + 1, T2 = (T1 - 3) / 2 + 1:
 *     out[n][t2][f2][c] = b1[c] + sum_{u,v<3} w1[c][u][v] * relu(b0[c] + sum_{a,b<3} w0[c][a][b] * x[4 t2 + 2u + a][4 f2 + 2v + b]) */
typedef enum { CFM_FE_VALU = 0, CFM_FE_MFMA_POS = 1, CFM_FE_MFMA_CH = 2 } cfm_fe_kernel;
cfm_status cfm_op_frontend_conv0_dw(const cfm_model* m, int32_t kernel, int32_t k, int32_t use_cmvn, const float* feats,
                                    const float* const* tab, int32_t step, const int32_t* meta, int32_t nwin, int32_t W,
                                    void* out, cfm_stream stream);

/* The front-end's dw2 (depthwise 3x3, stride 2, + bias) on a model's own weights, in [nwin][T2][19][d] ->
 * out [nwin][T3][9][d], T3 = (T2 - 3) / 2 + 1 (T2 >= 3), elements of the model's compute dtype:
 *   UNFUSED: fe_dw2_kernel (csrc/frontend.hip) with `seg` row segments per walk; `in` is the pw1 + ReLU output:
 *            out[n][t3][f3][c] = b2[c] + sum_{u,v<3} w2[c][u][v] * in[n][2 t3 + u][2 f3 + v][c]
 *            (16-bit models: the 9 taps rounded to the dtype, f32 accumulation).
 *   FUSED:   the pw1 + ReLU + dw2 weight-stationary GEMM (csrc/gemm_wst_impl.h, EPI_DW2) with the model's pw1, b_pw1,
 *            w2, b2; `in` is the dw1 output and the pw1 rows relu(in . pw1^T + b_pw1), rounded to the dtype, never
 *            reach memory.  Where gemm_bf16_wst declines (an fp32 model, d != 512) nothing is launched, out is left
 *            untouched and the call returns CFM_ERR_ASSERT naming the kernel; `seg` is unused. */
typedef enum { CFM_FE_DW2_UNFUSED = 0, CFM_FE_DW2_FUSED = 1 } cfm_fe_dw2_mode;
cfm_status cfm_op_frontend_dw2(const cfm_model* m, int32_t mode, const void* in, int32_t nwin, int32_t T2, int32_t seg,
                               void* out, cfm_stream stream);

/* One segment attention kernel of the attention decoder on caller-owned buffers (csrc/aed.hip).  `kernel` names the
 * kernel and nothing else runs in its place: a configuration the selected kernel does not take launches nothing,
 * leaves `out` untouched and returns CFM_ERR_ASSERT naming the kernel.
 *   q [q_rows][H*dk], out [q_rows][H*dk], kv [k_rows][K (H*dk) | V (H*dk)] (dtype elements), head h at column h*dk
 *   of each part; desc [n_seg][8] int32 on the device: (Q0, NQ, K0, NK, CAUSAL, 0, 0, 0).  For segment s, head h,
 *   query i < NQ (row Q0 + i) and the keys j < NK (row K0 + j) it sees -- all of them, or j <= i when CAUSAL:
 *     out_i = softmax_j(q_i . k_j / sqrt(dk)) . V      (f32 online softmax; no visible key: a zero row)
 *   Rows that no descriptor covers are neither read nor written.  Query ranges must not overlap.
 * GENERIC: f32 / bf16 / f16, dk a multiple of 16 up to 128.   MFMA: bf16 / f16, dk 64 or 128.
 * scratch: n_seg + 2 int32 on the device: [0] a status word, zero after the call unless a descriptor's range lies
 * outside its array (1; that segment is skipped) or the segments hold more query tiles than q_rows allows (4);
 * [1 ..] the segments' tile offsets. */
typedef enum { CFM_SEG_ATTN_GENERIC = 0, CFM_SEG_ATTN_MFMA = 1 } cfm_seg_attn_kernel;
cfm_status cfm_op_seg_attention(int32_t dtype, int32_t kernel, const void* q, int32_t q_rows, const void* kv,
                                int32_t k_rows, const int32_t* desc, int32_t n_seg, int32_t H, int32_t dk, void* out,
                                int32_t* scratch, cfm_stream stream);

/* One attention kernel of the attention decoding mode on caller-owned buffers (csrc/attdec.hip).  `kernel` names the
 * kernel and nothing else runs in its place (CFM_ERR_ASSERT naming it for a configuration it does not take).
 * Rows r = u * beam + j, R = B * beam, beam <= 16; q, out [R][H*dk] (dtype elements), head h at column h*dk.
 *   SELF_GATHER (f32 / bf16 / f16, dk a multiple of 16 up to 128): kv [kv_rows positions][R][K (H*dk) | V (H*dk)];
 *     row r attends over n_keys (1 .. kv_rows) positions: position p < n_keys - 1 is read from slot
 *     ancestry[r * ancestry_ld + p] (a row index), position n_keys - 1 from slot r.
 *   CROSS_GENERIC (as above) / CROSS_MFMA (bf16 / f16, dk 64 or 128): kv [kv_rows][K | V]; the beams of utterance u
 *     attend over its rows [utt_start[u], + utt_len[u]) (device int32 [B]; none, or a range outside kv: a zero row),
 *     split into n_split (1 .. 16) key parts merged by their (m, l, o); scratch: n_split * R * (H*dk + 2 H) f32
 *     (unused with one part).
 *   out_r = softmax_j(q_r . k_j / sqrt(dk)) . V, f32 online softmax. */
typedef enum { CFM_DEC_ATTN_SELF_GATHER = 0, CFM_DEC_ATTN_CROSS_GENERIC = 1, CFM_DEC_ATTN_CROSS_MFMA = 2 } cfm_dec_attn_kernel;
cfm_status cfm_op_decode_attention(int32_t dtype, int32_t kernel, const void* q, void* out, int32_t B, int32_t beam,
                                   int32_t H, int32_t dk, const void* kv, int32_t kv_rows, const int32_t* ancestry,
                                   int32_t ancestry_ld, int32_t n_keys, const int32_t* utt_start, const int32_t* utt_len,
                                   int32_t n_split, float* scratch, cfm_stream stream);

/* The kernels of the transducer prefix beam search (csrc/rnnt_beam.hip), one at a time.
 * fused_topk: per row of logits [R, V] f32: lp = log_softmax(row), f = log(transducer_weight * exp(lp) + ctc_weight *
 *   exp(ctc_logp row)) (ctc_logp [R, V] or null: the second term is 0), the K <= 16 largest f by (value descending,
 *   index ascending) into vals / ids [R, K].
 * beam_prune: T frames of the expand / fuse / prune step for one utterance, from the start state ([blank], score 0):
 *   topk_vals / topk_ids [T, K, K] are the fused top-k of the hypothesis in slot h at frame t (slots past the beam's
 *   count are not read); trace_parent / trace_token / trace_score [T, K] receive each frame's new beam (-1 parents past
 *   the count), n_hyps [T] its count.
 * lstm_step: embedding, LSTM layers and the composed projection + pred_ffn for R rows: tokens [R], h_in / c_in
 *   [num_layers, R, hidden] -> h_out / c_out, pred_out [R, join_dim]. */
cfm_status cfm_op_rnnt_fused_topk(const float* logits, const float* ctc_logp, int32_t R, int32_t V, int32_t K,
                                  float ctc_weight, float transducer_weight, float* vals, int32_t* ids,
                                  cfm_stream stream);
size_t cfm_op_rnnt_beam_prune_workspace_bytes(int32_t T, int32_t K);
cfm_status cfm_op_rnnt_beam_prune(const float* topk_vals, const int32_t* topk_ids, int32_t T, int32_t K, int32_t blank,
                                  int32_t* trace_parent, int32_t* trace_token, double* trace_score, int32_t* n_hyps,
                                  void* workspace, size_t workspace_bytes, cfm_stream stream);
size_t cfm_op_rnnt_lstm_step_workspace_bytes(const cfm_rnnt* h, int32_t R);
cfm_status cfm_op_rnnt_lstm_step(cfm_rnnt* h, const int32_t* tokens, const float* h_in, const float* c_in, int32_t R,
                                 float* h_out, float* c_out, float* pred_out, void* workspace, size_t workspace_bytes,
                                 cfm_stream stream);
/* predictor_step (a stateless handle only: CFM_ERR_VALUE on an LSTM one): the context kernel, the ffn GEMM (embedding),
 * LayerNorm + activation and the pred_ffn GEMM for R id windows: windows [R, history_size + 1] int32, oldest id
 * first, -1 = a position before the sos (a zero vector) -> y_out [R, embed_size] (the predictor output) and
 * pred_out [R, join_dim] (its pred_ffn projection). */
size_t cfm_op_rnnt_predictor_step_workspace_bytes(const cfm_rnnt* h, int32_t R);
cfm_status cfm_op_rnnt_predictor_step(cfm_rnnt* h, const int32_t* windows, int32_t R, float* y_out, float* pred_out,
                                      void* workspace, size_t workspace_bytes, cfm_stream stream);

/* The kernels of the full-sum transducer score (csrc/rnnt_lattice.hip, cfm_rnnt_td_score in cfm.h), one at a time.
 * lattice: the joint over the lattice nodes of cfm_rnnt_td_score's descriptors from given projections: enc_proj
 *   [rows, join_dim] f32 (enc_ffn with bias), pred_proj [n_states, join_dim] f32 (pred_ffn of the predictor output
 *   of each state); per node b = log_softmax(ffn_out(tanh(e + p)))[blank] and k = the same at the next state's
 *   token (0 on a hypothesis' last state) into b_out / k_out [total_nodes] f32.  dtype CFM_DTYPE_F32 / CFM_DTYPE_BF16.
 * alpha: the recursion of cfm_rnnt_td_score on given b / k [total_nodes] f32: hypothesis i has hyp_t[i] frames and
 *   hyp_u1[i] states, its nodes from node0[i] on -> td_out [n_hyp] f64; the first int32 of the workspace is the
 *   status word (1 = a hypothesis outside b / k, its td 0; 4 = a non-finite node). */
cfm_status cfm_op_rnnt_lattice(cfm_rnnt* h, int32_t dtype, const float* enc_proj, int32_t rows, const float* pred_proj,
                               int32_t n_states, const int32_t* tokens, const int32_t* row_start,
                               const int32_t* row_len, int32_t B, const int32_t* desc, const int64_t* node0,
                               int32_t n_hyp, int64_t total_nodes, float* b_out, float* k_out, cfm_stream stream);
size_t cfm_op_rnnt_alpha_workspace_bytes(int32_t n_hyp, int32_t max_u1);
cfm_status cfm_op_rnnt_alpha(const float* b, const float* k, const int32_t* hyp_t, const int32_t* hyp_u1,
                             const int64_t* node0, int32_t n_hyp, int32_t max_u1, int64_t total_nodes, double* td_out,
                             void* workspace, size_t workspace_bytes, cfm_stream stream);

#ifdef __cplusplus
}
#endif
#endif
