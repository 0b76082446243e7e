/*
 * cfm.h — C-ABI of the MI355X-native ChunkFormer encoder hot path (libcfm.so).
 *
 * Drop-in boundary for the reference's `ChunkFormerEncoder` method set
 * (ishine/chunkformer, chunkformer/modules/encoder.py).  The reference has no
 * FFI of its own: it is plain Python method calls on nn.Modules, so each entry
 * point below names the reference method it replaces; the Python mirror
 * (chunkformer_amd/encoder.py) binds them with ctypes exactly as the
 * reference's callers call the module.
 *
 * Conventions
 *   - every pointer named *_dev / buffer argument is DEVICE memory owned by the
 *     caller (torch tensors in the Python mirror); host arrays are named *_host
 *     or documented as host;
 *   - all device work is stream-ordered on `stream` (a hipStream_t);
 *   - cfm_encode_* and cfm_ctc_* perform no allocation and no host
 *     synchronisation, so they can be captured into a HIP graph;
 *   - one model handle per device, one host thread per device (one
 *     torch.distributed rank per GPU);
 *   - status codes map to the reference's exception types:
 *       CFM_ERR_VALUE   -> ValueError      (bad argument / size)
 *       CFM_ERR_ASSERT  -> AssertionError  (unsupported configuration, encoder.py:94-96,116)
 *       CFM_ERR_RUNTIME -> RuntimeError    (HIP failure, shape mismatch)
 *     cfm_last_error() returns the thread-local message of the last failure.
 */
#ifndef CFM_H
#define CFM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { CFM_OK = 0, CFM_ERR_VALUE = 1, CFM_ERR_ASSERT = 2, CFM_ERR_RUNTIME = 3 } cfm_status;
/* F16: the reference decoder's --autocast_dtype fp16 (chunkformer_model.py:709-743) */
typedef enum { CFM_DTYPE_F32 = 0, CFM_DTYPE_BF16 = 1, CFM_DTYPE_F16 = 2 } cfm_dtype;

/* encoder_conf subset (encoder.py:36-70) + CTC output_dim (init_model.py:73) */
typedef struct {
  int32_t input_dim;      /* 80 */
  int32_t d_model;        /* output_size: 128, 256 or 512 */
  int32_t n_heads;        /* attention_heads: head dim d_model / n_heads must be 64 or 128 */
  int32_t ffn_dim;        /* linear_units */
  int32_t num_blocks;
  int32_t kernel_size;    /* cnn_module_kernel (15) */
  int32_t vocab;          /* CTC output_dim, 0 = no CTC head */
  float norm_eps;         /* 1e-5 */
  int32_t has_cmvn;       /* global_cmvn present */
  int32_t compute_dtype;  /* cfm_dtype: F32 = exact-f32 MFMA parity mode, BF16 / F16 = 16-bit MFMA, f32 accumulate */
} cfm_config;

/* one state_dict tensor, by reference key name, host f32 contiguous */
typedef struct {
  const char* name;
  const float* data;
  int64_t numel;
} cfm_tensor_view;

typedef struct cfm_model cfm_model;
typedef void* cfm_stream; /* hipStream_t */

const char* cfm_version(void);
const char* cfm_last_error(void);

/* Build a model on `device` from reference state_dict tensors (replaces
 * init_speech_model + load_checkpoint for the encoder, init_model.py:61-145,
 * checkpoint.py:26-41).  Weights are repacked into device layouts owned by the
 * handle.  Missing / mis-shaped keys -> CFM_ERR_VALUE. */
cfm_status cfm_model_create(const cfm_config* cfg, const cfm_tensor_view* weights, int32_t n_weights,
                            int32_t device, cfm_model** out);
void cfm_model_destroy(cfm_model* m);
/* diagnostic knobs:
 *   "max_layers"    run only the first N blocks (-1 = all)
 *   "profile"       bitmask of kernel classes to bracket with HIP events on the launch
 *                   stream (bit i = class i of cfm_profile_read); 0 = off
 *   "profile_reset" clear the accumulated profile
 *   "ring_attention" 1 (default) = bf16 masked batch uses the sliding-ring attention kernel,
 *                   0 = the generic per-block kernel (A/B testing)
 *   "fe_fuse_dw2"   1 (default) = bf16 front-end pw1 + ReLU + dw2 in one weight-stationary GEMM,
 *                   0 = pw1 GEMM + the separate dw2 kernel (bit-identical; A/B testing)
 *   "fe_conv"       bf16 conv0 + ReLU + dw1: 6 (default) = channel-stationary, dw1 on MFMA with
 *                   conv0's ReLU output rounded to bf16 (as autocast does), about 5 chunks of 256
 *                   positions per workgroup, balanced per window (2 + k: about k + 1 chunks);
 *                   1 = position-stationary, dw1 in f32 on the VALU
 * (all per-model kernel options: struct Tuning in chunkformer_amd/csrc/cfm_kernels.h, keyed in
 *  cfm_model_set_option, chunkformer_amd/csrc/model.hip) */
cfm_status cfm_model_set_option(cfm_model* m, const char* key, int64_t value);
/* Per kernel class: name, accumulated milliseconds and launch count of the
 * event-bracketed launches since the last reset.  Host-synchronising (waits for
 * the recorded events); never call it inside graph capture.  Returns the number
 * of classes (fills at most `cap`). */
int32_t cfm_profile_read(const cfm_model* m, const char** names, double* total_ms, int64_t* launches, int32_t cap);

/* ------------------------------------------------------------------ plans
 * A plan is an int32 blob computed on the HOST (no GPU needed) and uploaded by
 * the caller; it carries the packer's integer work (chunk windows, masks as
 * [lo, hi) ranges, kernel block descriptors, per-row validity).
 *
 * cfm_plan_masked: the masked-batch packer of forward_parallel_chunk
 * (encoder.py:534-604 + masks 625-645), bit-exact.  Per utterance: lens[b]
 * fbank frames, offsets[b] carried offset (encoder.py:565-594).  Outputs
 * n_chunks[b], out_lens[b] = calc_length(lens[b]) (subsampling.py:270-288),
 * *total_chunks.  Call with plan == NULL to get *plan_ints, then again with a
 * buffer of that many int32. */
cfm_status cfm_plan_masked(const int32_t* lens_host, const int32_t* offsets_host, int32_t B, int32_t chunk_size,
                           int32_t left_context, int32_t right_context, int32_t* n_chunks_host,
                           int32_t* out_lens_host, int32_t* total_chunks, int32_t* plan_host, int64_t* plan_ints);
/* cfm_plan_masked_ex: the same with the feature row count of each utterance (lens_host: x.size(0),
 * which the reference pads and unfolds, encoder.py:556-564) separate from xs_origin_lens
 * (mask_lens_host, NULL = lens_host), which bounds the masks and gives out_lens (encoder.py:567-596,
 * 673).  A length pair whose bound count differs from the window count is the reference's shape
 * mismatch: CFM_ERR_RUNTIME. */
cfm_status cfm_plan_masked_ex(const int32_t* lens_host, const int32_t* mask_lens_host, const int32_t* offsets_host,
                              int32_t B, int32_t chunk_size, int32_t left_context, int32_t right_context,
                              int32_t* n_chunks_host, int32_t* out_lens_host, int32_t* total_chunks, int32_t* plan_host,
                              int64_t* plan_ints);

/* cfm_plan_padded: padded-batch geometry of forward_encoder (encoder.py:220-274,
 * attention.py:334-386, convolution.py:148-167).  chunk_size <= 0 -> full
 * attention.  *t_out = calc_length(T). */
cfm_status cfm_plan_padded(const int32_t* lens_host, int32_t B, int32_t T, int32_t chunk_size, int32_t left_context,
                           int32_t right_context, int32_t* t_out, int32_t* plan_host, int64_t* plan_ints);

/* ------------------------------------------------------------------ encoder
 * cfm_encode_masked replaces ChunkFormerEncoder.forward_parallel_chunk
 * (encoder.py:503-681).  feats_dev: the B utterances' fbank concatenated
 * [sum T_b, 80] f32.  att_cache_in / cnn_cache_in: [nb, L, H, 2*dk] / [nb, d, 7]
 * f32 or NULL (no cache: zeros, and no new cache is produced).  With caches,
 * the new caches (attention.py:466-467, convolution.py:228-230) are written to
 * att_cache_out / cnn_cache_out (may alias the inputs).  out_dev: [N*C, d] f32
 * after after_norm.  workspace: cfm_workspace_bytes_masked() bytes.  plan_host is the
 * host copy of the plan (only its header is read: launch geometry), plan_dev the
 * same blob in device memory (read by the kernels). */
size_t cfm_workspace_bytes_masked(const cfm_model* m, int32_t total_chunks, int32_t chunk_size, int32_t left_context,
                                  int32_t right_context);
cfm_status cfm_encode_masked(const cfm_model* m, const float* feats_dev, const int32_t* plan_host,
                             const int32_t* plan_dev, const float* att_cache_in, const float* cnn_cache_in, int32_t truncated_context_size,
                             float* att_cache_out, float* cnn_cache_out, float* out_dev, void* workspace,
                             size_t workspace_bytes, cfm_stream stream);

/* cfm_encode_masked reading each utterance's fbank where the caller holds it: utt_feats_dev is a
 * DEVICE array of B pointers, utterance b's [x.size(0), 80] f32 rows (the reference's list `xs`,
 * encoder.py:553-564), in the order of the plan's lengths.  Same result as cfm_encode_masked on the
 * concatenation, without the concatenation copy (torch.cat at encoder.py:606). */
cfm_status cfm_encode_masked_utts(const cfm_model* m, const float* const* utt_feats_dev, const int32_t* plan_host,
                                  const int32_t* plan_dev, const float* att_cache_in, const float* cnn_cache_in,
                                  int32_t truncated_context_size, float* att_cache_out, float* cnn_cache_out,
                                  float* out_dev, void* workspace, size_t workspace_bytes, cfm_stream stream);

/* cfm_encode_masked in stages, for pipelining consecutive endless_decode segments (segment k + 1's
 * layer l needs only segment k's layer-l caches): stage -1 = the front-end, relative positions and the
 * first LayerNorm; stage l = encoder layer l (the last one ends with after_norm into out_dev).  Calls
 * over consecutive stage ranges [stage_lo, stage_hi] with the same plan, caches and workspace equal one
 * cfm_encode_masked call bit for bit; the workspace carries the state between them. */
cfm_status cfm_encode_masked_stages(const cfm_model* m, const float* feats_dev, const int32_t* plan_host,
                                    const int32_t* plan_dev, const float* att_cache_in, const float* cnn_cache_in,
                                    int32_t truncated_context_size, float* att_cache_out, float* cnn_cache_out,
                                    float* out_dev, void* workspace, size_t workspace_bytes, int32_t stage_lo,
                                    int32_t stage_hi, cfm_stream stream);

/* cfm_encode_padded replaces ChunkFormerEncoder.forward_encoder (encoder.py:220-274)
 * and therefore ChunkFormerModel.encode (chunkformer_model.py:256-274).
 * xs_dev: [B, T, 80] f32 padded batch; out_dev: [B, T', d] f32. */
size_t cfm_workspace_bytes_padded(const cfm_model* m, int32_t B, int32_t T, int32_t chunk_size, int32_t left_context,
                                  int32_t right_context);
cfm_status cfm_encode_padded(const cfm_model* m, const float* xs_dev, const int32_t* plan_host, const int32_t* plan_dev,
                             float* out_dev, void* workspace, size_t workspace_bytes, cfm_stream stream);

/* ------------------------------------------------------------------ streaming
 * cfm_plan_stream + cfm_encode_stream replace ChunkFormerEncoder.forward_chunk
 * (encoder.py:310-385), the realtime path (apps/realtime-asr/stream_asr.py:164-172):
 * xs_dev [B, T, 80] f32 (every frame valid), T' = calc_length(T) with
 * right_context_size <= T' <= chunk_size + right_context_size; `offset` = frames already
 * streamed (keys of the first L - offset cache slots are masked, encoder.py:351-357).
 * att_cache_in [nb, B, H, L, 2*dk] and cnn_cache_in [nb, B, d, 7] f32 are required (the
 * reference's head-major layout); the new caches (encoder.py:374-383) go to
 * att_cache_out / cnn_cache_out (may alias the inputs; NULL = not wanted).  out_dev: [B, T', d]
 * f32 after after_norm.  One plan serves every batch element (they share T and offset). */
cfm_status cfm_plan_stream(int32_t T, int32_t chunk_size, int32_t left_context, int32_t right_context, int32_t offset,
                           int32_t* t_out, int32_t* plan_host, int64_t* plan_ints);
size_t cfm_workspace_bytes_stream(const cfm_model* m, int32_t T, int32_t chunk_size, int32_t left_context,
                                  int32_t right_context);
cfm_status cfm_encode_stream(const cfm_model* m, const float* xs_dev, int32_t B, const int32_t* plan_host,
                             const int32_t* plan_dev, const float* att_cache_in, const float* cnn_cache_in,
                             float* att_cache_out, float* cnn_cache_out, float* out_dev, void* workspace,
                             size_t workspace_bytes, cfm_stream stream);

/* Materialise att_mask [N, L+C+R] and mask_pad [N, C+14] (0/1 bytes) of a masked
 * plan: the exact tensors encoder.py:627-645 builds. */
cfm_status cfm_masks_from_plan(const int32_t* plan_host, const int32_t* plan_dev, uint8_t* att_mask_dev,
                               uint8_t* mask_pad_dev, cfm_stream stream);

/* ------------------------------------------------------------------ CTC head
 * CTC.log_softmax (ctc.py:73-81) + argmax (chunkformer_model.py:437-438, 526-527)
 * over enc_dev [rows, d].  logp_dev [rows, V] may be NULL (ids only: logits go to
 * the workspace); ids_dev [rows] int32 may be NULL. */
size_t cfm_ctc_workspace_bytes(const cfm_model* m, int32_t rows);
cfm_status cfm_ctc_logprobs(const cfm_model* m, const float* enc_dev, int32_t rows, float* logp_dev, int32_t* ids_dev,
                            void* workspace, size_t workspace_bytes, cfm_stream stream);

/* Fused CTC tail, ids only: ids_dev[rows] = argmax of CTC.log_softmax (ctc.py:73-81) as
 * chunkformer_model.py:437-438 / 526-527 take it.  On bf16 models with d_model 512 the logits never
 * leave registers (no [rows, V] tensor; workspace 0 bytes); otherwise it runs the log-softmax path
 * in the workspace (cfm_ctc_ids_workspace_bytes). */
size_t cfm_ctc_ids_workspace_bytes(const cfm_model* m, int32_t rows);
cfm_status cfm_ctc_ids(const cfm_model* m, const float* enc_dev, int32_t rows, int32_t* ids_dev, void* workspace,
                       size_t workspace_bytes, cfm_stream stream);

/* CTC post-processing on device, one utterance b = frames [row_start[b], row_start[b] + row_len[b])
 * of ids_dev (device int32 arrays; regions must not overlap).  Outputs are written compacted at
 * the start of each utterance's region:
 *   max_silence < 0: remove_duplicates_and_blank (utils/model_utils.py:23-32): tokens[] and the
 *     frame of each token (gen_ctc_peak_time, model_utils.py:49-58), n_tokens[b];
 *   max_silence >= 0: the sentence split of get_output_with_timestamps (model_utils.py:174-221)
 *     at max_silence (= max_silence_duration // 0.08) blank frames: per segment the de-duplicated
 *     non-blank tokens (tokens[], token_frames[]) and segments[s] = {first token, start frame,
 *     end frame} (80 ms frames), n_tokens[b], n_segments[b]. */
cfm_status cfm_ctc_collapse(const int32_t* ids_dev, const int32_t* row_start_dev, const int32_t* row_len_dev, int32_t B,
                            int32_t blank_id, int32_t max_silence, int32_t* tokens_dev, int32_t* token_frames_dev,
                            int32_t* n_tokens_dev, int32_t* segments_dev /* [rows, 3] or NULL */,
                            int32_t* n_segments_dev /* [B] or NULL */, cfm_stream stream);

/* ---- CTC prefix beam search (modules/search.py:131-249 with score = log_add([s, ns]); hotword
 * biasing: utils/context_graph.py).
 *
 * Per-frame top-k of the CTC log-probs over enc_dev [rows, d]: the k largest logit - lse of every row
 * (lse as CTC.log_softmax forms it), ordered by value descending, index ascending.  The head GEMM runs
 * in row slabs inside the call, so the logit workspace is bounded whatever `rows` is, and no [rows, V]
 * log-prob tensor is written.  1 <= k <= 16, k <= V.  No allocation, no host synchronisation. */
size_t cfm_ctc_topk_workspace_bytes(const cfm_model* m, int32_t rows, int32_t k);
int32_t cfm_ctc_topk_slab_rows(const cfm_model* m);
cfm_status cfm_ctc_topk(const cfm_model* m, const float* enc_dev, int32_t rows, int32_t k,
                        float* topk_logp_dev /* [rows, k] */, int32_t* topk_ids_dev /* [rows, k] */,
                        void* workspace, size_t workspace_bytes, cfm_stream stream);
/* The same selection over log-probs logp_dev [rows, V] f32 given directly (on the current device). */
cfm_status cfm_ctc_topk_logp(const float* logp_dev, int32_t rows, int32_t V, int32_t k, float* topk_logp_dev,
                             int32_t* topk_ids_dev, cfm_stream stream);

/* Biasing graph: flat HOST arrays of an Aho-Corasick graph with n_nodes nodes (root = 0, ids in
 * creation order): per node the fail arc and the token / node / output scores; n_trans transitions
 * (node, token, next) sorted by (node, token). */
typedef struct cfm_ctx cfm_ctx;
cfm_status cfm_ctx_create(int32_t n_nodes, const int32_t* fail_host, const double* token_score_host,
                          const double* node_score_host, const double* output_score_host, int32_t n_trans,
                          const int32_t* trans_node_host, const int32_t* trans_token_host,
                          const int32_t* trans_next_host, int32_t device, cfm_ctx** out);
void cfm_ctx_destroy(cfm_ctx* h);

/* The search over packed top-k rows [rows, k], one workgroup per utterance b = rows
 * [row_start[b], row_start[b] + row_len[b]) as in cfm_ctc_collapse; nothing synchronises between
 * workgroups.  Hypothesis n of utterance b is written compacted at out_*[n, row_start[b] ..];
 * out_len / out_score [B, k] (score = total score after finalize, f64), n_hyps [B] (fewer than k
 * hypotheses can exist; row_len == 0 gives one empty hypothesis with score 0).  out_times_dev NULL: no
 * times.  The first int32 of the workspace is an error word, zero after a complete search (1: a row
 * range outside [0, rows); 4: a NaN score, from non-finite log-probs; other values: internal); read it after the stream has completed.  A
 * workspace smaller than cfm_ctc_beam_workspace_bytes is CFM_ERR_VALUE before anything is launched. */
size_t cfm_ctc_beam_workspace_bytes(int32_t rows, int32_t B, int32_t k, int32_t with_times, int32_t n_context_nodes);
cfm_status cfm_ctc_beam_search(const float* topk_logp_dev, const int32_t* topk_ids_dev, int32_t rows, int32_t k,
                               const int32_t* row_start_dev, const int32_t* row_len_dev, int32_t B, int32_t blank_id,
                               const cfm_ctx* context /* or NULL */, int32_t* out_tokens_dev /* [k, rows] */,
                               int32_t* out_times_dev /* [k, rows] or NULL */, int32_t* out_len_dev /* [B, k] */,
                               double* out_score_dev /* [B, k] */, int32_t* n_hyps_dev /* [B] */, void* workspace,
                               size_t workspace_bytes, cfm_stream stream);

/* ---- CTC forced alignment (utils/model_utils.py:103-117 force_align, which the reference runs through
 * torchaudio.functional.forced_align on the CPU; semantics: DESIGN.md 9c).
 *
 * Viterbi alignment of a known target to packed log-probs logp_dev [rows, V] f32 (what cfm_ctc_logprobs
 * writes), one workgroup per utterance b = rows [row_start[b], row_start[b] + row_len[b]) as in
 * cfm_ctc_collapse, its target = targets_dev[target_start[b] .. + target_len[b]) (int32, packed,
 * n_targets in all).  Scores in f64; on exact ties stay, then step, then skip.  Outputs:
 *   frames_dev [rows] int32      the label of every frame of the utterance's rows (other rows untouched);
 *   frame_logp_dev [rows] f32    logp[t][frames[t]] (or NULL);
 *   spans_dev [n_targets, 2]     first and last frame, inclusive and relative to the utterance, of each
 *                                target token (or NULL);
 *   score_dev [B] f64            the alignment's log-probability;
 *   status_dev [B] int32         0 ok; 1 infeasible (row_len < target_len + adjacent repeats); 2 a row or
 *                                target range outside its array; 3 a target id outside [0, V) or equal to
 *                                blank_id; 4 end state not finite (NaN / -inf log-probs); 5 the
 *                                utterance's workspace region lies outside the workspace or the device
 *                                lengths differ from the host's.  Non-zero: that utterance's other
 *                                outputs are untouched.
 * cfm_ctc_align_plan (host only) returns the workspace bytes for the HOST length arrays and writes each
 * utterance's byte offset into it (upload them as ws_offset_dev): 2-bit backpointers, 4 bytes per frame
 * and 16 states, plus two alpha rows.  cfm_ctc_align takes the same host arrays again: a workspace
 * smaller than the plan is CFM_ERR_VALUE before anything is launched.  The alpha rows live in LDS for
 * utterances of up to lds_max_states states (2 * target_len + 1; negative = the default and maximum,
 * 8192; 0 = never), else in the workspace (256-byte aligned).  No allocation, no host synchronisation. */
#define CFM_ALIGN_GENERIC_STRIPS 1 /* flags: the strip loop without per-thread label registers (any length) */
size_t cfm_ctc_align_plan(const int32_t* row_len_host, const int32_t* target_len_host, int32_t B,
                          int64_t* ws_offset_host_out /* [B] or NULL */);
cfm_status cfm_ctc_align(const float* logp_dev, int32_t rows, int32_t V, const int32_t* row_start_dev,
                         const int32_t* row_len_dev, int32_t B, int32_t blank_id, const int32_t* targets_dev,
                         int32_t n_targets, const int32_t* target_start_dev, const int32_t* target_len_dev,
                         const int64_t* ws_offset_dev, const int32_t* row_len_host, const int32_t* target_len_host,
                         int32_t* frames_dev, float* frame_logp_dev /* or NULL */, int32_t* spans_dev /* or NULL */,
                         double* score_dev, int32_t* status_dev, int32_t lds_max_states, int32_t flags,
                         void* workspace, size_t workspace_bytes, cfm_stream stream);

/* ---- Kaldi log-mel filterbank (the reference's feature front: chunkformer_model.py:276-318 and
 * dataset/processor.py:210-239 call torchaudio.compliance.kaldi.fbank).  Fields and defaults follow
 * torchaudio's fbank() signature; the reference decodes with dither 0, energy_floor 0, 80 bins,
 * 25 / 10 ms, povey window, int16-scale samples.  Supported: dither 0, snip_edges, use_energy 0,
 * padded frames of 128 .. 1024 samples. */
typedef enum { CFM_WINDOW_POVEY = 0, CFM_WINDOW_HAMMING = 1, CFM_WINDOW_HANNING = 2, CFM_WINDOW_RECTANGULAR = 3,
               CFM_WINDOW_BLACKMAN = 4 } cfm_window_type;
typedef struct {
  float sample_frequency;        /* 16000 */
  float frame_length_ms;         /* 25 */
  float frame_shift_ms;          /* 10 */
  int32_t num_mel_bins;          /* 80 in the reference (torchaudio default 23) */
  float low_freq;                /* 20 */
  float high_freq;               /* 0: Nyquist; < 0: offset from Nyquist */
  float preemphasis_coefficient; /* 0.97 */
  float dither;                  /* must be 0 */
  int32_t remove_dc_offset;      /* 1 */
  int32_t round_to_power_of_two; /* 1 */
  int32_t snip_edges;            /* must be 1 */
  int32_t use_energy;            /* must be 0 */
  int32_t use_log_fbank;         /* 1 */
  int32_t window_type;           /* cfm_window_type, POVEY (blackman uses coefficient 0.42) */
} cfm_fbank_config;
typedef struct cfm_fbank cfm_fbank;

/* window, FFT twiddles and mel filters on `device` (replaces the per-call get_mel_banks /
 * _feature_window_function of compliance/kaldi.py) */
cfm_status cfm_fbank_create(const cfm_fbank_config* cfg, int32_t device, cfm_fbank** out);
void cfm_fbank_destroy(cfm_fbank* h);
/* frames of a waveform of num_samples samples: 1 + (n - win) / shift, 0 when n < win */
int64_t cfm_fbank_num_frames(const cfm_fbank* h, int64_t num_samples);
/* out_dev[frames, num_mel_bins] (f32) = kaldi.fbank(wave_dev[num_samples]) (f32 device samples,
 * int16 scale); stream-ordered, no allocation, no host synchronisation */
cfm_status cfm_fbank_compute(const cfm_fbank* h, const float* wave_dev, int64_t num_samples, float* out_dev,
                             cfm_stream stream);

/* ---- RNN-T consumer (model: transducer checkpoints): greedy search over encoder outputs, the
 * reference's optimized_search / batch_greedy_search (transducer/search/greedy_search.py:6-92) as
 * endless_decode / batch_decode call them (chunkformer_model.py:439-448, 533-543), with the shipped
 * RNNPredictor (lstm; transducer/predictor.py:66-208) and TransducerJoint (prejoin_linear, add,
 * tanh, ffn_out; transducer/joint.py:74-111).  Predictor and joint compute in f32. */
typedef struct {
  int32_t vocab;        /* output_dim */
  int32_t enc_dim;      /* joint_conf.enc_output_size (the encoder's d_model) */
  int32_t embed_size;   /* predictor_conf.embed_size */
  int32_t hidden;       /* predictor_conf.hidden_size */
  int32_t num_layers;   /* predictor_conf.num_layers (<= 4) */
  int32_t pred_out;     /* predictor_conf.output_size = joint_conf.pred_output_size */
  int32_t join_dim;     /* joint_conf.join_dim */
  int32_t blank;        /* 0 (init_model.py:125-128) */
} cfm_rnnt_config;
typedef struct cfm_rnnt cfm_rnnt;

/* weights by reference key: predictor.embed.weight, predictor.rnn.{weight,bias}_{ih,hh}_l{k},
 * predictor.projection.{weight,bias}, joint.{enc_ffn,pred_ffn,ffn_out}.{weight,bias} */
cfm_status cfm_rnnt_create(const cfm_rnnt_config* cfg, const cfm_tensor_view* weights, int32_t n_weights,
                           int32_t device, cfm_rnnt** out);
/* The reference's two stateless predictors (transducer/predictor.py:210-471) over the same joint: the output is a
 * function of the last history_size + 1 tokens, positions before the sos being zero vectors (init_state), not the
 * blank's embedding.
 *   CFM_RNNT_PRED_EMBEDDING (arXiv 2109.07513): x = sum_c (c_c . q_c) c_c / (n_head * K), q_c[d] = sum over heads of
 *     pos_embed.weight[head, d * K + c]; y = act(LayerNorm(ffn(x))).  Keys: predictor.embed.weight,
 *     predictor.pos_embed.weight [n_head, E * K] (pos_embed.bias is accepted and, as in the reference, never read),
 *     predictor.ffn.{weight,bias}, predictor.norm.{weight,bias}.
 *   CFM_RNNT_PRED_CONV: x[d] = sum_c conv.weight[d, 0, c] c_c[d] (+ conv.bias[d] with conv_bias); y = act(LayerNorm(x)).
 *     Keys: predictor.embed.weight, predictor.conv.weight [E, 1, K], predictor.conv.bias (conv_bias only),
 *     predictor.norm.{weight,bias}.
 * Both feed joint.pred_ffn as a separate [join_dim, E] product.  For these kinds cfg->hidden and cfg->num_layers are
 * ignored and cfg->embed_size == cfg->pred_out is required (CFM_ERR_ASSERT otherwise).  kind CFM_RNNT_PRED_RNN with a
 * null or any pcfg is cfm_rnnt_create.  Every other cfm_rnnt_* entry point works on either kind of handle.  The
 * multi-CU greedy search is not built for a stateless handle: cfm_rnnt_grid_blocks returns 0 and the option
 * "grid_blocks" is accepted and has no effect. */
#define CFM_RNNT_PRED_RNN 0
#define CFM_RNNT_PRED_EMBEDDING 1
#define CFM_RNNT_PRED_CONV 2
#define CFM_RNNT_ACT_RELU 0
#define CFM_RNNT_ACT_SWISH 1
#define CFM_RNNT_ACT_TANH 2
#define CFM_RNNT_ACT_GELU 3
typedef struct {
  int32_t kind;          /* CFM_RNNT_PRED_* */
  int32_t history_size;  /* 0 .. 8 */
  int32_t n_head;        /* embedding: >= 1 */
  int32_t activation;    /* CFM_RNNT_ACT_* */
  int32_t conv_bias;     /* conv: predictor.conv.bias is present and added */
  float ln_eps;          /* layer_norm_epsilon */
} cfm_rnnt_predictor_config;
cfm_status cfm_rnnt_create_ex(const cfm_rnnt_config* cfg, const cfm_rnnt_predictor_config* pcfg,
                              const cfm_tensor_view* weights, int32_t n_weights, int32_t device, cfm_rnnt** out);
void cfm_rnnt_destroy(cfm_rnnt* h);
size_t cfm_rnnt_workspace_bytes(const cfm_rnnt* h, int32_t rows);
/* Greedy search of utterances b = rows [row_start[b], row_start[b] + row_len[b]) of enc_dev
 * [rows, enc_dim] f32 (device int32 row arrays).  out_dev [rows, n_steps] int32 must be zeroed by the
 * caller; row t of an utterance receives the ids decided at its frame t in step order, exactly the
 * reference's output[:, t * n_steps + step] with the sos column removed (0 = blank). */
cfm_status cfm_rnnt_greedy(const cfm_rnnt* h, const float* enc_dev, int32_t rows, const int32_t* row_start_dev,
                           const int32_t* row_len_dev, int32_t B, int32_t n_steps, int32_t* out_dev, void* workspace,
                           size_t workspace_bytes, cfm_stream stream);
/* cfm_rnnt_greedy with per-call flags: CFM_RNNT_ONE_WORKGROUP runs this call on the one-workgroup kernel
 * whatever "grid_blocks" says (the caller's rerun after a grid barrier timed out), leaving the handle's
 * options and its grid weight image untouched. */
#define CFM_RNNT_ONE_WORKGROUP 1
cfm_status cfm_rnnt_greedy_ex(const cfm_rnnt* h, const float* enc_dev, int32_t rows, const int32_t* row_start_dev,
                              const int32_t* row_len_dev, int32_t B, int32_t n_steps, int32_t* out_dev, void* workspace,
                              size_t workspace_bytes, int32_t flags, cfm_stream stream);
/* Options: "grid_lds" (default 1) caches each workgroup's weight slices in LDS when they fit;
 * "grid_atomic" (default 1) exchanges the shared vectors by agent-scope atomics instead of fences;
 * "grid_blocks" = workgroups per utterance of the multi-CU search (default 32; 0 = one
 * workgroup per utterance always).  The multi-CU search runs when B <= 32 and B * grid_blocks <= the
 * device's CU count; cfm_rnnt_grid_blocks returns the workgroups per utterance a call with B
 * utterances uses (0: the one-workgroup kernel).  "lattice_dtype" (CFM_DTYPE_F32, the default, or CFM_DTYPE_BF16):
 * the operand type of cfm_rnnt_td_score's joint lattice kernel for calls that pass dtype -1. */
cfm_status cfm_rnnt_set_option(cfm_rnnt* h, const char* key, int64_t value);
int32_t cfm_rnnt_grid_blocks(const cfm_rnnt* h, int32_t B);
/* After a multi-CU call has completed: nonzero if one of its grid barriers timed out (the search then
 * stopped early and its output is incomplete); -1 if the word could not be read.  Synchronous. */
int32_t cfm_rnnt_error(const cfm_rnnt* h, const void* workspace, int32_t rows);

/* ---- Transducer prefix beam search (the reference's mode rnnt_beam_search: transducer/search/
 * prefix_beam_search.py:41-146) over the same handle, every utterance of the packed batch at once (csrc/rnnt_beam.hip).
 * Frame-synchronous, one predictor + joint step per hypothesis and frame, shallow-fused with the frame's CTC posterior:
 * logp = log(transducer_weight * p_rnnt + ctc_weight * p_ctc) in f32; candidate scores f32(score) + logp in f32,
 * prefix fusion (log_add) and ranking in f64, ties by creation order; top-k by (value descending, index ascending).
 *   enc_dev [rows, enc_dim] f32; ctc_logp_dev [rows, vocab] f32 (what cfm_ctc_logprobs writes) or null with
 *   ctc_weight == 0; utterance b = rows [row_start[b], + row_len[b]) (device int32 [B]); max_len >= every row_len
 *   (the host's frame count); beam 1 .. 16 and <= vocab; weights >= 0, not both 0.  embed_size, hidden_size and
 *   join_dim must be multiples of 32 (CFM_ERR_ASSERT otherwise).  A stateless handle (cfm_rnnt_create_ex) runs its
 *   context kernel, LayerNorm + activation and f32 GEMMs per frame in place of the LSTM steps, and a slot's state is
 *   history_size int32 ids: its workspace is the smaller for it.
 * Outputs, for up to `beam` hypotheses per utterance in final (score-descending) order:
 *   out_tokens / out_times [beam, rows] int32: hypothesis k of utterance b at [k * rows + row_start[b] ..), the frame
 *   at which each token was appended beside it; out_len [B, beam]; out_score [B, beam] f64; n_hyps [B].
 * Trace (all five arrays or none; row = row_start[b] + t): trace_parent / trace_token / trace_score [rows, beam]: the
 *   beam after frame t (parent slot, appended token or blank for an unchanged hypothesis, score; -1 parents past the
 *   count); trace_topv / trace_topi [rows, beam, beam]: the fused top-k of each hypothesis entering frame t.
 * Stream-ordered, no allocation after the handle's first search, no host synchronisation.  The first int32 of the
 * workspace is an error word: 0, or 1 = a row range outside the rows or longer than max_len (searched as empty),
 * 2 = trie map full, 3 = empty beam, 4 = NaN score (ranked as -inf); the error accessor below reads it
 * (synchronous). */
size_t cfm_rnnt_beam_workspace_bytes(const cfm_rnnt* h, int32_t rows, int32_t B, int32_t beam);
cfm_status cfm_rnnt_beam_search(cfm_rnnt* h, const float* enc_dev, int32_t rows, const float* ctc_logp_dev,
                                const int32_t* row_start_dev, const int32_t* row_len_dev, int32_t B, int32_t max_len,
                                int32_t beam, float ctc_weight, float transducer_weight, int32_t* out_tokens,
                                int32_t* out_times, int32_t* out_len, double* out_score, int32_t* n_hyps,
                                int32_t* trace_parent, int32_t* trace_token, double* trace_score, float* trace_topv,
                                int32_t* trace_topi, void* workspace, size_t workspace_bytes, cfm_stream stream);
int32_t cfm_rnnt_beam_error(const void* workspace);

/* ---- Full-sum transducer score of given hypotheses (the td score of the reference's modes rnnt_beam_attn_rescoring /
 * ctc_beam_td_attn_rescoring: Transducer._cal_transducer_score = -rnnt_loss, transducer/transducer.py:257-391) over
 * the same handle (csrc/rnnt_lattice.hip).  Hypothesis i of utterance utt (rows [row_start[utt], + row_len[utt]),
 * T = row_len[utt] >= 1) with U tokens owns U + 1 predictor states and T * (U + 1) lattice nodes, node (t, u) at
 * node0[i] + t * (U + 1) + u:
 *   tokens_dev [n_states] int32: state u of hypothesis i at first_state + u holds the token the predictor consumed to
 *     reach it (the blank for u = 0, y_u after); desc_dev [n_hyp][4] int32 = (utt, first_state, U + 1, 0);
 *   node0_dev [n_hyp + 1] int64: the running sum of T * (U + 1), node0[n_hyp] = total_nodes; max_u1 >= every U + 1.
 * One call = enc_ffn over the rows, max_u1 predictor steps over all hypotheses (a stateless handle: one predictor
 * pass over all n_states states, state s of a hypothesis reading tokens[max(first_state, s - history_size) .. s] and
 * zero vectors before first_state), the joint lattice kernel (per node
 * only b = log p(blank) and k = log p(next token), f32; `dtype` selects exact f32 MFMA operands (CFM_DTYPE_F32) or
 * bf16 operands with f32 accumulation (CFM_DTYPE_BF16), -1 the handle's "lattice_dtype" option, so that callers of
 * different types share a handle without touching its state) and the f64 recursion
 *   alpha[0,0] = 0, alpha[t,u] = log_add(alpha[t-1,u] + b[t-1,u], alpha[t,u-1] + k[t,u-1]),
 *   td = alpha[T-1,U] + b[T-1,U]                                                       -> td_out [n_hyp] f64.
 * Stream-ordered, no allocation after the handle's first call, no host synchronisation.  The first int32 of the
 * workspace is a status word (cfm_rnnt_beam_error reads it): 0, 1 = a descriptor outside its arrays (that
 * hypothesis' td is 0), 4 = a non-finite lattice node.  The workspace size is 0 for a geometry it cannot hold. */
size_t cfm_rnnt_td_workspace_bytes(const cfm_rnnt* h, int32_t rows, int32_t n_hyp, int32_t n_states, int32_t max_u1,
                                   int64_t total_nodes);
cfm_status cfm_rnnt_td_score(cfm_rnnt* h, const float* enc_dev, int32_t rows, const int32_t* row_start_dev,
                             const int32_t* row_len_dev, int32_t B, const int32_t* tokens_dev, int32_t n_states,
                             const int32_t* desc_dev, const int64_t* node0_dev, int32_t n_hyp, int32_t max_u1,
                             int64_t total_nodes, int32_t dtype, double* td_out, void* workspace,
                             size_t workspace_bytes, cfm_stream stream);

/* ---- classification consumer (model: classification checkpoints): masked mean pool over time of the
 * encoder output and the per-task linear heads, the reference's SpeechClassificationModel
 * _average_pooling + classify (modules/classification_model.py:174-200, 232-281), on packed rows:
 * utterance b = rows [row_start[b], row_start[b] + row_len[b]) of enc_dev [rows, d] f32 (device int32
 * row arrays as in cfm_ctc_collapse; regions must not overlap, gaps between them are never read).
 *   pooled[b, :] = sum of the utterance's rows / (row_len[b] + 1e-10f)      (zeros when row_len[b] == 0)
 *   logits[b, :] = W . pooled[b] + bias      W [sum_classes, d]: the tasks' Linear weights stacked in task order
 *   per task: pred = argmax (lowest index on ties), prob = softmax(logits_task)[pred]
 * Pooling and heads compute in f32 whatever the encoder's compute dtype (the reference runs the heads
 * under its fp16 autocast; this is the more exact of the two).  The summation order is fixed (no
 * floating-point atomics): two calls on the same input are bit-identical.  The pool and classify calls
 * perform no allocation and no host synchronisation (graph-capturable); their launch geometry follows
 * from rows and B alone.  d: a multiple of 4 up to 1024.  Limits (CFM_ERR_VALUE beyond): 1 to 16 tasks,
 * 1 to 1024 classes per task, 4096 classes in total. */
typedef struct {
  int32_t enc_dim;          /* the encoder's d_model */
  int32_t n_tasks;          /* len(model_conf.tasks) */
  int32_t num_classes[16];  /* in the order of model_conf.tasks */
} cfm_cls_config;
typedef struct cfm_cls cfm_cls;

/* weights: 2 * n_tasks views in task order, {weight [num_classes, enc_dim], bias [num_classes]} per task,
 * i.e. the reference keys classification_heads.<task>.linear.weight / .bias for the tasks of
 * model_conf.tasks in their order (the caller builds the keys; names are used in error messages only).
 * A missing or mis-sized view -> CFM_ERR_VALUE. */
cfm_status cfm_cls_create(const cfm_cls_config* cfg, const cfm_tensor_view* weights, int32_t n_weights,
                          int32_t device, cfm_cls** out);
void cfm_cls_destroy(cfm_cls* h);
/* workspace: int32 slab offsets [B + 1] (256-byte padded), then (ceil(rows / 64) + B) partial column
 * sums of d floats (one per 64-row slab of an utterance) */
size_t cfm_cls_pool_workspace_bytes(int32_t rows, int32_t d, int32_t B);
size_t cfm_cls_workspace_bytes(const cfm_cls* h, int32_t rows, int32_t B);
/* pooling alone (embeddings), on the current device; needs no handle.  pooled_dev [B, d] f32. */
cfm_status cfm_cls_pool(const float* enc_dev, int32_t rows, int32_t d, const int32_t* row_start_dev,
                        const int32_t* row_len_dev, int32_t B, float* pooled_dev, void* workspace,
                        size_t workspace_bytes, cfm_stream stream);
cfm_status cfm_cls_classify(const cfm_cls* h, const float* enc_dev, int32_t rows, const int32_t* row_start_dev,
                            const int32_t* row_len_dev, int32_t B, float* pooled_dev /* [B, d] or NULL */,
                            float* logits_dev /* [B, sum_classes] or NULL */, int32_t* pred_dev /* [B, n_tasks] */,
                            float* prob_dev /* [B, n_tasks] f32 */, void* workspace, size_t workspace_bytes,
                            cfm_stream stream);

/* ---- attention decoder consumer (model: hybrid CTC / attention checkpoints, `decoder: transformer` /
 * `bitransformer`): the left-to-right and right-to-left TransformerDecoder (modules/decoder.py:35-226, 330-484;
 * normalize_before, relu, position-wise feed-forward, all biases, dropout off) scoring the CTC prefix beam n-best
 * against the encoder output, as attention_rescoring consumes it (modules/search.py:358-439 over
 * asr_model.py:399-492).  Semantics: DESIGN.md 9d.  compute dtype: F32 = exact-f32 GEMMs and the generic segment
 * attention kernel; BF16 / F16 = 16-bit GEMMs (f32 accumulate) and the MFMA segment attention kernel at head dim
 * 64 / 128 (other head dims: the generic kernel on 16-bit rows).  Embedding, residual stream, LayerNorm statistics,
 * softmax and the log-sum-exp are f32 in every mode. */
typedef struct {
  int32_t d;             /* encoder output_size = the decoder's attention dim; a multiple of 64 */
  int32_t H;             /* decoder_conf.attention_heads; head dim d / H a multiple of 16 up to 128 */
  int32_t ff;            /* decoder_conf.linear_units; a multiple of 64 */
  int32_t num_blocks;    /* decoder_conf.num_blocks */
  int32_t r_num_blocks;  /* decoder_conf.r_num_blocks (read when the right decoder's weights are given) */
  int32_t V;             /* output_dim */
  float eps;             /* decoder_conf.norm_eps (1e-5) */
  int32_t sos, eos;      /* asr_model.py:49-58 */
  int32_t dtype;         /* cfm_dtype */
} cfm_aed_config;
typedef struct cfm_aed cfm_aed;

/* weights by reference key: decoder.left_decoder.* and, for a bitransformer, decoder.right_decoder.*:
 *   embed.0.weight [V, d], after_norm.{weight,bias}, output_layer.{weight,bias},
 *   decoders.{i}.{self_attn,src_attn}.linear_{q,k,v,out}.{weight,bias}, decoders.{i}.feed_forward.w_{1,2}.{weight,bias},
 *   decoders.{i}.norm{1,2,3}.{weight,bias}
 * (a `decoder: transformer` checkpoint's decoder.* tensors are passed under the left decoder's names; without
 * decoder.right_decoder.embed.0.weight the handle has no right decoder).  Repacked once: Q [d, d], K|V [2d, d] for
 * self- and cross-attention, 16-bit copies in the 16-bit modes; other keys (embed.1.pe among them: the
 * positional table is computed) are ignored.  Missing / mis-sized keys -> CFM_ERR_VALUE. */
cfm_status cfm_aed_create(const cfm_aed_config* cfg, const cfm_tensor_view* weights, int32_t n_weights, int32_t device,
                          cfm_aed** out);
void cfm_aed_destroy(cfm_aed* h);
size_t cfm_aed_workspace_bytes(const cfm_aed* h, int32_t tokens, int32_t mem_rows);
/* Scores every hypothesis of every utterance of a batch in one call.  Utterance u = rows [utt_row_start[u],
 * + utt_row_len[u]) of mem_dev [mem_rows, d] f32 (device int32 arrays as in cfm_ctc_collapse; zero rows: the
 * cross-attention context is exactly zero).  Hypothesis h = the packed token rows [hyp_start[h], + hyp_len[h]) of
 * tokens_dev [tokens] int32, hyp_len = its n tokens + 1: row 0 is the sos row (its content is ignored), row 1 + i
 * holds token i; hyp_utt[h] names its utterance.  Each hypothesis is a causal segment of its own (the reference's
 * padded batch with masked padding computes the same).  direction_mask bit 0: left to right, bit 1: right to left
 * (input [sos, token n-1 .. token 0], read in reverse by index; CFM_ERR_ASSERT without a right decoder).  Outputs,
 * f32 [tokens] per direction: out[hyp_start + j] = the log-prob of row j's target in that direction's own order --
 * its next input token, eos on the last row.  The per-hypothesis sums, the combination with the CTC score and the
 * argmax are the caller's (Python float64).
 * The first int32 of the workspace is a status word, zero after a complete call (1: a hypothesis' row range outside
 * [0, tokens), empty or longer than 5000; 2: its utterance index or the utterance's row range outside their arrays;
 * 3: a token id outside [0, V)); read it after the stream has completed.  A rejected hypothesis is skipped (its
 * output rows are untouched, nothing is read out of range); the others are scored as without it.  Rows of no
 * hypothesis are never written.  Stream-ordered, caller-allocated: no allocation, no host synchronisation. */
cfm_status cfm_aed_score(const cfm_aed* h, const float* mem_dev, int32_t mem_rows, const int32_t* utt_row_start_dev,
                         const int32_t* utt_row_len_dev, int32_t B, const int32_t* tokens_dev, int32_t tokens,
                         const int32_t* hyp_start_dev, const int32_t* hyp_len_dev, const int32_t* hyp_utt_dev,
                         int32_t n_hyps, int32_t direction_mask, float* tok_logp_l2r_dev, float* tok_logp_r2l_dev,
                         void* workspace, size_t workspace_bytes, cfm_stream stream);

/* ---- attention decoding mode over the same handle: the reference's autoregressive attention_beam_search
 * (modules/search.py:252-355) with the left decoder, every utterance of a masked batch at once, `beam` (1 .. 16, at
 * most V) rows each; row r = u * beam + j.  Semantics: DESIGN.md 9e.  All running utterances step together (step i
 * feeds position i - 1); an utterance stops after its own limit[u] steps or once all its beams ended with eos, and is
 * frozen from then on.  The geometry (B, beam, mem_rows, max_steps) names the layout of the caller-allocated state
 * and must be the same in every call on it; max_steps <= 5000 bounds the self-attention cache and the trace.
 * The first int32 of the state is a status word (0; 2: an utterance's row range outside the encoder rows; 5: a
 * limit outside [0, max_steps]; such an utterance is skipped, the others are unaffected), the second the number of
 * utterances still running; read them after the stream has completed.  Scores accumulate in f32. */
size_t cfm_attdec_workspace_bytes(const cfm_aed* h, int32_t B, int32_t beam, int32_t mem_rows, int32_t max_steps);
/* Validates the utterance row ranges [utt_row_start[u], + utt_row_len[u]) of mem_dev [mem_rows, d] f32 and the limits
 * on the device, projects the cross-attention K|V of every left-decoder block once over all encoder rows, and
 * writes the start state: hypotheses [sos], scores [0, -inf, ...].  The three int32 arrays are device arrays [B]. */
cfm_status cfm_attdec_begin(const cfm_aed* h, const float* mem_dev, int32_t mem_rows, const int32_t* utt_row_start_dev,
                            const int32_t* utt_row_len_dev, const int32_t* limit_dev, int32_t B, int32_t beam,
                            int32_t max_steps, void* state, size_t state_bytes, cfm_stream stream);
/* Steps first_step .. first_step + n_steps - 1 (1-based, consecutive over the calls, at most max_steps).
 * Stream-ordered: no allocation, no host synchronisation; steps of frozen utterances change nothing. */
cfm_status cfm_attdec_steps(const cfm_aed* h, void* state, int32_t B, int32_t beam, int32_t mem_rows, int32_t max_steps,
                            int32_t first_step, int32_t n_steps, cfm_stream stream);
/* Backtrace and selection.  tokens [B * beam, max_steps] int32: row r's lengths[r] tokens after the sos (eos tokens
 * included); final_scores [B * beam] f32 = score / (count of tokens != eos over the row, sos included)^length_penalty;
 * best [B]: the first maximum (a NaN counts as the maximum).  Optional trace [max_steps, B * beam] of (parent beam,
 * token, score) per step; rows of steps an utterance did not take hold (-1, -1, 0). */
cfm_status cfm_attdec_finish(const cfm_aed* h, void* state, int32_t B, int32_t beam, int32_t mem_rows, int32_t max_steps,
                             float length_penalty, int32_t* tokens_dev, int32_t* lengths_dev, float* final_scores_dev,
                             int32_t* best_dev, int32_t* trace_parent_dev, int32_t* trace_token_dev,
                             float* trace_score_dev, cfm_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* CFM_H */
