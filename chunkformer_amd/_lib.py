"""ctypes binding of libcfm.so (include/cfm.h).

The library is the product: there is no Python/CPU fallback.  If the shared
object is missing this module raises at import time, and every encoder call
goes through it.  torch is imported first so that libcfm's libamdhip64.so.7
dependency resolves to the HIP runtime torch already loaded (one runtime per
process).
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (load torch's HIP runtime before libcfm)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CFM_LIB", os.path.join(HERE, "_build", "libcfm.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError(f"libcfm.so not found at {LIB_PATH}: run `python -m chunkformer_amd.build` "
                      "(the HIP extension is required; there is no CPU fallback)")

lib = ctypes.CDLL(LIB_PATH)

P = ctypes.c_void_p
I32 = ctypes.c_int32
I64 = ctypes.c_int64
SZ = ctypes.c_size_t
PI32 = ctypes.POINTER(ctypes.c_int32)
PI64 = ctypes.POINTER(ctypes.c_int64)

CFM_OK, CFM_ERR_VALUE, CFM_ERR_ASSERT, CFM_ERR_RUNTIME = 0, 1, 2, 3
DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2
PLAN_HEADER = 16
PLAN_REC = 8


class CfmConfig(ctypes.Structure):
    _fields_ = [("input_dim", I32), ("d_model", I32), ("n_heads", I32), ("ffn_dim", I32), ("num_blocks", I32),
                ("kernel_size", I32), ("vocab", I32), ("norm_eps", ctypes.c_float), ("has_cmvn", I32),
                ("compute_dtype", I32)]


class CfmTensorView(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", P), ("numel", I64)]


def _sig(name, res, *args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


cfm_version = _sig("cfm_version", ctypes.c_char_p)
cfm_last_error = _sig("cfm_last_error", ctypes.c_char_p)
cfm_model_create = _sig("cfm_model_create", I32, ctypes.POINTER(CfmConfig), ctypes.POINTER(CfmTensorView), I32, I32,
                        ctypes.POINTER(P))
cfm_model_destroy = _sig("cfm_model_destroy", None, P)
cfm_model_set_option = _sig("cfm_model_set_option", I32, P, ctypes.c_char_p, I64)
cfm_plan_masked = _sig("cfm_plan_masked", I32, P, P, I32, I32, I32, I32, P, P, PI32, P, PI64)
cfm_plan_masked_ex = _sig("cfm_plan_masked_ex", I32, P, P, P, I32, I32, I32, I32, P, P, PI32, P, PI64)
cfm_plan_padded = _sig("cfm_plan_padded", I32, P, I32, I32, I32, I32, I32, PI32, P, PI64)
cfm_plan_stream = _sig("cfm_plan_stream", I32, I32, I32, I32, I32, I32, PI32, P, PI64)
cfm_workspace_bytes_stream = _sig("cfm_workspace_bytes_stream", SZ, P, I32, I32, I32, I32)
cfm_encode_stream = _sig("cfm_encode_stream", I32, P, P, I32, P, P, P, P, P, P, P, P, SZ, P)
cfm_workspace_bytes_masked = _sig("cfm_workspace_bytes_masked", SZ, P, I32, I32, I32, I32)
cfm_workspace_bytes_padded = _sig("cfm_workspace_bytes_padded", SZ, P, I32, I32, I32, I32, I32)
cfm_encode_masked = _sig("cfm_encode_masked", I32, P, P, P, P, P, P, I32, P, P, P, P, SZ, P)
cfm_encode_padded = _sig("cfm_encode_padded", I32, P, P, P, P, P, P, SZ, P)
cfm_encode_masked_utts = _sig("cfm_encode_masked_utts", I32, P, P, P, P, P, P, I32, P, P, P, P, SZ, P)
cfm_encode_masked_stages = _sig("cfm_encode_masked_stages", I32, P, P, P, P, P, P, I32, P, P, P, P, SZ, I32, I32, P)
cfm_masks_from_plan = _sig("cfm_masks_from_plan", I32, P, P, P, P, P)
cfm_profile_read = _sig("cfm_profile_read", I32, P, P, P, P, I32)
cfm_ctc_workspace_bytes = _sig("cfm_ctc_workspace_bytes", SZ, P, I32)
cfm_ctc_logprobs = _sig("cfm_ctc_logprobs", I32, P, P, I32, P, P, P, SZ, P)
cfm_ctc_ids_workspace_bytes = _sig("cfm_ctc_ids_workspace_bytes", SZ, P, I32)
cfm_ctc_ids = _sig("cfm_ctc_ids", I32, P, P, I32, P, P, SZ, P)
cfm_ctc_collapse = _sig("cfm_ctc_collapse", I32, P, P, P, I32, I32, I32, P, P, P, P, P, P)
# CTC prefix beam search (include/cfm.h)
cfm_ctc_topk_workspace_bytes = _sig("cfm_ctc_topk_workspace_bytes", SZ, P, I32, I32)
cfm_ctc_topk_slab_rows = _sig("cfm_ctc_topk_slab_rows", I32, P)
cfm_ctc_topk = _sig("cfm_ctc_topk", I32, P, P, I32, I32, P, P, P, SZ, P)
cfm_ctc_topk_logp = _sig("cfm_ctc_topk_logp", I32, P, I32, I32, I32, P, P, P)
cfm_ctx_create = _sig("cfm_ctx_create", I32, I32, P, P, P, P, I32, P, P, P, I32, ctypes.POINTER(P))
cfm_ctx_destroy = _sig("cfm_ctx_destroy", None, P)
cfm_ctc_beam_workspace_bytes = _sig("cfm_ctc_beam_workspace_bytes", SZ, I32, I32, I32, I32, I32)
cfm_ctc_beam_search = _sig("cfm_ctc_beam_search", I32, P, P, I32, I32, P, P, I32, I32, P, P, P, P, P, P, P, SZ, P)
# CTC forced alignment (include/cfm.h)
CFM_ALIGN_GENERIC_STRIPS = 1
cfm_ctc_align_plan = _sig("cfm_ctc_align_plan", SZ, P, P, I32, P)
cfm_ctc_align = _sig("cfm_ctc_align", I32, P, I32, I32, P, P, I32, I32, P, I32, P, P, P, P, P, P, P, P, P, P, I32, I32, P,
                     SZ, P)
# Kaldi fbank (include/cfm.h)
class CfmFbankConfig(ctypes.Structure):
    _fields_ = [("sample_frequency", ctypes.c_float), ("frame_length_ms", ctypes.c_float),
                ("frame_shift_ms", ctypes.c_float), ("num_mel_bins", I32), ("low_freq", ctypes.c_float),
                ("high_freq", ctypes.c_float), ("preemphasis_coefficient", ctypes.c_float), ("dither", ctypes.c_float),
                ("remove_dc_offset", I32), ("round_to_power_of_two", I32), ("snip_edges", I32), ("use_energy", I32),
                ("use_log_fbank", I32), ("window_type", I32)]


cfm_fbank_create = _sig("cfm_fbank_create", I32, ctypes.POINTER(CfmFbankConfig), I32, ctypes.POINTER(P))
cfm_fbank_destroy = _sig("cfm_fbank_destroy", None, P)
cfm_fbank_num_frames = _sig("cfm_fbank_num_frames", I64, P, I64)
cfm_fbank_compute = _sig("cfm_fbank_compute", I32, P, P, I64, P, P)
# RNN-T greedy search (include/cfm.h)
class CfmRnntConfig(ctypes.Structure):
    _fields_ = [("vocab", I32), ("enc_dim", I32), ("embed_size", I32), ("hidden", I32), ("num_layers", I32),
                ("pred_out", I32), ("join_dim", I32), ("blank", I32)]


cfm_rnnt_create = _sig("cfm_rnnt_create", I32, ctypes.POINTER(CfmRnntConfig), ctypes.POINTER(CfmTensorView), I32, I32,
                       ctypes.POINTER(P))


class CfmRnntPredictorConfig(ctypes.Structure):
    _fields_ = [("kind", I32), ("history_size", I32), ("n_head", I32), ("activation", I32), ("conv_bias", I32),
                ("ln_eps", ctypes.c_float)]


cfm_rnnt_create_ex = _sig("cfm_rnnt_create_ex", I32, ctypes.POINTER(CfmRnntConfig), ctypes.POINTER(CfmRnntPredictorConfig),
                          ctypes.POINTER(CfmTensorView), I32, I32, ctypes.POINTER(P))
cfm_rnnt_destroy = _sig("cfm_rnnt_destroy", None, P)
cfm_rnnt_workspace_bytes = _sig("cfm_rnnt_workspace_bytes", SZ, P, I32)
cfm_rnnt_greedy = _sig("cfm_rnnt_greedy", I32, P, P, I32, P, P, I32, I32, P, P, SZ, P)
cfm_rnnt_greedy_ex = _sig("cfm_rnnt_greedy_ex", I32, P, P, I32, P, P, I32, I32, P, P, SZ, I32, P)
CFM_RNNT_ONE_WORKGROUP = 1
cfm_rnnt_set_option = _sig("cfm_rnnt_set_option", I32, P, ctypes.c_char_p, I64)
cfm_rnnt_grid_blocks = _sig("cfm_rnnt_grid_blocks", I32, P, I32)
cfm_rnnt_error = _sig("cfm_rnnt_error", I32, P, P, I32)
# transducer prefix beam search over the same handle (csrc/rnnt_beam.hip)
F32 = ctypes.c_float
cfm_rnnt_beam_workspace_bytes = _sig("cfm_rnnt_beam_workspace_bytes", SZ, P, I32, I32, I32)
cfm_rnnt_beam_search = _sig("cfm_rnnt_beam_search", I32, P, P, I32, P, P, P, I32, I32, I32, F32, F32, P, P, P, P, P, P, P,
                            P, P, P, P, SZ, P)
cfm_rnnt_beam_error = _sig("cfm_rnnt_beam_error", I32, P)
# full-sum transducer score of given hypotheses over the same handle (csrc/rnnt_lattice.hip)
cfm_rnnt_td_workspace_bytes = _sig("cfm_rnnt_td_workspace_bytes", SZ, P, I32, I32, I32, I32, I64)
cfm_rnnt_td_score = _sig("cfm_rnnt_td_score", I32, P, P, I32, P, P, I32, P, I32, P, P, I32, I32, I64, I32, P, P, SZ, P)
# classification consumer (include/cfm.h)
CLS_MAX_TASKS = 16


class CfmClsConfig(ctypes.Structure):
    _fields_ = [("enc_dim", I32), ("n_tasks", I32), ("num_classes", I32 * CLS_MAX_TASKS)]


cfm_cls_create = _sig("cfm_cls_create", I32, ctypes.POINTER(CfmClsConfig), ctypes.POINTER(CfmTensorView), I32, I32,
                      ctypes.POINTER(P))
cfm_cls_destroy = _sig("cfm_cls_destroy", None, P)
cfm_cls_pool_workspace_bytes = _sig("cfm_cls_pool_workspace_bytes", SZ, I32, I32, I32)
cfm_cls_workspace_bytes = _sig("cfm_cls_workspace_bytes", SZ, P, I32, I32)
cfm_cls_pool = _sig("cfm_cls_pool", I32, P, I32, I32, P, P, I32, P, P, SZ, P)
cfm_cls_classify = _sig("cfm_cls_classify", I32, P, P, I32, P, P, I32, P, P, P, P, P, SZ, P)
# attention decoder consumer (include/cfm.h)
class CfmAedConfig(ctypes.Structure):
    _fields_ = [("d", I32), ("H", I32), ("ff", I32), ("num_blocks", I32), ("r_num_blocks", I32), ("V", I32),
                ("eps", ctypes.c_float), ("sos", I32), ("eos", I32), ("dtype", I32)]


cfm_aed_create = _sig("cfm_aed_create", I32, ctypes.POINTER(CfmAedConfig), ctypes.POINTER(CfmTensorView), I32, I32,
                      ctypes.POINTER(P))
cfm_aed_destroy = _sig("cfm_aed_destroy", None, P)
cfm_aed_workspace_bytes = _sig("cfm_aed_workspace_bytes", SZ, P, I32, I32)
cfm_aed_score = _sig("cfm_aed_score", I32, P, P, I32, P, P, I32, P, I32, P, P, P, I32, I32, P, P, P, SZ, P)
# attention decoding mode over the same handle (csrc/attdec.hip)
cfm_attdec_workspace_bytes = _sig("cfm_attdec_workspace_bytes", SZ, P, I32, I32, I32, I32)
cfm_attdec_begin = _sig("cfm_attdec_begin", I32, P, P, I32, P, P, P, I32, I32, I32, P, SZ, P)
cfm_attdec_steps = _sig("cfm_attdec_steps", I32, P, P, I32, I32, I32, I32, I32, I32, P)
cfm_attdec_finish = _sig("cfm_attdec_finish", I32, P, P, I32, I32, I32, I32, ctypes.c_float, P, P, P, P, P, P, P, P)
# include/cfm_ops.h
SEG_ATTN_GENERIC, SEG_ATTN_MFMA = 0, 1
DEC_ATTN_SELF_GATHER, DEC_ATTN_CROSS_GENERIC, DEC_ATTN_CROSS_MFMA = 0, 1, 2
cfm_op_decode_attention = _sig("cfm_op_decode_attention", I32, I32, I32, P, P, I32, I32, I32, I32, P, I32, P, I32, I32, P,
                               P, I32, P, P)
cfm_op_seg_attention = _sig("cfm_op_seg_attention", I32, I32, I32, P, I32, P, I32, P, I32, I32, I32, P, P, P)
cfm_op_gemm = _sig("cfm_op_gemm", I32, I32, I32, I32, P, I32, P, I32, I32, I32, I32, P, ctypes.c_float, P, I32, I32, P,
                   I32, P, I32, P, I32, P)
GEMM_NONE, GEMM_128, GEMM_256, GEMM_WST = 0, 1, 2, 3
cfm_op_gemm_route = _sig("cfm_op_gemm_route", I32, I32, I32, I32, I32, I32, I32, I32, I32, I32, I32, I32, I32)
ATTN_GENERIC, ATTN_RING, ATTN_A128, ATTN_DENSE = 0, 1, 2, 3
cfm_op_attention = _sig("cfm_op_attention", I32, I32, I32, P, P, I32, P, I32, I32, P, P, P, I32, I32, I32, I32, I32, P,
                        I32, P, I32, I32, I32, I32, P)
LN, LN2, LN2_F32 = 0, 1, 2
cfm_op_layernorm = _sig("cfm_op_layernorm", I32, I32, I32, P, I32, I32, P, ctypes.c_float, P, P, ctypes.c_float, P, I32, P,
                        P, P, P, ctypes.c_float, P, P, P)
cfm_op_conv_module = _sig("cfm_op_conv_module", I32, I32, P, P, I32, I32, P, P, P, P, ctypes.c_float, P, P)
cfm_op_pos_table = _sig("cfm_op_pos_table", I32, I32, I32, I32, I32, P, P)
FE_VALU, FE_MFMA_POS, FE_MFMA_CH = 0, 1, 2
cfm_op_frontend_conv0_dw = _sig("cfm_op_frontend_conv0_dw", I32, P, I32, I32, I32, P, P, I32, P, I32, I32, P, P)
FE_DW2_UNFUSED, FE_DW2_FUSED = 0, 1
cfm_op_frontend_dw2 = _sig("cfm_op_frontend_dw2", I32, P, I32, P, I32, I32, I32, P, P)
cfm_op_rnnt_fused_topk = _sig("cfm_op_rnnt_fused_topk", I32, P, P, I32, I32, I32, F32, F32, P, P, P)
cfm_op_rnnt_beam_prune_workspace_bytes = _sig("cfm_op_rnnt_beam_prune_workspace_bytes", SZ, I32, I32)
cfm_op_rnnt_beam_prune = _sig("cfm_op_rnnt_beam_prune", I32, P, P, I32, I32, I32, P, P, P, P, P, SZ, P)
cfm_op_rnnt_lstm_step_workspace_bytes = _sig("cfm_op_rnnt_lstm_step_workspace_bytes", SZ, P, I32)
cfm_op_rnnt_lstm_step = _sig("cfm_op_rnnt_lstm_step", I32, P, P, P, P, I32, P, P, P, P, SZ, P)
cfm_op_rnnt_predictor_step_workspace_bytes = _sig("cfm_op_rnnt_predictor_step_workspace_bytes", SZ, P, I32)
cfm_op_rnnt_predictor_step = _sig("cfm_op_rnnt_predictor_step", I32, P, P, I32, P, P, P, SZ, P)
cfm_op_rnnt_lattice = _sig("cfm_op_rnnt_lattice", I32, P, I32, P, I32, P, I32, P, P, P, I32, P, P, I32, I64, P, P, P)
cfm_op_rnnt_alpha_workspace_bytes = _sig("cfm_op_rnnt_alpha_workspace_bytes", SZ, I32, I32)
cfm_op_rnnt_alpha = _sig("cfm_op_rnnt_alpha", I32, P, P, P, P, P, I32, I32, I64, P, P, SZ, P)
EXPORTED_OPS = ["cfm_op_gemm", "cfm_op_gemm_route", "cfm_op_attention", "cfm_op_layernorm", "cfm_op_conv_module", "cfm_op_pos_table",
                "cfm_op_frontend_conv0_dw", "cfm_op_frontend_dw2", "cfm_op_seg_attention", "cfm_op_decode_attention",
                "cfm_op_rnnt_fused_topk", "cfm_op_rnnt_beam_prune_workspace_bytes", "cfm_op_rnnt_beam_prune",
                "cfm_op_rnnt_lstm_step_workspace_bytes", "cfm_op_rnnt_lstm_step",
                "cfm_op_rnnt_predictor_step_workspace_bytes", "cfm_op_rnnt_predictor_step",
                "cfm_op_rnnt_lattice", "cfm_op_rnnt_alpha_workspace_bytes", "cfm_op_rnnt_alpha"]

EXPORTED = ["cfm_version", "cfm_last_error", "cfm_model_create", "cfm_model_destroy", "cfm_model_set_option",
            "cfm_plan_masked", "cfm_plan_masked_ex", "cfm_plan_padded", "cfm_workspace_bytes_masked", "cfm_workspace_bytes_padded",
            "cfm_encode_masked", "cfm_encode_masked_utts", "cfm_encode_masked_stages", "cfm_encode_padded", "cfm_masks_from_plan", "cfm_profile_read", "cfm_ctc_workspace_bytes",
            "cfm_ctc_logprobs", "cfm_ctc_ids_workspace_bytes", "cfm_ctc_ids", "cfm_ctc_collapse",
            "cfm_plan_stream", "cfm_workspace_bytes_stream", "cfm_encode_stream",
            "cfm_fbank_create", "cfm_fbank_destroy", "cfm_fbank_num_frames", "cfm_fbank_compute",
            "cfm_rnnt_create", "cfm_rnnt_create_ex", "cfm_rnnt_destroy", "cfm_rnnt_workspace_bytes", "cfm_rnnt_greedy",
            "cfm_rnnt_greedy_ex", "cfm_rnnt_set_option", "cfm_rnnt_grid_blocks", "cfm_rnnt_error",
            "cfm_rnnt_beam_workspace_bytes", "cfm_rnnt_beam_search", "cfm_rnnt_beam_error",
            "cfm_rnnt_td_workspace_bytes", "cfm_rnnt_td_score",
            "cfm_cls_create", "cfm_cls_destroy", "cfm_cls_pool_workspace_bytes", "cfm_cls_workspace_bytes",
            "cfm_cls_pool", "cfm_cls_classify",
            "cfm_ctc_topk_workspace_bytes", "cfm_ctc_topk_slab_rows", "cfm_ctc_topk", "cfm_ctc_topk_logp",
            "cfm_ctx_create", "cfm_ctx_destroy", "cfm_ctc_beam_workspace_bytes", "cfm_ctc_beam_search",
            "cfm_ctc_align_plan", "cfm_ctc_align",
            "cfm_aed_create", "cfm_aed_destroy", "cfm_aed_workspace_bytes", "cfm_aed_score",
            "cfm_attdec_workspace_bytes", "cfm_attdec_begin", "cfm_attdec_steps", "cfm_attdec_finish"]


def profile_read(h):
    """{kernel class: (total_ms, launches)} accumulated by the in-stream event profiler."""
    cap = 32
    names = (ctypes.c_char_p * cap)()
    ms = (ctypes.c_double * cap)()
    n = (ctypes.c_int64 * cap)()
    k = cfm_profile_read(h, ctypes.cast(names, P), ctypes.cast(ms, P), ctypes.cast(n, P), cap)
    return {names[i].decode(): (ms[i], n[i]) for i in range(min(k, cap))}


PROFILE_CLASSES = ["frontend_conv0_dw", "frontend_pw_gemm", "frontend_dw2", "pos_gemm", "layernorm", "ffn_w1_gemm",
                   "ffn_w2_gemm", "qkv_gemm", "chunk_attention", "out_proj_gemm", "pw1_glu_gemm", "conv_dw_ln_silu",
                   "pw2_gemm", "cache_copy", "ctc"]


def check(status: int) -> None:
    """Map a cfm_status to the reference's exception types (include/cfm.h)."""
    if status == CFM_OK:
        return
    msg = (cfm_last_error() or b"").decode(errors="replace")
    if status == CFM_ERR_VALUE:
        raise ValueError(msg)
    if status == CFM_ERR_ASSERT:
        raise AssertionError(msg)
    raise RuntimeError(msg)


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def i32_host(values) -> torch.Tensor:
    """Row starts, lengths and the like (any iterable of integer-likes) as an int32 CPU tensor."""
    return torch.tensor([int(v) for v in values], dtype=torch.int32)


def packed_ranges(row_start, row_len, rows: int, what: str):
    """The utterances of a packed batch, utterance b = rows [row_start[b], row_start[b] + row_len[b]) of `rows` rows,
    as two int32 CPU tensors; ValueError when the two differ in length or a range is negative or runs past `rows`
    (`what` names the packed tensor in the message)."""
    rs, rl = [int(v) for v in row_start], [int(v) for v in row_len]
    if len(rs) != len(rl) or any(s < 0 or n < 0 or s + n > rows for s, n in zip(rs, rl)):
        raise ValueError(f"utterance row ranges exceed the {what}")
    return torch.tensor(rs, dtype=torch.int32), torch.tensor(rl, dtype=torch.int32)


def plan_masked(lens, offsets, C: int, L: int, R: int, mask_lens=None):
    """Host planner (no GPU): returns (plan int32 CPU tensor, n_chunks list, out_lens list).
    lens: feature rows per utterance; mask_lens: xs_origin_lens when it differs (None = lens)."""
    B = len(lens)
    lens_t = i32_host(lens)
    ml_t = i32_host(mask_lens) if mask_lens is not None else None
    offs_t = i32_host(offsets) if offsets is not None else None
    nch = torch.zeros(B, dtype=torch.int32)
    olen = torch.zeros(B, dtype=torch.int32)
    total = I32(0)
    n = I64(0)
    check(cfm_plan_masked_ex(lens_t.data_ptr(), ptr(ml_t), ptr(offs_t), B, C, L, R, nch.data_ptr(), olen.data_ptr(),
                             ctypes.byref(total), None, ctypes.byref(n)))
    plan = torch.zeros(n.value, dtype=torch.int32)
    check(cfm_plan_masked_ex(lens_t.data_ptr(), ptr(ml_t), ptr(offs_t), B, C, L, R, None, None, ctypes.byref(total),
                             plan.data_ptr(), ctypes.byref(n)))
    return plan, nch.tolist(), olen.tolist()


def plan_stream(T: int, C: int, L: int, R: int, offset: int):
    """Host planner of one forward_chunk step (no GPU): returns (plan int32 CPU tensor, T')."""
    tout = I32(0)
    n = I64(0)
    check(cfm_plan_stream(int(T), int(C), int(L), int(R), int(offset), ctypes.byref(tout), None, ctypes.byref(n)))
    plan = torch.zeros(n.value, dtype=torch.int32)
    check(cfm_plan_stream(int(T), int(C), int(L), int(R), int(offset), ctypes.byref(tout), plan.data_ptr(),
                          ctypes.byref(n)))
    return plan, tout.value


def plan_padded(lens, T: int, C: int, L: int, R: int):
    B = len(lens)
    lens_t = i32_host(lens)
    tout = I32(0)
    n = I64(0)
    check(cfm_plan_padded(lens_t.data_ptr(), B, T, C, L, R, ctypes.byref(tout), None, ctypes.byref(n)))
    plan = torch.zeros(n.value, dtype=torch.int32)
    check(cfm_plan_padded(lens_t.data_ptr(), B, T, C, L, R, ctypes.byref(tout), plan.data_ptr(), ctypes.byref(n)))
    return plan, tout.value
