"""Attention rescoring of the CTC prefix beam n-best with the checkpoint's attention decoder.

The reference's `attention_rescoring` decoding mode (modules/search.py:358-439 over
ASRModel.forward_attention_decoder, asr_model.py:399-492, with TransformerDecoder /
BiTransformerDecoder of modules/decoder.py and DecoderLayer of modules/decoder_layer.py), dropout off,
the `normalize_before=True` path:

    x = embed[token] * sqrt(d) + pe[pos]                       (embedding.py:31-58, max_len 5000)
    per block:  x += SelfAttn(LN1(x))  causal;  x += SrcAttn(LN2(x), memory);  x += W2 ReLU(W1 LN3(x))
    logp = log_softmax(output_layer(after_norm(x)))

Left to right, hypothesis h of n tokens is the input [sos, h_0 .. h_{n-1}] and scores
sum_j logp[j][h_j] + logp[n][eos]; right to left the input is [sos, h_{n-1} .. h_0] through
right_decoder and the score sum_j r_logp[n-1-j][h_j] + r_logp[n][eos].

The reference pads one utterance's hypotheses to a common length, repeats the encoder output once per
hypothesis and builds [n_hyps, L, V] log-softmax tensors it then reads single elements of.  Here every
hypothesis is its own causal segment of n + 1 packed token rows (the same result: padded keys are
masked there), the encoder rows are shared by all hypotheses of an utterance, and the decoder writes
one float per token row: the log-prob of that row's target (the next token, or eos on the last row).

Two implementations share this formulation:
  - device: AttentionRescorer over cfm_aed_* (csrc/aed.hip): embedding, segment attention and output
    head kernels around the library's GEMM and LayerNorm launchers, one call per masked batch;
  - CPU tensors: `score_host` / `rescore_host`, a torch restatement in f32 or f64 (the checker of the
    tests, and what runs when the encoder rows are on the CPU).
The short per-hypothesis sums, the combination with the CTC score and the argmax are Python float64
in both.
"""
from __future__ import annotations

import ctypes
import math
import weakref
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .search import DecodeResult

MAX_POSITIONS = 5000   # PositionalEncoding max_len (embedding.py:22)
LEFT, RIGHT = "decoder.left_decoder.", "decoder.right_decoder."


@dataclass
class AEDConfig:
    vocab: int = 5000
    d_model: int = 256
    heads: int = 4              # decoder_conf.attention_heads
    ff: int = 2048              # decoder_conf.linear_units
    num_blocks: int = 3         # decoder_conf.num_blocks
    r_num_blocks: int = 3       # decoder_conf.r_num_blocks (bitransformer only)
    eps: float = 1e-5           # decoder_conf.norm_eps
    sos: int = -1               # tokenizer_conf.special_tokens["<sos>"], default vocab - 1 (asr_model.py:49-58)
    eos: int = -1
    bidirectional: bool = True  # decoder: bitransformer (keys decoder.left_decoder.* / decoder.right_decoder.*)
    ctc_weight: float = 0.5     # model_conf.ctc_weight (ASRModel default)
    reverse_weight: float = 0.0  # model_conf.reverse_weight

    def __post_init__(self):
        if self.sos < 0:
            self.sos = self.vocab - 1
        if self.eos < 0:
            self.eos = self.vocab - 1

    @property
    def has_right(self) -> bool:
        """A right decoder exists (a bitransformer's runs even with r_num_blocks 0: embedding, after_norm, output)."""
        return self.bidirectional

    @classmethod
    def from_conf(cls, conf: dict, vocab: int, d_model: int) -> "AEDConfig":
        """From a reference config.yaml (init_model.py:81-143).  Unsupported decoder settings raise
        AssertionError, the way transducer.py treats unsupported predictors."""
        kind = conf.get("decoder", "transformer")
        assert kind in ("transformer", "bitransformer"), f"decoder: {kind} is not transformer / bitransformer"
        dc = dict(conf.get("decoder_conf") or {})
        mc = dict(conf.get("model_conf") or {})
        assert dc.get("normalize_before", True), "decoder normalize_before: false is not supported"
        assert dc.get("layer_norm_type", "layer_norm") == "layer_norm", "decoder rms_norm is not supported"
        assert not dc.get("use_sdpa", False), "decoder use_sdpa is not supported"
        assert dc.get("n_kv_head") is None and dc.get("head_dim") is None, "decoder n_kv_head / head_dim is not supported"
        assert dc.get("mlp_type", "position_wise_feed_forward") == "position_wise_feed_forward", \
            "only the position-wise feed-forward decoder MLP is supported"
        assert dc.get("activation_type", "relu") == "relu", "only activation_type relu is supported in the decoder"
        assert not dc.get("tie_word_embedding", False), "decoder tie_word_embedding is not supported"
        assert dc.get("src_attention", True), "decoder src_attention: false is not supported"
        assert dc.get("input_layer", "embed") == "embed", "only the embed decoder input layer is supported"
        assert dc.get("use_output_layer", True), "a decoder without output layer cannot rescore"
        for k in ("query_bias", "key_bias", "value_bias", "mlp_bias", "src_query_bias", "src_key_bias", "src_value_bias"):
            assert dc.get(k, True), f"decoder {k}: false is not supported"
        sp = (conf.get("tokenizer_conf") or {}).get("special_tokens", None)
        sos = vocab - 1 if sp is None else int(sp.get("<sos>", vocab - 1))
        eos = vocab - 1 if sp is None else int(sp.get("<eos>", vocab - 1))
        bi = kind == "bitransformer"
        c = cls(vocab=int(vocab), d_model=int(d_model), heads=int(dc.get("attention_heads", 4)),
                ff=int(dc.get("linear_units", 2048)), num_blocks=int(dc.get("num_blocks", 6)),
                r_num_blocks=int(dc.get("r_num_blocks", 0)) if bi else 0, eps=float(dc.get("norm_eps", 1e-5)),
                sos=sos, eos=eos, bidirectional=bi, ctc_weight=float(mc.get("ctc_weight", 0.5)),
                reverse_weight=float(mc.get("reverse_weight", 0.0)))
        c.validate()
        return c

    def validate(self) -> None:
        assert self.vocab > 1 and 0 <= self.sos < self.vocab and 0 <= self.eos < self.vocab
        assert self.heads >= 1 and self.d_model % self.heads == 0, "d_model must divide into the heads"
        dk = self.d_model // self.heads
        assert dk % 16 == 0 and dk <= 128, "decoder head dim: a multiple of 16 up to 128"
        assert self.d_model % 64 == 0 and self.ff % 64 == 0, "decoder widths must be multiples of 64"
        assert self.num_blocks >= 0 and self.r_num_blocks >= 0


def _decoder_schema(p: str, c: AEDConfig, nb: int) -> List[Tuple[str, Tuple[int, ...]]]:
    d, ff, V = c.d_model, c.ff, c.vocab
    out = [(p + "embed.0.weight", (V, d)), (p + "after_norm.weight", (d,)), (p + "after_norm.bias", (d,)),
           (p + "output_layer.weight", (V, d)), (p + "output_layer.bias", (V,))]
    for i in range(nb):
        q = f"{p}decoders.{i}."
        for att in ("self_attn", "src_attn"):
            for lin in ("linear_q", "linear_k", "linear_v", "linear_out"):
                out += [(f"{q}{att}.{lin}.weight", (d, d)), (f"{q}{att}.{lin}.bias", (d,))]
        out += [(q + "feed_forward.w_1.weight", (ff, d)), (q + "feed_forward.w_1.bias", (ff,)),
                (q + "feed_forward.w_2.weight", (d, ff)), (q + "feed_forward.w_2.bias", (d,))]
        for n in ("norm1", "norm2", "norm3"):
            out += [(f"{q}{n}.weight", (d,)), (f"{q}{n}.bias", (d,))]
    return out


def schema(c: AEDConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of every decoder tensor, keys as in the reference ASRModel state dict: decoder.* for
    `decoder: transformer`, decoder.left_decoder.* / decoder.right_decoder.* for bitransformer (whose right
    decoder keeps its embedding, after_norm and output layer even with r_num_blocks 0).  The `embed.1.pe`
    buffers are not part of it: the table is computed."""
    if not c.bidirectional:
        return _decoder_schema("decoder.", c, c.num_blocks)
    return _decoder_schema(LEFT, c, c.num_blocks) + _decoder_schema(RIGHT, c, c.r_num_blocks)


def synthetic_decoder_state_dict(c: AEDConfig, seed: int = 0, logit_scale: float = 3.0
                                 ) -> "OrderedDict[str, torch.Tensor]":
    """Seeded decoder weights with the reference modules' default init magnitudes (Embedding N(0, 1) scaled
    by 1 / sqrt(d) so that x has unit scale after the sqrt(d) factor, Linear U(+-1/sqrt(fan_in)), LayerNorm
    weights near 1), the output layer scaled by `logit_scale` so that the log-probs depend on the context."""
    g = torch.Generator().manual_seed(seed)
    sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    shapes = dict(schema(c))
    for name, shape in schema(c):
        if name.endswith("embed.0.weight"):
            t = torch.randn(shape, generator=g) / math.sqrt(c.d_model)
        elif "norm" in name:
            t = (1.0 + 0.1 * torch.randn(shape, generator=g)) if name.endswith("weight") else 0.1 * torch.randn(shape, generator=g)
        else:
            fan = shapes[name[: -len("bias")] + "weight"][1] if name.endswith("bias") else shape[1]
            t = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan)
            if "output_layer" in name:
                t = t * logit_scale
        sd[name] = t.contiguous()
    return sd


def native_names(c: AEDConfig, sd: Dict[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
    """The decoder tensors under the keys the native layer takes (decoder.left_decoder.* / decoder.right_decoder.*);
    a `decoder: transformer` checkpoint's decoder.* keys become the left decoder.  Missing or mis-shaped: KeyError /
    ValueError."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for name, shape in schema(c):
        if name not in sd:
            raise KeyError(f"missing weight {name}")
        if tuple(sd[name].shape) != tuple(shape):
            raise ValueError(f"weight {name}: shape {tuple(sd[name].shape)} != {shape}")
        key = name if c.bidirectional else LEFT + name[len("decoder."):]
        out[key] = sd[name]
    return out


def positional_table(d: int, n: int = MAX_POSITIONS, dtype=torch.float32) -> torch.Tensor:
    """PositionalEncoding.pe[0, :n] as the reference builds it (embedding.py:31-38, f32 arithmetic)."""
    pe = torch.zeros(n, d)
    position = torch.arange(0, n, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.to(dtype)


# ------------------------------------------------------------------------------------ host restatement
def _ln(x, w, b, eps):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, eps)


def _mha(W, p: str, q_in, kv_in, mask, H: int):
    """MultiHeadedAttention.forward (attention.py:104-150, 199-219): q_in [B, Lq, d], kv_in [B, Lk, d], mask
    [B, Lq or 1, Lk] bool (True = visible); rows without a visible key give a zero context."""
    B, Lq, d = q_in.shape
    Lk = kv_in.shape[1]
    dk = d // H
    lin = lambda n, x: torch.nn.functional.linear(x, W[p + n + ".weight"], W[p + n + ".bias"])   # noqa: E731
    q = lin("linear_q", q_in).view(B, Lq, H, dk).transpose(1, 2)
    k = lin("linear_k", kv_in).view(B, Lk, H, dk).transpose(1, 2)
    v = lin("linear_v", kv_in).view(B, Lk, H, dk).transpose(1, 2)
    scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(dk)
    if Lk > 0:
        m = ~mask.unsqueeze(1)
        scores = scores.masked_fill(m, float("-inf"))
        attn = torch.softmax(scores, dim=-1).masked_fill(m, 0.0)
        attn = torch.nan_to_num(attn, nan=0.0)   # a row with no visible key: softmax of all -inf
        ctx = torch.matmul(attn, v)
    else:
        ctx = torch.zeros(B, H, Lq, dk, dtype=q.dtype, device=q.device)
    return lin("linear_out", ctx.transpose(1, 2).reshape(B, Lq, d))


def decoder_logp_padded(W: Dict[str, torch.Tensor], p: str, c: AEDConfig, nb: int, ys_in: torch.Tensor,
                        ys_lens: Sequence[int], memory: torch.Tensor, pe: torch.Tensor) -> torch.Tensor:
    """TransformerDecoder.forward (decoder.py:173-226) + log_softmax on a padded batch: ys_in [B, L] int64 (padding
    beyond ys_lens[b] is any valid id), memory [T, d] shared by the batch -> [B, L, V] log-probs.  Runs where
    its tensors live (tools/bench_rescore.py times it on the GPU as the reference's formulation)."""
    B, L = ys_in.shape
    dev = memory.device
    lens = torch.as_tensor(list(ys_lens), dtype=torch.long, device=dev)
    key_ok = torch.arange(L, device=dev).unsqueeze(0) < lens.unsqueeze(1)        # [B, L]
    tgt_mask = key_ok.unsqueeze(1) & torch.tril(torch.ones(L, L, dtype=torch.bool, device=dev)).unsqueeze(0)
    mem = memory.unsqueeze(0).expand(B, -1, -1)     # (the reference repeats it: asr_model.py:425)
    mem_mask = torch.ones(B, 1, memory.shape[0], dtype=torch.bool, device=dev)
    x = W[p + "embed.0.weight"][ys_in] * math.sqrt(c.d_model) + pe[:L].unsqueeze(0)
    for i in range(nb):
        q = f"{p}decoders.{i}."
        h = _ln(x, W[q + "norm1.weight"], W[q + "norm1.bias"], c.eps)
        x = x + _mha(W, q + "self_attn.", h, h, tgt_mask, c.heads)
        h = _ln(x, W[q + "norm2.weight"], W[q + "norm2.bias"], c.eps)
        x = x + _mha(W, q + "src_attn.", h, mem, mem_mask, c.heads)
        h = _ln(x, W[q + "norm3.weight"], W[q + "norm3.bias"], c.eps)
        h = torch.relu(torch.nn.functional.linear(h, W[q + "feed_forward.w_1.weight"], W[q + "feed_forward.w_1.bias"]))
        x = x + torch.nn.functional.linear(h, W[q + "feed_forward.w_2.weight"], W[q + "feed_forward.w_2.bias"])
    x = _ln(x, W[p + "after_norm.weight"], W[p + "after_norm.bias"], c.eps)
    logits = torch.nn.functional.linear(x, W[p + "output_layer.weight"], W[p + "output_layer.bias"])
    return torch.log_softmax(logits, dim=-1)


def _check_hyps(c: AEDConfig, nbest: Sequence[Sequence[Sequence[int]]]) -> None:
    for hyps in nbest:
        for h in hyps:
            if len(h) + 1 > MAX_POSITIONS:
                raise ValueError(f"a hypothesis of {len(h)} tokens exceeds the decoder's {MAX_POSITIONS} positions")
            if any(int(t) < 0 or int(t) >= c.vocab for t in h):
                raise ValueError("a hypothesis holds a token id outside [0, vocab)")


def use_right(c: AEDConfig, reverse_weight: float) -> bool:
    """The right decoder runs and counts: reverse_weight > 0 on a bitransformer (search.py:414; a
    `decoder: transformer` returns a 0-dim r_decoder_out)."""
    return reverse_weight > 0 and c.bidirectional


def score_host(c: AEDConfig, sd: Dict[str, torch.Tensor], enc_rows: torch.Tensor, row_start, row_len,
               nbest: Sequence[Sequence[Sequence[int]]], right: bool = True, dtype=torch.float32):
    """Per utterance b (encoder rows [row_start[b], + row_len[b]) of enc_rows [rows, d]) and hypothesis: the packed
    formulation on the CPU.  Returns out[b][i] = (l2r [n + 1], r2l [n + 1] or None): l2r[j] = logp[j][h_j] for j < n and
    l2r[n] = logp[n][eos]; r2l[j] = r_logp[j][h_{n-1-j}] (in the right decoder's own order) and r2l[n] = r_logp[n][eos]."""
    _check_hyps(c, nbest)
    W = {k: v.detach().to("cpu", dtype) for k, v in native_names(c, sd).items()}
    pe = positional_table(c.d_model, MAX_POSITIONS, dtype)
    enc = enc_rows.detach().to("cpu", dtype)
    right = right and c.bidirectional
    out = []
    for b, hyps in enumerate(nbest):
        mem = enc[int(row_start[b]): int(row_start[b]) + int(row_len[b])]
        res = []
        for h in hyps:
            n = len(h)
            per_dir = []
            for p, nb, seq in ((LEFT, c.num_blocks, list(h)), (RIGHT, c.r_num_blocks, list(h)[::-1])):
                if p == RIGHT and not right:
                    per_dir.append(None)
                    continue
                ys = torch.tensor([[c.sos] + [int(t) for t in seq]], dtype=torch.long)
                lp = decoder_logp_padded(W, p, c, nb, ys, [n + 1], mem, pe)[0]
                tgt = torch.tensor([int(t) for t in seq] + [c.eos], dtype=torch.long)
                per_dir.append(lp[torch.arange(n + 1), tgt])
            res.append((per_dir[0], per_dir[1]))
        out.append(res)
    return out


def combine(c: AEDConfig, scored, results: Sequence[DecodeResult], ctc_weight: float, reverse_weight: float,
            return_nbest: bool = False) -> List[DecodeResult]:
    """search.py:400-438 from the per-row target log-probs, in Python float64.  `scored[b][i]` = (l2r, r2l) as
    score_host / AttentionRescorer.score return them.  The chosen hypothesis is the first with a strictly larger
    total.  The result carries the rescored totals of the whole list in `nbest_scores` (with `return_nbest` the
    n-best re-ranked by them, ties in n-best order) and the chosen index in `best_index`."""
    rev = use_right(c, reverse_weight)
    out = []
    for res, sc in zip(results, scored):
        hyps, ctc_scores = res.nbest, res.nbest_scores
        if hyps is None or ctc_scores is None:
            raise ValueError("attention rescoring needs the n-best of ctc_prefix_beam_search")
        totals, confs, tcs, dec = [], [], [], []
        for i, h in enumerate(hyps):
            n = len(h)
            l2r = [float(v) for v in sc[i][0].tolist()]
            score = math.fsum(l2r)
            tc = [math.exp(v) for v in l2r[:n]]
            if rev:
                if sc[i][1] is None:
                    raise ValueError("reverse_weight > 0 needs the right decoder's scores")
                r2l = [float(v) for v in sc[i][1].tolist()]
                tc = [(tc[j] + math.exp(r2l[n - 1 - j])) / 2 for j in range(n)]
                score = score * (1 - reverse_weight) + math.fsum(r2l) * reverse_weight
            dec.append(score)
            confs.append(math.exp(score / (n + 1)))
            totals.append(score + float(ctc_scores[i]) * ctc_weight)
            tcs.append(tc)
        best = 0
        for i in range(1, len(totals)):
            if totals[i] > totals[best]:
                best = i
        times = res.nbest_times
        order = sorted(range(len(hyps)), key=lambda i: -totals[i]) if return_nbest else list(range(len(hyps)))
        r = DecodeResult(list(hyps[best]), totals[best], confidence=confs[best], tokens_confidence=tcs[best],
                         times=times[best] if times is not None else None,
                         nbest=[hyps[i] for i in order], nbest_scores=[totals[i] for i in order],
                         nbest_times=[times[i] for i in order] if times is not None else None)
        r.best_index = best
        r.decoder_scores = dec
        out.append(r)
    return out


def rescore_host(c: AEDConfig, sd: Dict[str, torch.Tensor], enc_rows: torch.Tensor, row_start, row_len,
                 results: Sequence[DecodeResult], ctc_weight: Optional[float] = None,
                 reverse_weight: Optional[float] = None, dtype=torch.float32, return_nbest: bool = False
                 ) -> List[DecodeResult]:
    """attention_rescoring on the CPU: `results` are the prefix beam search's DecodeResults (nbest, nbest_scores,
    nbest_times) of the utterances whose encoder rows are [row_start[b], + row_len[b]) of enc_rows."""
    cw = c.ctc_weight if ctc_weight is None else float(ctc_weight)
    rw = c.reverse_weight if reverse_weight is None else float(reverse_weight)
    scored = score_host(c, sd, enc_rows, row_start, row_len, [r.nbest for r in results], use_right(c, rw), dtype)
    return combine(c, scored, results, cw, rw, return_nbest)


# ------------------------------------------------------------------------------------ device
_DT = {"fp32": 0, "bf16": 1, "fp16": 2}
_STATUS = {1: "a hypothesis' row range lies outside the token rows, or is longer than the decoder's positions",
           2: "an utterance's row range lies outside the encoder rows, or a hypothesis names no utterance",
           3: "a token id lies outside [0, vocab)"}


class AttentionRescorer:
    """Owns a cfm_aed handle: the decoder weights repacked on the device (csrc/aed.hip)."""

    def __init__(self, cfg: AEDConfig, state_dict: Dict[str, torch.Tensor], device, dtype: str = "bf16"):
        from . import _lib
        cfg.validate()
        if dtype not in _DT:
            raise ValueError(f"dtype {dtype!r}: fp32, bf16 or fp16")
        self.cfg, self.dtype = cfg, dtype
        self.device = torch.device(device)
        named = native_names(cfg, state_dict)
        c = _lib.CfmAedConfig(cfg.d_model, cfg.heads, cfg.ff, cfg.num_blocks, cfg.r_num_blocks if cfg.has_right else 0,
                              cfg.vocab, cfg.eps, cfg.sos, cfg.eos, _DT[dtype])
        keep = []
        views = (_lib.CfmTensorView * len(named))()
        for i, (k, v) in enumerate(named.items()):
            t = v.detach().to("cpu", torch.float32).contiguous()
            keep.append(t)
            views[i] = _lib.CfmTensorView(k.encode(), t.data_ptr(), t.numel())
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.cfm_aed_create(ctypes.byref(c), views, len(named), self.device.index or 0, ctypes.byref(h)))
        self._h = h
        self._finalizer = weakref.finalize(self, _lib.cfm_aed_destroy, ctypes.c_void_p(h.value))

    @torch.no_grad()
    def score(self, enc_rows: torch.Tensor, row_start, row_len, nbest: Sequence[Sequence[Sequence[int]]],
              right: bool = True, check_host: bool = True):
        """One cfm_aed_score call over the packed encoder rows enc_rows [rows, d] (utterance b = rows
        [row_start[b], + row_len[b])) and every hypothesis of every utterance.  Returns out[b][i] = (l2r, r2l or
        None) as score_host does, as CPU f32 tensors.  A bad descriptor or token id raises ValueError after the
        call (`check_host` False leaves the checks to the device's status word; the outputs of the other
        hypotheses are in `last_scores`)."""
        from . import _lib
        c, dev = self.cfg, self.device
        if check_host:
            _check_hyps(c, nbest)
        enc = enc_rows.reshape(-1, c.d_model).to(dev, torch.float32).contiguous()
        rows, B = enc.shape[0], len(nbest)
        if check_host:
            rs, rl = _lib.packed_ranges(row_start, row_len, rows, "encoder rows")
        else:
            rs, rl = _lib.i32_host(row_start), _lib.i32_host(row_len)
        right = bool(right) and c.has_right
        toks, hs, hl, hu = [], [], [], []
        for b, hyps in enumerate(nbest):
            for h in hyps:
                hs.append(len(toks))
                hl.append(len(h) + 1)
                hu.append(b)
                toks.append(c.sos)
                toks.extend(int(t) for t in h)
        n_tok, n_hyp = len(toks), len(hs)
        l2r = torch.zeros(max(n_tok, 1), dtype=torch.float32, device=dev)
        r2l = torch.zeros(max(n_tok, 1), dtype=torch.float32, device=dev) if right else None
        if n_hyp:
            i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)   # noqa: E731
            tok_d, hs_d, hl_d, hu_d, rs_d, rl_d = i32(toks), i32(hs), i32(hl), i32(hu), rs.to(dev), rl.to(dev)
            nbytes = int(_lib.cfm_aed_workspace_bytes(self._h, n_tok, rows))
            ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.cfm_aed_score(self._h, enc.data_ptr(), rows, rs_d.data_ptr(), rl_d.data_ptr(), B,
                                              tok_d.data_ptr(), n_tok, hs_d.data_ptr(), hl_d.data_ptr(), hu_d.data_ptr(),
                                              n_hyp, 3 if right else 1, l2r.data_ptr(), _lib.ptr(r2l), ws.data_ptr(),
                                              nbytes, torch.cuda.current_stream(dev).cuda_stream))
            status = int(ws[:4].view(torch.int32).item())   # synchronises: the inputs above are consumed
            self.last_workspace_bytes = nbytes
        else:
            status = 0
        l_h = l2r.cpu()
        r_h = r2l.cpu() if right else None
        out, k = [], 0
        for hyps in nbest:
            res = []
            for h in hyps:
                s, n1 = hs[k], hl[k]
                res.append((l_h[s: s + n1], r_h[s: s + n1] if right else None))
                k += 1
            out.append(res)
        self.last_scores = out
        if status != 0:
            raise ValueError(f"attention rescoring failed (status {status}): {_STATUS.get(status, 'internal')}")
        return out

    def rescore(self, results: Sequence[DecodeResult], enc_rows: torch.Tensor, row_start, row_len,
                ctc_weight: Optional[float] = None, reverse_weight: Optional[float] = None,
                return_nbest: bool = False) -> List[DecodeResult]:
        """attention_rescoring (search.py:358-439) of the prefix beam search's `results` for the utterances whose
        encoder rows are [row_start[b], + row_len[b]) of enc_rows: DecodeResults with the reference's fields."""
        c = self.cfg
        cw = c.ctc_weight if ctc_weight is None else float(ctc_weight)
        rw = c.reverse_weight if reverse_weight is None else float(reverse_weight)
        for r in results:
            if r.nbest is None or r.nbest_scores is None:
                raise ValueError("attention rescoring needs the n-best of ctc_prefix_beam_search")
        scored = self.score(enc_rows, row_start, row_len, [r.nbest for r in results], use_right(c, rw))
        return combine(c, scored, results, cw, rw, return_nbest)
