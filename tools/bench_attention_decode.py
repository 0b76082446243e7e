"""Measure the `attention` decoding mode: the device beam search against the reference's formulation in torch.

    python tools/bench_attention_decode.py [--iters 3] [--cases a,b] [--max-len 160] [--out profiles/NAME.json]

Decoder: d = 512, 8 heads (head dim 64), 3 blocks, ff = 2048, V = 5,000, bf16, beam 10, seeded weights with a
sharpened output layer (attention_decode.sharpened_decoder_state_dict, scale 8, eos offset -2) so that searches run
for tens to hundreds of steps; random encoder rows.  `--max-len` bounds the steps of both sides (the reference's
decode_maxlen); the step counts are recorded.
(a) the 240-minute batch: 70 utterances x 2,601 encoder rows;
(b) 256 utterances x 374 rows.

Baseline: the reference's formulation written in torch on the same GPU, in the same process and on the same inputs,
under torch.autocast(bfloat16): the padded batch of B x N rows stepping together until all rows ended or the longest
limit, a per-step decoder with K / V caches (self-attention: [R, i, d] grown by torch.cat; cross-attention: the
memory repeated per beam and projected once), the whole self-attention cache index_select-ed by the parents at every
step, a full [R, V] log-softmax and two topk calls.  Its tokens are compared with ours; 16-bit near-ties may differ,
the count of utterances with equal tokens is reported.

Times are device events around each whole search after a warm-up, the two alternating; every repeat is listed.
Split of our step, from calls of their own on the search's shapes:
  self_attention / cross_attention   cfm_op_decode_attention at the median cached length, times the blocks;
  head_topk_prune                    a decoder handle with 0 blocks stepping the same batch (embedding, after_norm, head
                                     GEMM, top-N, prune);
  gemm_layernorm                     the remainder.
host_bound: the wall time the host needs to enqueue the steps (no synchronisation) over the device time of the same
steps; near or above 1 the step is launch-bound.

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEAM = 10


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ts):
    return {"ms": ts, "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


@torch.no_grad()
def baseline(R, cfg, W, pe, enc, B, T, beam, max_len):
    """the reference's attention_beam_search on the padded batch, with its caches, in torch"""
    dev, d, H, nb, p = enc.device, cfg.d_model, cfg.heads, cfg.num_blocks, R.LEFT
    dk = d // H
    lin = lambda n, x: torch.nn.functional.linear(x, W[n + ".weight"], W[n + ".bias"])   # noqa: E731
    ln = lambda n, x: torch.nn.functional.layer_norm(x, (d,), W[n + ".weight"], W[n + ".bias"], cfg.eps)   # noqa: E731
    Rn = B * beam
    mem = enc.reshape(B, T, d).repeat_interleave(beam, dim=0)          # repeated per beam (search.py via the decoder)
    hyps = torch.full((Rn, 1), cfg.sos, dtype=torch.long, device=dev)
    scores = torch.tensor([0.0] + [-math.inf] * (beam - 1), device=dev).repeat(B).unsqueeze(1)
    end = torch.zeros_like(scores, dtype=torch.bool)
    self_cache = {}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cross = [(lin(f"{p}decoders.{l}.src_attn.linear_k", mem).view(Rn, T, H, dk).transpose(1, 2),
                  lin(f"{p}decoders.{l}.src_attn.linear_v", mem).view(Rn, T, H, dk).transpose(1, 2)) for l in range(nb)]
    steps = 0
    for i in range(1, max_len + 1):
        if bool(end.sum() == Rn):
            break
        steps += 1
        with torch.autocast("cuda", dtype=torch.bfloat16):
            x = (W[p + "embed.0.weight"][hyps[:, -1]] * math.sqrt(d) + pe[i - 1]).unsqueeze(1)
            for l in range(nb):
                q_ = f"{p}decoders.{l}."
                h = ln(q_ + "norm1", x)
                k = lin(q_ + "self_attn.linear_k", h).view(Rn, 1, H, dk).transpose(1, 2)
                v = lin(q_ + "self_attn.linear_v", h).view(Rn, 1, H, dk).transpose(1, 2)
                if l in self_cache:
                    k, v = torch.cat([self_cache[l][0], k], dim=2), torch.cat([self_cache[l][1], v], dim=2)
                self_cache[l] = (k, v)
                q = lin(q_ + "self_attn.linear_q", h).view(Rn, 1, H, dk).transpose(1, 2)
                a = torch.softmax(torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(dk), dim=-1)
                x = x + lin(q_ + "self_attn.linear_out", torch.matmul(a, v).transpose(1, 2).reshape(Rn, 1, d))
                h = ln(q_ + "norm2", x)
                q = lin(q_ + "src_attn.linear_q", h).view(Rn, 1, H, dk).transpose(1, 2)
                a = torch.softmax(torch.matmul(q, cross[l][0].transpose(-2, -1)) / math.sqrt(dk), dim=-1)
                x = x + lin(q_ + "src_attn.linear_out", torch.matmul(a, cross[l][1]).transpose(1, 2).reshape(Rn, 1, d))
                h = ln(q_ + "norm3", x)
                x = x + lin(q_ + "feed_forward.w_2", torch.relu(lin(q_ + "feed_forward.w_1", h)))
            logp = torch.log_softmax(lin(p + "output_layer", ln(p + "after_norm", x[:, 0])), dim=-1)
        top_v, top_i = logp.float().topk(beam)
        top_v = torch.where(end, torch.tensor([0.0] + [-math.inf] * (beam - 1), device=dev).expand(Rn, beam), top_v)
        top_i = torch.where(end, torch.full_like(top_i, cfg.eos), top_i)
        cand = (scores + top_v).view(B, beam * beam)
        scores, off = cand.topk(beam)
        parent = (off // beam + torch.arange(B, device=dev).unsqueeze(1) * beam).view(-1)
        self_cache = {l: (torch.index_select(kv[0], 0, parent), torch.index_select(kv[1], 0, parent))
                      for l, kv in self_cache.items()}
        best = (off + torch.arange(B, device=dev).unsqueeze(1) * beam * beam).view(-1)
        hyps = torch.cat([torch.index_select(hyps, 0, parent), torch.index_select(top_i.reshape(-1), 0, best).view(-1, 1)], 1)
        scores = scores.view(-1, 1)
        end = (hyps[:, -1] == cfg.eos).view(-1, 1)
    best = scores.view(B, beam).argmax(dim=-1) + torch.arange(B, device=dev) * beam      # length_penalty 0
    rows = hyps[best, 1:].cpu().tolist()
    return [[t for t in r if t != cfg.eos] for r in rows], steps


def op_time(_lib, kernel, B, H, dk, n_keys, T, ns, iters, stream):
    dev, d, Rn = "cuda", H * dk, B * BEAM
    g = torch.Generator().manual_seed(5)
    q = torch.randn(Rn, d, generator=g).to(dev, torch.bfloat16)
    out = torch.empty_like(q)
    if kernel == _lib.DEC_ATTN_SELF_GATHER:
        kv = torch.randn(n_keys, Rn, 2 * d, generator=g).to(dev, torch.bfloat16)
        anc = (torch.arange(Rn).unsqueeze(1) // BEAM * BEAM + torch.randint(0, BEAM, (Rn, n_keys), generator=g)).to(dev, torch.int32)
        args = (kv.data_ptr(), n_keys, anc.data_ptr(), n_keys, n_keys, 0, 0, 1, 0)
        keep = (kv, anc)
    else:
        kv = torch.randn(B * T, 2 * d, generator=g).to(dev, torch.bfloat16)
        us = (torch.arange(B, dtype=torch.int32) * T).to(dev)
        ul = torch.full((B,), T, dtype=torch.int32, device=dev)
        scratch = torch.empty(ns * Rn * (d + 2 * H) + 8, device=dev)
        args = (kv.data_ptr(), B * T, 0, 0, 0, us.data_ptr(), ul.data_ptr(), ns, scratch.data_ptr())
        keep = (kv, us, ul, scratch)

    def run():
        _lib.check(_lib.cfm_op_decode_attention(_lib.DTYPE_BF16, kernel, q.data_ptr(), out.data_ptr(), B, BEAM, H, dk,
                                                *args, stream))
    run()
    torch.cuda.synchronize()
    ts = [timed(run) for _ in range(max(iters, 5))]
    del keep
    return statistics.median(ts)


def run_case(A, R, _lib, dec, head_only, cfg, W, pe, B, T, seed, iters, max_len):
    dev = dec.device
    rng = np.random.default_rng(seed)
    rows, starts = [T] * B, [b * T for b in range(B)]
    enc = torch.from_numpy(rng.standard_normal((B * T, cfg.d_model)).astype(np.float32)).to(dev)
    ours = dec.search(enc, starts, rows, BEAM, 0.0, max_len)          # warm-up
    base_tok, base_steps = baseline(R, cfg, W, pe, enc, B, T, BEAM, max_len)
    torch.cuda.synchronize()
    t_ours, t_base, t_head = [], [], []
    for _ in range(iters):
        t_ours.append(timed(lambda: dec.search(enc, starts, rows, BEAM, 0.0, max_len)))
        steps_enq = dec.last_steps_enqueued
        t_head.append(timed(lambda: head_only.search(enc, starts, rows, BEAM, 0.0, steps_enq)))
        head_steps = head_only.last_steps_enqueued
        t_base.append(timed(lambda: baseline(R, cfg, W, pe, enc, B, T, BEAM, max_len)))
    steps = [r.steps for r in ours]
    n_steps = max(1, steps_enq)
    total = statistics.median(t_ours)
    H, dk, nb = cfg.heads, cfg.d_model // cfg.heads, cfg.num_blocks
    stream = torch.cuda.current_stream(dev).cuda_stream
    ns = 1 if B * H >= 2048 else max(1, min(16, (2048 + B * H - 1) // (B * H), T // 64))   # attdec.hip ad_key_splits, 256 CUs
    mid = max(1, n_steps // 2)
    t_self = op_time(_lib, _lib.DEC_ATTN_SELF_GATHER, B, H, dk, mid, T, 1, iters, stream) * nb * n_steps
    t_cross = op_time(_lib, _lib.DEC_ATTN_CROSS_MFMA, B, H, dk, 0, T, ns, iters, stream) * nb * n_steps
    t_cross_gen = op_time(_lib, _lib.DEC_ATTN_CROSS_GENERIC, B, H, dk, 0, T, ns, iters, stream) * nb * n_steps
    t_h = statistics.median(t_head) / max(1, head_steps) * n_steps
    # host-bound fraction: enqueue POLL-free steps on a fresh state, wall time without a synchronisation
    S = max_len
    nbytes = int(_lib.cfm_attdec_workspace_bytes(dec.rescorer._h, B, BEAM, B * T, S))
    state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)   # noqa: E731
    rs, rl, lim = i32(starts), i32(rows), i32([S] * B)
    _lib.check(_lib.cfm_attdec_begin(dec.rescorer._h, enc.data_ptr(), B * T, rs.data_ptr(), rl.data_ptr(), lim.data_ptr(), B,
                                     BEAM, S, state.data_ptr(), nbytes, stream))
    torch.cuda.synchronize()
    k = min(32, S)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    _lib.check(_lib.cfm_attdec_steps(dec.rescorer._h, state.data_ptr(), B, BEAM, B * T, S, 1, k, stream))
    host_ms = (time.perf_counter() - t0) * 1e3
    b.record()
    b.synchronize()
    dev_ms = a.elapsed_time(b)
    launches = 1 + nb * (12 + (1 if ns > 1 else 0)) + 1 + (2 if cfg.vocab % 256 else 1) + 1 + 1
    same = sum(1 for r, t in zip(ours, base_tok) if r.tokens == t)
    return {"utterances": B, "rows_per_utterance": T, "beam": BEAM, "max_len": max_len,
            "steps_per_utterance": {"min": min(steps), "median": statistics.median(steps), "max": max(steps)},
            "steps_enqueued": steps_enq, "polls": dec.last_polls, "baseline_steps": base_steps,
            "ours": spread(t_ours), "torch_reference_formulation": spread(t_base),
            "speedup": statistics.median(t_base) / total, "ms_per_step": total / n_steps,
            "baseline_ms_per_step": statistics.median(t_base) / max(1, base_steps),
            "utterances_with_equal_tokens": same,
            "split_ms": {"self_attention": t_self, "cross_attention": t_cross, "head_topk_prune": t_h,
                         "gemm_layernorm": total - t_self - t_cross - t_h},
            "cross_attention_generic_ms": t_cross_gen, "key_splits": ns, "launches_per_step": launches,
            "host_enqueue_ms_per_step": host_ms / k, "device_ms_per_step_first_steps": dev_ms / k,
            "host_bound": host_ms / dev_ms, "state_bytes": dec.last_workspace_bytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--max-len", type=int, default=160)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_decode.py measures on the GPU")
    from chunkformer_amd import _lib
    from chunkformer_amd import attention_decode as A
    from chunkformer_amd import rescore as R
    cfg = R.AEDConfig(vocab=5000, d_model=512, heads=8, ff=2048, num_blocks=3, r_num_blocks=0)
    sd = A.sharpened_decoder_state_dict(cfg, 0, 8.0, -2.0)
    dec = A.AttentionDecoder(R.AttentionRescorer(cfg, sd, "cuda", "bf16"))
    head_only = A.AttentionDecoder(R.AttentionRescorer(dataclasses.replace(cfg, num_blocks=0), sd, "cuda", "bf16"))
    dev = dec.device
    W = {k: v.to(dev) for k, v in R.native_names(cfg, sd).items()}
    pe = R.positional_table(cfg.d_model).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "iters": a.iters, "poll_steps": A.POLL_STEPS,
           "decoder": {k: getattr(cfg, k) for k in ("d_model", "heads", "ff", "num_blocks", "vocab")}}
    shapes = {"a": ("batch_240min", 70, 2601), "b": ("batch_256_short", 256, 374)}
    for key in a.cases.split(","):
        name, B, T = shapes[key]
        res[name] = run_case(A, R, _lib, dec, head_only, cfg, W, pe, B, T, 1 + ord(key), a.iters, a.max_len)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
