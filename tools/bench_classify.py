#!/usr/bin/env python3
"""Time the classification tail (cfm_cls_classify: masked mean pool + heads) on the benchmark's
shape: the configs[1] masked batch (240 min of audio, 70 utterances, 2,845 chunks of 64 ->
182,080 packed encoder rows x 512 f32), against the reference's own expression run with torch on
the same device data: (enc * mask).sum(1) / (count + 1e-10) on the padded equivalent, then the
Linear heads, argmax and softmax (modules/classification_model.py:188-198, 266-279).

    python tools/bench_classify.py [--iters 200] [--warmup 20]

One process, device events around `iters` back-to-back calls after a warm-up, the two versions
alternated over `--rounds` rounds; prints one JSON line.  The pool must read every valid row once:
bytes_valid = sum(out_len) * d * 4; GB/s = bytes_valid / pool time.  Needs a GPU (no fallback).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import C, workload_lengths  # noqa: E402
from chunkformer_amd import _lib  # noqa: E402
from chunkformer_amd.classifier import ClassifierConfig, ClassifierHeads, masked_mean_pool  # noqa: E402
from chunkformer_amd.distributed import chunks_of, out_len  # noqa: E402

TASKS = {"gender": 2, "emotion": 7, "region": 5}


def timed(fn, iters: int) -> float:
    """milliseconds per call over `iters` back-to-back calls (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=10, help="iterations of the torch expression (GB-sized temporaries)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--minutes", type=float, default=240.0)
    ap.add_argument("--d", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classify needs a GPU")
    dev = torch.device("cuda", 0)
    d = args.d
    lens = workload_lengths(int(args.minutes * 60 * 100), seed=0)
    n_chunks = [chunks_of(t, C) for t in lens]
    row_len = [out_len(t) for t in lens]
    row_start = (np.cumsum([0] + n_chunks[:-1]) * C).tolist()
    rows, B = sum(n_chunks) * C, len(lens)
    g = torch.Generator(device=dev).manual_seed(0)
    enc = torch.randn(rows, d, generator=g, device=dev) + 0.8
    cfg = ClassifierConfig(tasks=dict(TASKS), enc_dim=d)
    gw = torch.Generator().manual_seed(1)
    sd = {}
    for name, n in TASKS.items():
        sd[f"classification_heads.{name}.linear.weight"] = (torch.rand(n, d, generator=gw) * 2 - 1) / d ** 0.5
        sd[f"classification_heads.{name}.linear.bias"] = (torch.rand(n, generator=gw) * 2 - 1) / d ** 0.5
    heads = ClassifierHeads(cfg, sd, dev)

    # the padded equivalent the reference's expression works on: [B, T'max, d] + mask [B, T'max, 1]
    Tmax = max(row_len)
    padded = torch.zeros(B, Tmax, d, device=dev)
    for b, (s, n) in enumerate(zip(row_start, row_len)):
        padded[b, :n] = enc[s: s + n]
    mask = (torch.arange(Tmax, device=dev)[None, :] < torch.tensor(row_len, device=dev)[:, None]).unsqueeze(-1).float()
    W = {n: sd[f"classification_heads.{n}.linear.weight"].to(dev) for n in TASKS}
    bias = {n: sd[f"classification_heads.{n}.linear.bias"].to(dev) for n in TASKS}

    def torch_pool():
        return (padded * mask).sum(dim=1) / (mask.sum(dim=1) + 1e-10)

    def torch_classify():
        pooled = torch_pool()
        out = {}
        for n in TASKS:
            logits = torch.nn.functional.linear(pooled, W[n], bias[n])
            pred = torch.argmax(logits, dim=-1)
            out[n] = (pred, torch.softmax(logits, dim=-1).gather(1, pred.unsqueeze(1)).squeeze(1))
        return pooled, out

    def hip_pool():
        return masked_mean_pool(enc, row_start, row_len)

    def hip_classify():
        return heads.classify(enc, row_start, row_len)

    # the C-ABI calls alone: row arrays, outputs and workspace prepared once (as a graph-captured caller holds them)
    rs = torch.tensor(row_start, dtype=torch.int32, device=dev)
    rl = torch.tensor(row_len, dtype=torch.int32, device=dev)
    S, T = cfg.sum_classes, len(TASKS)
    o_pooled = torch.empty(B, d, device=dev)
    o_logits = torch.empty(B, S, device=dev)
    o_pred = torch.empty(B, T, dtype=torch.int32, device=dev)
    o_prob = torch.empty(B, T, device=dev)
    nbytes = int(_lib.cfm_cls_workspace_bytes(heads._h, rows, B))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def raw_classify():
        _lib.check(_lib.cfm_cls_classify(heads._h, enc.data_ptr(), rows, rs.data_ptr(), rl.data_ptr(), B,
                                         o_pooled.data_ptr(), o_logits.data_ptr(), o_pred.data_ptr(),
                                         o_prob.data_ptr(), ws.data_ptr(), nbytes, stream))

    def raw_pool():
        _lib.check(_lib.cfm_cls_pool(enc.data_ptr(), rows, d, rs.data_ptr(), rl.data_ptr(), B, o_pooled.data_ptr(),
                                     ws.data_ptr(), nbytes, stream))

    # same results first
    pooled, logits, pred, prob = hip_classify()
    t_pooled, t_out = torch_classify()
    pool_diff = float((pooled - t_pooled).abs().max())
    same_ids = all(torch.equal(pred[:, t].long(), t_out[n][0]) for t, n in enumerate(TASKS))
    prob_diff = max(float((prob[:, t] - t_out[n][1]).abs().max()) for t, n in enumerate(TASKS))

    raw_classify()
    raw_same = torch.equal(o_pooled, pooled) and torch.equal(o_pred, pred) and torch.equal(o_prob, prob)
    fns = {"cfm_cls_classify": raw_classify, "cfm_cls_pool": raw_pool, "wrapper_classify": hip_classify,
           "wrapper_pool": hip_pool, "torch_classify": torch_classify, "torch_pool": torch_pool}
    iters = {k: (args.torch_iters if k.startswith("torch") else args.iters) for k in fns}
    for k, fn in fns.items():
        for _ in range(min(args.warmup, iters[k])):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):   # alternate the versions
        for k, fn in fns.items():
            ms[k].append(timed(fn, iters[k]))
    best = {k: min(v) for k, v in ms.items()}
    bytes_valid = sum(row_len) * d * 4
    res = {"tool": "bench_classify", "rows": rows, "d": d, "B": B, "valid_rows": sum(row_len),
           "padded_shape": [B, Tmax, d], "bytes_valid": bytes_valid, "iters": args.iters, "rounds": args.rounds,
           "us_per_call": {k: round(v * 1e3, 2) for k, v in best.items()},
           "us_per_call_all_rounds": {k: [round(x * 1e3, 2) for x in v] for k, v in ms.items()},
           "cfm_cls_pool_GBps": round(bytes_valid / (best["cfm_cls_pool"] * 1e-3) / 1e9, 1),
           "note": "wrapper_* = the Python methods (row arrays uploaded and outputs allocated per call)",
           "raw_equals_wrapper": raw_same,
           "max_abs_pooled_diff_vs_torch": pool_diff, "ids_equal_torch": same_ids,
           "max_abs_prob_diff_vs_torch": prob_diff}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
