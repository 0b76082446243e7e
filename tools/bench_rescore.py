"""Measure attention rescoring: one cfm_aed_score call per batch against the reference's formulation in torch.

    python tools/bench_rescore.py [--iters 5] [--cases a,b] [--out profiles/NAME.json]

Decoder: d = 512, 8 heads (head dim 64), 3 + 3 blocks, ff = 2048, V = 5,000, bf16, seeded weights; random encoder
rows and random hypotheses (rescoring does not depend on where they come from).
(a) the 240-minute batch: 70 utterances x 2,601 encoder rows, 10 hypotheses of about 650 tokens each;
(b) 256 utterances x 374 rows, 10 hypotheses of about 90 tokens each.

Baseline: the reference's formulation written in torch on the same GPU, in the same process and on the same inputs
(rescore.decoder_logp_padded under torch.autocast(bfloat16), as the reference decodes): one utterance at a time,
hypotheses padded to a common length, the memory repeated per hypothesis, [n_hyps, H, L, T'] scores, a full
[n_hyps, L, V] log-softmax, then gathers.  Its chosen indices (ctc_weight 0.3, reverse_weight 0.3) must equal ours.

Times are device events around each call after a warm-up, the two alternating; every repeat is listed, with median,
min and max.  The split of our call is measured with calls of its own, same buffers and shapes:
  attention_self / attention_cross   cfm_op_seg_attention (the MFMA kernel, and the generic one beside it) on the
                                     call's own descriptors, times the 6 blocks;
  head                               a decoder handle with 0 + 0 blocks: embedding, after_norm, the output GEMM in
                                     row slabs and the target log-prob kernel, both directions;
  gemm_layernorm                     the remainder of the call (projections, feed-forward, LayerNorms).
The attention FLOP count is 4 d per visible (query, key) pair; its rate is given as a fraction of the 2.5 PFLOP/s
bf16 peak.

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 2.5e15


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ts):
    return {"ms": ts, "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


class ScoreCall:
    """cfm_aed_score with every buffer allocated once: run() is the launches only."""

    def __init__(self, resc, enc, starts, rows, nbest):
        from chunkformer_amd import _lib
        self._lib, self.h = _lib, resc._h
        c, dev = resc.cfg, resc.device
        toks, hs, hl, hu = [], [], [], []
        for b, hyps in enumerate(nbest):
            for h in hyps:
                hs.append(len(toks)); hl.append(len(h) + 1); hu.append(b)
                toks.append(c.sos); toks.extend(h)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)   # noqa: E731
        self.enc = enc
        self.rows, self.B, self.n_tok, self.n_hyp = enc.shape[0], len(nbest), len(toks), len(hs)
        self.hs, self.hl, self.hu = hs, hl, hu
        self.d = [i32(starts), i32(rows), i32(toks), i32(hs), i32(hl), i32(hu)]
        self.l2r = torch.zeros(self.n_tok, device=dev)
        self.r2l = torch.zeros(self.n_tok, device=dev)
        self.nbytes = int(_lib.cfm_aed_workspace_bytes(self.h, self.n_tok, self.rows))
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def run(self):
        d = self.d
        self._lib.check(self._lib.cfm_aed_score(self.h, self.enc.data_ptr(), self.rows, d[0].data_ptr(), d[1].data_ptr(),
                                                self.B, d[2].data_ptr(), self.n_tok, d[3].data_ptr(), d[4].data_ptr(),
                                                d[5].data_ptr(), self.n_hyp, 3, self.l2r.data_ptr(), self.r2l.data_ptr(),
                                                self.ws.data_ptr(), self.nbytes, self.stream))

    def scores(self):
        assert int(self.ws[:4].view(torch.int32).item()) == 0
        l, r = self.l2r.cpu(), self.r2l.cpu()
        out, k = [], 0
        for b in range(self.B):
            res = []
            while k < self.n_hyp and self.hu[k] == b:
                s, n = self.hs[k], self.hl[k]
                res.append((l[s: s + n], r[s: s + n]))
                k += 1
            out.append(res)
        return out


def attention_split(_lib, call, starts, rows, d, H, iters):
    """the two attention uses alone, on the call's descriptors and random bf16 rows"""
    dev = call.enc.device
    self_d = [[s, n, s, n, 1, 0, 0, 0] for s, n in zip(call.hs, call.hl)]
    cross_d = [[s, n, starts[u], rows[u], 0, 0, 0, 0] for s, n, u in zip(call.hs, call.hl, call.hu)]
    g = torch.Generator().manual_seed(3)
    q = torch.randn(call.n_tok, d, generator=g).to(dev, torch.bfloat16)
    kv_s = torch.randn(call.n_tok, 2 * d, generator=g).to(dev, torch.bfloat16)
    kv_c = torch.randn(call.rows, 2 * d, generator=g).to(dev, torch.bfloat16)
    out = torch.empty_like(q)
    scratch = torch.zeros(call.n_hyp + 2, dtype=torch.int32, device=dev)
    res = {}
    for name, desc, kv, kr in (("self", self_d, kv_s, call.n_tok), ("cross", cross_d, kv_c, call.rows)):
        dd = torch.tensor(desc, dtype=torch.int32).to(dev)
        for kname, kid in (("mfma", _lib.SEG_ATTN_MFMA), ("generic", _lib.SEG_ATTN_GENERIC)):
            def run():
                _lib.check(_lib.cfm_op_seg_attention(_lib.DTYPE_BF16, kid, q.data_ptr(), call.n_tok, kv.data_ptr(), kr,
                                                     dd.data_ptr(), call.n_hyp, H, d // H, out.data_ptr(),
                                                     scratch.data_ptr(), call.stream))
            run()
            torch.cuda.synchronize()
            res[f"{name}_{kname}"] = spread([timed(run) for _ in range(iters)])
    pairs_self = sum(n * (n + 1) // 2 for n in call.hl)
    pairs_cross = sum(n * rows[u] for n, u in zip(call.hl, call.hu))
    res["flop_self_per_layer"] = 4 * d * pairs_self
    res["flop_cross_per_layer"] = 4 * d * pairs_cross
    return res


def baseline(R, cfg, W, pe, enc, starts, rows, nbest):
    """the reference's formulation: per utterance, padded, memory repeated, full log-softmax, gathers"""
    dev = enc.device
    out = []
    for b, hyps in enumerate(nbest):
        mem = enc[starts[b]: starts[b] + rows[b]]
        L = max(len(h) for h in hyps) + 1
        per = []
        for p, nb, rev in ((R.LEFT, cfg.num_blocks, False), (R.RIGHT, cfg.r_num_blocks, True)):
            seqs = [h[::-1] if rev else h for h in hyps]
            ys = torch.tensor([[cfg.sos] + s + [cfg.eos] * (L - 1 - len(s)) for s in seqs], dtype=torch.long, device=dev)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                lp = R.decoder_logp_padded(W, p, cfg, nb, ys, [len(s) + 1 for s in seqs], mem, pe)
            tgt = torch.tensor([s + [cfg.eos] * (L - len(s)) for s in seqs], dtype=torch.long, device=dev)
            per.append(lp.float().gather(2, tgt.unsqueeze(-1)).squeeze(-1))
        out.append(per)
    return out


def baseline_scores(out, nbest):
    res = []
    for per, hyps in zip(out, nbest):
        l, r = per[0].cpu(), per[1].cpu()
        res.append([(l[i, : len(h) + 1], r[i, : len(h) + 1]) for i, h in enumerate(hyps)])
    return res


def run_case(R, _lib, resc, head_only, cfg, W, pe, B, T, n_hyps, n_tok, seed, iters):
    dev = resc.device
    rng = np.random.default_rng(seed)
    rows = [T] * B
    starts = [b * T for b in range(B)]
    enc = torch.from_numpy(rng.standard_normal((B * T, cfg.d_model)).astype(np.float32)).to(dev)
    lo = max(1, int(n_tok * 0.97))
    nbest = [[[int(t) for t in rng.integers(1, cfg.vocab - 1, int(rng.integers(lo, n_tok + 1)))] for _ in range(n_hyps)]
             for _ in range(B)]
    ctc = [sorted((-float(x) for x in rng.uniform(0.0, 20.0, n_hyps)), reverse=True) for _ in range(B)]
    call = ScoreCall(resc, enc, starts, rows, nbest)
    head = ScoreCall(head_only, enc, starts, rows, nbest)
    call.run(); head.run()
    baseline(R, cfg, W, pe, enc, starts[:1], rows[:1], nbest[:1])   # warm-up
    torch.cuda.synchronize()
    t_ours, t_base, t_head = [], [], []
    base_out = None
    for _ in range(iters):
        t_ours.append(timed(call.run))
        t_head.append(timed(head.run))
        hold = []
        t_base.append(timed(lambda: hold.append(baseline(R, cfg, W, pe, enc, starts, rows, nbest))))
        base_out = hold[0]
    from chunkformer_amd.search import DecodeResult
    results = [DecodeResult(h[0], nbest=h, nbest_scores=c, nbest_times=None) for h, c in zip(nbest, ctc)]
    ours = R.combine(cfg, call.scores(), results, 0.3, 0.3)
    theirs = R.combine(cfg, baseline_scores(base_out, nbest), results, 0.3, 0.3)
    same = [a.best_index for a in ours] == [b.best_index for b in theirs]
    att = attention_split(_lib, call, starts, rows, cfg.d_model, cfg.heads, iters)
    nl = cfg.num_blocks + cfg.r_num_blocks
    total = statistics.median(t_ours)
    a_self, a_cross = nl * att["self_mfma"]["median_ms"], nl * att["cross_mfma"]["median_ms"]
    h_ms = statistics.median(t_head)
    flop = nl * (att["flop_self_per_layer"] + att["flop_cross_per_layer"])
    return {"utterances": B, "rows_per_utterance": T, "hypotheses": n_hyps, "token_rows": call.n_tok,
            "ours": spread(t_ours), "torch_reference_formulation": spread(t_base),
            "speedup": statistics.median(t_base) / total, "chosen_indices_equal": same,
            "split_ms": {"attention_self": a_self, "attention_cross": a_cross, "head": h_ms,
                         "gemm_layernorm": total - a_self - a_cross - h_ms},
            "attention_kernels_per_layer": {k: v for k, v in att.items() if not k.startswith("flop")},
            "attention_flop": flop, "attention_fraction_of_bf16_peak": flop / ((a_self + a_cross) * 1e-3) / PEAK_BF16,
            "workspace_bytes": call.nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rescore.py measures on the GPU")
    from chunkformer_amd import _lib
    from chunkformer_amd import rescore as R
    cfg = R.AEDConfig(vocab=5000, d_model=512, heads=8, ff=2048, num_blocks=3, r_num_blocks=3)
    sd = R.synthetic_decoder_state_dict(cfg, 0)
    resc = R.AttentionRescorer(cfg, sd, "cuda", "bf16")
    head_only = R.AttentionRescorer(dataclasses.replace(cfg, num_blocks=0, r_num_blocks=0), sd, "cuda", "bf16")
    dev = resc.device
    W = {k: v.to(dev) for k, v in R.native_names(cfg, sd).items()}
    pe = R.positional_table(cfg.d_model).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "iters": a.iters,
           "decoder": {k: getattr(cfg, k) for k in ("d_model", "heads", "ff", "num_blocks", "r_num_blocks", "vocab")}}
    shapes = {"a": ("batch_240min", 70, 2601, 10, 650), "b": ("batch_256_short", 256, 374, 10, 90)}
    for key in a.cases.split(","):
        name, B, T, nh, nt = shapes[key]
        res[name] = run_case(R, _lib, resc, head_only, cfg, W, pe, B, T, nh, nt, 1 + ord(key), a.iters)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    bad = [k for k, v in res.items() if isinstance(v, dict) and v.get("chosen_indices_equal") is False]
    if bad:
        raise SystemExit(f"the baseline's chosen indices differ from ours in {bad}")


if __name__ == "__main__":
    main()
