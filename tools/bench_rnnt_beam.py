"""Measure the transducer prefix beam search (decoding_method "rnnt_beam_search"): the device search against the
reference's formulation in torch.

    python tools/bench_rnnt_beam.py [--iters 3] [--cases a,b,c] [--beams 5,10] [--baseline-frames 200]
                                    [--predictor rnn|embedding|conv] [--out profiles/NAME.json]

Model: the vie recipe's predictor and joint (embed 256, LSTM 2 x 512, join_dim 512) at enc_dim 512, V = 1,024, seeded
weights with blank_bias 7 (transducer.synthetic_transducer_state_dict); random encoder rows, CTC log-probs from seeded
logits, weights (0.3, 0.7).
(a) the 240-minute batch: 70 utterances x 2,601 encoder rows;
(b) 256 utterances x 374 rows;
(c) one utterance of 45,000 rows (endless_decode's B = 1).

Baseline: the reference's formulation written in torch on the same GPU, in the same process and on the same inputs:
one utterance at a time, per frame one batched predictor + joint step, log_softmax, fusion, topk, then the Python
candidate loop with an .item() per candidate, list copies, the pairwise prefix fusion and a sort.  It is run for
`--baseline-frames` frames of the first utterance and scaled to the case's utterances x rows (it is linear in both):
the full shapes would take minutes to hours.  Its tokens over those frames are compared with ours.

Times are device events around each whole search after a warm-up; every repeat is listed.
Split of our frame, from calls of their own on the search's shapes (include/cfm_ops.h):
  predictor        cfm_op_rnnt_lstm_step for B x beam rows (embedding, LSTM GEMMs + cells, projection GEMM, and the
                   operator's ten small state copies in and out, which the search does not have: an upper bound,
                   loose at a handful of rows);
  fused_topk       cfm_op_rnnt_fused_topk for [B x beam, V];
  prune            cfm_op_rnnt_beam_prune, one utterance (the search runs one workgroup per utterance in one launch);
  joint_head_gather   the remainder: tanh(enc + pred), the ffn_out GEMM to [B x beam, V], the state gathers.
host_bound: the wall time the host needs to enqueue the whole search (no synchronisation) over the device time of the
same search.  Near 1 either the host is the bound or the enqueueing call ran into the queue's depth and waited for
the device (searches of thousands of frames); the short case (b) shows the enqueue cost alone.

`--predictor embedding|conv` measures a stateless handle of equal widths (embed = output = 512, history 2, 4 heads)
instead, beside the LSTM handle in the same process on the same inputs (boxes differ by 1-3%): per case and beam the
whole search and the predictor pass alone (cfm_op_rnnt_predictor_step / cfm_op_rnnt_lstm_step for B x beam rows) of
both handles, and the greedy search at B = 1 (2,000 rows, n_steps 4, blank_bias 3.72: most frames emit) in ms per
emission -- the stateless one-workgroup kernel beside the LSTM's one-workgroup and multi-CU kernels.  The torch
baseline is not run in this form.

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ts):
    return {"ms": ts, "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def log_add(a, b):
    import math
    if a == -math.inf and b == -math.inf:
        return -math.inf
    m = max(a, b)
    return m + math.log(math.exp(a - m) + math.exp(b - m))


@torch.no_grad()
def baseline(W, rnn, cfg, enc, ctc, K, cw, tw, frames):
    """prefix_beam_search's formulation for the first `frames` frames of one utterance, in torch on the device"""
    dev = enc.device
    lin = lambda n, x: torch.nn.functional.linear(x, W[n + ".weight"], W[n + ".bias"])   # noqa: E731
    zero = torch.zeros(cfg.num_layers, 1, cfg.hidden, device=dev)
    beam = [([cfg.blank], 0.0, (zero, zero))]
    for i in range(frames):
        inp = torch.tensor([s[0][-1] for s in beam], dtype=torch.int, device=dev).unsqueeze(-1)
        hb = torch.cat([s[2][0] for s in beam], dim=1)
        cb = torch.cat([s[2][1] for s in beam], dim=1)
        scores = torch.tensor([s[1] for s in beam]).to(dev)
        out, (m, c) = rnn(W["predictor.embed.weight"][inp], (hb, cb))
        pre = lin("predictor.projection", out)
        x = lin("joint.enc_ffn", enc[i].view(1, 1, -1)).unsqueeze(2) + lin("joint.pred_ffn", pre).unsqueeze(1)
        logp = lin("joint.ffn_out", torch.tanh(x)).log_softmax(dim=-1).squeeze(1).squeeze(1)
        new_cache = list(zip(torch.split(m, 1, dim=1), torch.split(c, 1, dim=1)))
        logp = torch.log(torch.add(tw * torch.exp(logp), cw * torch.exp(ctc[i].unsqueeze(0))))
        top_v, top_i = logp.topk(K)
        sc = torch.add(scores.unsqueeze(1), top_v)
        cand = []
        for j, base in enumerate(beam):
            for t in range(K):
                if top_i[j, t] == cfg.blank:
                    cand.append([base[0].copy(), sc[j, t].item(), base[2]])
                else:
                    hyp = base[0].copy()
                    hyp.append(top_i[j, t].item())
                    cand.append([hyp, sc[j, t].item(), new_cache[j]])
        fused = [cand[0]]
        for s1 in cand[1:]:
            for s0 in fused:
                if s1[0] == s0[0]:
                    s0[1] = log_add(s0[1], s1[1])
                    break
            else:
                fused.append(s1)
        fused.sort(key=lambda s: s[1], reverse=True)
        beam = [tuple(s) for s in fused[:K]]
    return beam[0][0][1:]


def run_case(TB, _lib, search, W, rnn, cfg, B, T, K, seed, iters, base_frames):
    dev = search.device
    rng = np.random.default_rng(seed)
    rows, starts = [T] * B, [b * T for b in range(B)]
    enc = torch.from_numpy(rng.standard_normal((B * T, cfg.enc_dim)).astype(np.float32)).to(dev)
    g = torch.Generator().manual_seed(seed)
    ctc = (torch.randn(B * T, cfg.vocab, generator=g) * 2.0).to(dev).log_softmax(-1)
    cw, tw = 0.3, 0.7
    ours = search.search_packed(enc, ctc, starts, rows, K, cw, tw)          # warm-up
    nf = min(base_frames, T)
    base_tok = baseline(W, rnn, cfg, enc[:T], ctc[:T], K, cw, tw, min(nf, 8))   # warm-up
    torch.cuda.synchronize()
    t_ours = [timed(lambda: search.search_packed(enc, ctc, starts, rows, K, cw, tw)) for _ in range(iters)]
    t_base = []
    for _ in range(max(1, min(iters, 2))):
        t0 = time.perf_counter()
        base_tok = baseline(W, rnn, cfg, enc[:T], ctc[:T], K, cw, tw, nf)
        torch.cuda.synchronize()
        t_base.append((time.perf_counter() - t0) * 1e3)
    ours_nf = search.search_packed(enc[:nf], ctc[:nf], [0], [nf], K, cw, tw)[0].tokens
    total = statistics.median(t_ours)
    base_full = statistics.median(t_base) / nf * T * B
    # split: the single kernels on the search's shapes
    R = B * K
    stream = torch.cuda.current_stream(dev).cuda_stream
    def repeat(call, n=20):   # n calls back to back between two events: no allocation, no synchronisation inside
        call()
        torch.cuda.synchronize()
        return timed(lambda: [call() for _ in range(n)]) / n
    tok = torch.randint(0, cfg.vocab, (R,), generator=g).to(dev, torch.int32)
    h = torch.rand(cfg.num_layers, R, cfg.hidden, generator=g).to(dev)
    ho, co, pj = torch.empty_like(h), torch.empty_like(h), torch.empty(R, cfg.join_dim, device=dev)
    lb = int(_lib.cfm_op_rnnt_lstm_step_workspace_bytes(search.rnnt._h, R))
    lws = torch.zeros(lb, dtype=torch.uint8, device=dev)
    t_pred = repeat(lambda: _lib.check(_lib.cfm_op_rnnt_lstm_step(
        search.rnnt._h, tok.data_ptr(), h.data_ptr(), h.data_ptr(), R, ho.data_ptr(), co.data_ptr(), pj.data_ptr(),
        lws.data_ptr(), lb, stream)))
    logits = torch.randn(R, cfg.vocab, generator=g).to(dev)
    tv, ti = torch.empty(R, K, device=dev), torch.empty(R, K, dtype=torch.int32, device=dev)
    cr = ctc[:R].contiguous() if R <= B * T else ctc[:1].expand(R, -1).contiguous()
    t_topk = repeat(lambda: _lib.check(_lib.cfm_op_rnnt_fused_topk(logits.data_ptr(), cr.data_ptr(), R, cfg.vocab, K, cw, tw,
                                                                  tv.data_ptr(), ti.data_ptr(), stream)))
    Tp = 64
    pv = -torch.sort(torch.rand(Tp, K, K, generator=g) * 8, dim=-1).values
    pi = torch.stack([torch.stack([torch.randperm(cfg.vocab, generator=g)[:K] for _ in range(K)]) for _ in range(Tp)])
    pv, pi = pv.to(dev), pi.to(dev, torch.int32)
    TB.beam_prune_device(pv, pi)
    t_prune = statistics.median([timed(lambda: TB.beam_prune_device(pv, pi)) for _ in range(5)]) / Tp
    # host-bound fraction: the whole search enqueued without a synchronisation
    i32 = dict(dtype=torch.int32, device=dev)
    out_tok, out_time = torch.zeros(K, B * T, **i32), torch.zeros(K, B * T, **i32)
    out_len, n_hyps = torch.zeros(B, K, **i32), torch.zeros(B, **i32)
    out_score = torch.zeros(B, K, dtype=torch.float64, device=dev)
    nbytes = int(_lib.cfm_rnnt_beam_workspace_bytes(search.rnnt._h, B * T, B, K))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rs, rl = torch.tensor(starts, **i32), torch.tensor(rows, **i32)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    _lib.check(_lib.cfm_rnnt_beam_search(search.rnnt._h, enc.data_ptr(), B * T, ctc.data_ptr(), rs.data_ptr(), rl.data_ptr(),
                                         B, T, K, cw, tw, out_tok.data_ptr(), out_time.data_ptr(), out_len.data_ptr(),
                                         out_score.data_ptr(), n_hyps.data_ptr(), 0, 0, 0, 0, 0, ws.data_ptr(), nbytes,
                                         stream))
    host_ms = (time.perf_counter() - t0) * 1e3
    b.record()
    b.synchronize()
    dev_ms = a.elapsed_time(b)
    lens = [len(r.tokens) for r in ours]
    return {"utterances": B, "rows_per_utterance": T, "beam": K, "ours": spread(t_ours), "ms_per_frame": total / T,
            "torch_reference_formulation": {"frames_run": nf, "ms": t_base, "ms_per_frame_one_utterance":
                                            statistics.median(t_base) / nf, "scaled_to_case_ms": base_full},
            "speedup_vs_scaled_baseline": base_full / total, "baseline_tokens_equal_over_its_frames": base_tok == ours_nf,
            "tokens_per_utterance": {"min": min(lens), "median": statistics.median(lens), "max": max(lens)},
            "split_ms_per_frame": {"predictor": t_pred, "fused_topk": t_topk, "prune": t_prune,
                                   "joint_head_gather": total / T - t_pred - t_topk - t_prune},
            "launches_per_frame": 1 + 2 * cfg.num_layers + 1 + 1 + 1 + 1 + 1 + cfg.num_layers,
            "host_enqueue_ms_per_frame": host_ms / T, "device_ms_per_frame": dev_ms / T, "host_bound": host_ms / dev_ms,
            "workspace_bytes": nbytes}


def stateless_compare(TB, _lib, kind, cases, beams, iters):
    from chunkformer_amd.transducer import RNNTConfig, RNNTGreedy, synthetic_transducer_state_dict
    scfg = RNNTConfig(vocab=1024, embed_size=512, hidden=0, num_layers=0, pred_out=512, join_dim=512, predictor=kind,
                      history_size=2, n_head=4)
    lcfg = RNNTConfig(vocab=1024)
    res = {"predictor": kind, "stateless_model": {k: getattr(scfg, k) for k in ("embed_size", "join_dim", "history_size", "n_head")}}
    handles = {}
    for key, cfg in (("stateless", scfg), ("lstm", lcfg)):
        handles[key] = {bb: TB.RNNTBeamSearch(RNNTGreedy(cfg, synthetic_transducer_state_dict(cfg, 0, blank_bias=bb), "cuda"))
                        for bb in (7.0, 3.72)}
    dev = handles["lstm"][7.0].device
    for name, B, T, seed in cases:
        rng = np.random.default_rng(seed)
        rows, starts = [T] * B, [b * T for b in range(B)]
        enc = torch.from_numpy(rng.standard_normal((B * T, lcfg.enc_dim)).astype(np.float32)).to(dev)
        g = torch.Generator().manual_seed(seed)
        ctc = (torch.randn(B * T, lcfg.vocab, generator=g) * 2.0).to(dev).log_softmax(-1)
        for K in beams:
            out = {"utterances": B, "rows_per_utterance": T, "beam": K}
            R = B * K
            for key in ("stateless", "lstm"):
                s = handles[key][7.0]
                s.search_packed(enc, ctc, starts, rows, K, 0.3, 0.7)
                torch.cuda.synchronize()
                ts = [timed(lambda: s.search_packed(enc, ctc, starts, rows, K, 0.3, 0.7)) for _ in range(iters)]
                if key == "stateless":
                    win = torch.randint(0, 1024, (R, scfg.context), generator=g).to(dev, torch.int32)
                    s.predictor_step(win)
                    tp = statistics.median([timed(lambda: s.predictor_step(win)) for _ in range(5)])
                else:
                    tok = torch.zeros(R, dtype=torch.int32, device=dev)
                    h0 = torch.zeros(lcfg.num_layers, R, lcfg.hidden, device=dev)
                    s.lstm_step(tok, h0, h0)
                    tp = statistics.median([timed(lambda: s.lstm_step(tok, h0, h0)) for _ in range(5)])
                out[key] = dict(spread(ts), ms_per_frame=statistics.median(ts) / T, predictor_op_ms=tp,
                                workspace_bytes=int(_lib.cfm_rnnt_beam_workspace_bytes(s.rnnt._h, B * T, B, K)))
            out["stateless_over_lstm"] = out["stateless"]["median_ms"] / out["lstm"]["median_ms"]
            res[f"{name}_beam{K}"] = out
    # greedy at B = 1
    T = 2000
    enc = torch.from_numpy(np.random.default_rng(5).standard_normal((T, lcfg.enc_dim)).astype(np.float32)).to(dev)
    gr = {}
    for key, grid in (("stateless", None), ("lstm_one_workgroup", 0), ("lstm_multi_cu", 32)):
        r = handles["stateless" if key == "stateless" else "lstm"][3.72].rnnt
        if grid is not None:
            r.set_option("grid_blocks", grid)
        dense = r.greedy_packed(enc, [0], [T], 4)
        torch.cuda.synchronize()
        ts = [timed(lambda: r.greedy_packed(enc, [0], [T], 4)) for _ in range(iters)]
        em = int((dense != 0).sum())
        gr[key] = dict(spread(ts), rows=T, emissions=em, ms_per_emission=statistics.median(ts) / max(em, 1),
                       grid_blocks=r.grid_blocks(1))
    res["greedy_b1"] = gr
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--beams", default="5,10")
    ap.add_argument("--baseline-frames", type=int, default=200)
    ap.add_argument("--predictor", default="rnn", choices=("rnn", "embedding", "conv"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnnt_beam.py measures on the GPU")
    from chunkformer_amd import _lib
    from chunkformer_amd import transducer_beam as TB
    from chunkformer_amd.transducer import RNNTConfig, RNNTGreedy, synthetic_transducer_state_dict
    shapes = {"a": ("batch_240min", 70, 2601), "b": ("batch_256_short", 256, 374), "c": ("endless_one_utterance", 1, 45000)}
    if a.predictor != "rnn":
        res = stateless_compare(TB, _lib, a.predictor, [shapes[k] + (1 + ord(k),) for k in a.cases.split(",")],
                                [int(v) for v in a.beams.split(",")], a.iters)
        res["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    cfg = RNNTConfig(vocab=1024)
    sd = synthetic_transducer_state_dict(cfg, 0, blank_bias=7.0)
    search = TB.RNNTBeamSearch(RNNTGreedy(cfg, sd, "cuda"))
    dev = search.device
    W = {k: v.to(dev) for k, v in sd.items()}
    rnn = torch.nn.LSTM(cfg.embed_size, cfg.hidden, cfg.num_layers, batch_first=True).to(dev)
    rnn.load_state_dict({k[len("predictor.rnn."):]: v for k, v in sd.items() if k.startswith("predictor.rnn.")})
    rnn.eval()
    res = {"device": torch.cuda.get_device_name(0), "dtype": "f32", "iters": a.iters, "weights": [0.3, 0.7],
           "model": {k: getattr(cfg, k) for k in ("vocab", "enc_dim", "embed_size", "hidden", "num_layers", "join_dim")}}
    for key in a.cases.split(","):
        name, B, T = shapes[key]
        for K in (int(v) for v in a.beams.split(",")):
            res[f"{name}_beam{K}"] = run_case(TB, _lib, search, W, rnn, cfg, B, T, K, 1 + ord(key), a.iters,
                                              a.baseline_frames)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
