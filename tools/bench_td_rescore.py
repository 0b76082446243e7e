"""Measure the full-sum transducer score of the transducer rescoring modes (decoding_method "rnnt_beam_attn_rescoring"
/ "ctc_beam_td_attn_rescoring"): cfm_rnnt_td_score and its two kernels, fp32 and bf16, against the reference's
formulation in torch.

    python tools/bench_td_rescore.py [--iters 3] [--cases a,b] [--utts-a N] [--utts-b N] [--predictor rnn|embedding|conv]
                                     [--out profiles/NAME.json]

Model: the vie recipe's predictor and joint (embed 256, LSTM 2 x 512, join_dim J = 512) at enc_dim 512, V = 1,024,
seeded weights (transducer.synthetic_transducer_state_dict); random encoder rows; 10 random hypotheses per utterance.
(a) 256 utterances x 374 rows, ~90 tokens per hypothesis;
(b) the 240-minute batch: 70 utterances x 2,601 rows, ~650 tokens per hypothesis.
`--utts-a` / `--utts-b` measure the first N utterances of a case (the work is linear in the utterances: every
utterance brings its own lattices); the JSON names the count measured.

Per case and dtype, device events around each call after a warm-up, every repeat listed:
  whole       TransducerRescorer.td_scores: grouping (1 GiB of lattice buffers per device call), descriptors, enc_ffn,
              the predictor steps, the lattice kernel, the recursion, the copy back;
  lattice     cfm_op_rnnt_lattice alone over one group of the case (its nodes are named), with its FLOP rate
              2 * nodes * J * V against the MFMA peak of the operand type (157.3 TF f32, 2,500 TF bf16);
  alpha       cfm_op_rnnt_alpha alone over the same group.
Baseline, case (a) only: the reference's formulation of _cal_transducer_score for one utterance in torch on the same
GPU (f32): predictor over the padded hypotheses, the broadcast joint tanh(enc + pred) -> [n_hyps, T, U + 1, V]
logits, log_softmax, and the gather of the blank and target log-probs.  It covers what the reference does up to the
input of rnnt_loss and, instead of torchaudio's loss kernel (not installed here), nothing: the recursion is left out
of the baseline, so the comparison favours the baseline.  It is timed for `--baseline-utts` utterances and scaled to
the case (one utterance at a time, as the reference's batch size 1 has it).

`--predictor embedding|conv` adds, per case, the predictor's share of a td call for a stateless handle of equal widths
(embed = output = 512, history 2, 4 heads) beside the LSTM handle in the same process on the same inputs (fp32): the
whole call of each, and the predictor pass alone -- one cfm_op_rnnt_predictor_step over all the group's states for the
stateless handle, max(U + 1) cfm_op_rnnt_lstm_step calls over the group's hypotheses for the LSTM (as the call runs them).

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = {"fp32": 157.3, "bf16": 2500.0}
CASES = {"a": (256, 374, 90), "b": (70, 2601, 650)}


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
def baseline_one(sd, cfg, rnn, enc, hyps):
    """The reference's formulation for one utterance: joint tensor, log_softmax, gather."""
    lin = torch.nn.functional.linear
    n, U = len(hyps), max(len(h) for h in hyps)
    pad = torch.full((n, U + 1), cfg.blank, dtype=torch.long, device=enc.device)
    for i, h in enumerate(hyps):
        pad[i, 1: len(h) + 1] = torch.tensor(h, device=enc.device)
    out, _ = rnn(sd["predictor.embed.weight"][pad])
    p = lin(out, sd["predictor.projection.weight"], sd["predictor.projection.bias"])
    e = lin(enc, sd["joint.enc_ffn.weight"], sd["joint.enc_ffn.bias"])
    q = lin(p, sd["joint.pred_ffn.weight"], sd["joint.pred_ffn.bias"])
    z = torch.tanh(e.unsqueeze(0).unsqueeze(2) + q.unsqueeze(1))                    # [n, T, U + 1, J]
    lp = lin(z, sd["joint.ffn_out.weight"], sd["joint.ffn_out.bias"]).log_softmax(-1)
    tgt = torch.cat([pad[:, 1:], pad[:, :1]], 1)
    return lp[..., cfg.blank], lp.gather(-1, tgt.view(n, 1, U + 1, 1).expand(n, enc.shape[0], U + 1, 1))


def stateless_config(kind):
    from chunkformer_amd.transducer import RNNTConfig
    return RNNTConfig(embed_size=512, hidden=0, num_layers=0, pred_out=512, join_dim=512, predictor=kind, history_size=2,
                      n_head=4)


def predictor_share(kind, rnnt, enc, starts, lens, nbest, iters):
    """The predictor pass alone and the whole fp32 td call, stateless handle and LSTM handle, same inputs."""
    from chunkformer_amd.transducer import RNNTGreedy, synthetic_transducer_state_dict
    from chunkformer_amd.transducer_beam import RNNTBeamSearch, hyp_windows
    from chunkformer_amd.transducer_rescore import TransducerRescorer, _groups
    dev = enc.device
    scfg = stateless_config(kind)
    sl = RNNTGreedy(scfg, synthetic_transducer_state_dict(scfg, 3, blank_bias=7.0), dev)
    out = {"kind": kind}
    T = lens[0]
    nodes = [T * (len(h) + 1) for hyps in nbest for h in hyps]
    flat = [h for hyps in nbest for h in hyps]
    for key, handle in (("stateless", sl), ("lstm", rnnt)):
        tr = TransducerRescorer(handle, None, "fp32")
        tr.td_scores(enc, starts, lens, nbest)
        whole = statistics.median([timed(lambda: tr.td_scores(enc, starts, lens, nbest)) for _ in range(iters)])
        groups = _groups(nodes, tr.max_lattice_bytes)
        bs = RNNTBeamSearch(handle)
        pred = 0.0
        for grp in groups:
            hyps = [flat[j] for j in grp]
            if key == "stateless":
                win = torch.from_numpy(np.concatenate([hyp_windows(scfg, h) for h in hyps])).to(dev, torch.int32)
                bs.predictor_step(win)
                pred += statistics.median([timed(lambda: bs.predictor_step(win)) for _ in range(iters)])
            else:
                c = handle.cfg
                n, steps = len(hyps), max(len(h) for h in hyps) + 1
                tok = torch.zeros(n, dtype=torch.int32, device=dev)
                h0 = torch.zeros(c.num_layers, n, c.hidden, device=dev)
                bs.lstm_step(tok, h0, h0)
                pred += statistics.median([timed(lambda: bs.lstm_step(tok, h0, h0)) for _ in range(iters)]) * steps
        out[key] = {"whole_ms": whole, "predictor_alone_ms": pred, "predictor_share": pred / whole,
                    "device_calls": len(groups)}
    out["stateless_over_lstm_whole"] = out["stateless"]["whole_ms"] / out["lstm"]["whole_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--utts-a", type=int, default=256)
    ap.add_argument("--utts-b", type=int, default=70)
    ap.add_argument("--baseline-utts", type=int, default=4)
    ap.add_argument("--predictor", default="rnn", choices=("rnn", "embedding", "conv"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from chunkformer_amd.transducer import RNNTConfig, RNNTGreedy, synthetic_transducer_state_dict
    from chunkformer_amd.transducer_rescore import TransducerRescorer, _groups, alpha_device
    dev = torch.device("cuda:0")
    cfg = RNNTConfig()
    sd = synthetic_transducer_state_dict(cfg, 3, blank_bias=7.0)
    rnnt = RNNTGreedy(cfg, sd, dev)
    res = {"model": {"J": cfg.join_dim, "V": cfg.vocab, "hyps": 10}, "cases": {}}
    g = np.random.default_rng(0)
    for name in args.cases.split(","):
        B_full, T, U = CASES[name]
        B = min(B_full, args.utts_a if name == "a" else args.utts_b)
        enc = torch.randn(B * T, cfg.enc_dim, generator=torch.Generator().manual_seed(1)).to(dev)
        starts, lens = [b * T for b in range(B)], [T] * B
        nbest = [[g.integers(1, cfg.vocab, size=int(g.integers(U - U // 10, U + U // 10 + 1))).tolist() for _ in range(10)]
                 for _ in range(B)]
        nodes = [T * (len(h) + 1) for hyps in nbest for h in hyps]
        out = {"utterances": B, "of": B_full, "rows": T, "tokens": U, "nodes": int(sum(nodes))}
        for dtype in ("fp32", "bf16"):
            tr = TransducerRescorer(rnnt, None, dtype)
            tr.td_scores(enc, starts, lens, nbest)   # warm-up (weights repack, allocator)
            whole = [timed(lambda: tr.td_scores(enc, starts, lens, nbest)) for _ in range(args.iters)]
            # one group of the case for the kernels alone
            grp = _groups(nodes, tr.max_lattice_bytes)[0]
            flat = [(b, h) for b, hyps in enumerate(nbest) for h in hyps]
            hyps = [flat[j] for j in grp]
            n_states = sum(len(h) + 1 for _, h in hyps)
            e = torch.randn(B * T, cfg.join_dim, device=dev)
            p = torch.randn(n_states, cfg.join_dim, device=dev)
            gn = int(sum(nodes[j] for j in grp))
            tr.lattice(e, p[: len(hyps[0][1]) + 1], starts, lens, hyps[:1], dtype)   # warm-up
            lat = [timed(lambda: tr.lattice(e, p, starts, lens, hyps, dtype)) for _ in range(args.iters)]
            # (tr.lattice copies b / k back to the host inside the timed region: the copy is subtracted by timing it)
            cp = torch.empty(2 * gn, dtype=torch.float32, device=dev)
            copy = statistics.median([timed(lambda: cp.cpu()) for _ in range(args.iters)])
            med = max(statistics.median(lat) - copy, 1e-3)
            tf = 2.0 * gn * cfg.join_dim * cfg.vocab / (med * 1e-3) / 1e12
            lats = [(np.full((T, len(h) + 1), -1.0, np.float32), np.full((T, len(h)), -2.0, np.float32)) for _, h in hyps[:40]]
            alpha_device(lats[:1], dev)
            al = [timed(lambda: alpha_device(lats, dev)) for _ in range(args.iters)]
            out[dtype] = {"whole": spread(whole), "device_calls": tr.last_groups,
                          "lattice": dict(spread(lat), nodes=gn, copy_back_ms=copy, kernel_ms=med, tflops=tf,
                                          fraction_of_peak=tf / PEAK_TF[dtype]),
                          "alpha_40_hyps_with_copies": spread(al)}
        if name == "a":
            dsd = {k: v.to(dev) for k, v in sd.items()}
            rnn = torch.nn.LSTM(cfg.embed_size, cfg.hidden, cfg.num_layers, batch_first=True).to(dev)
            rnn.load_state_dict({k[len("predictor.rnn."):]: v for k, v in sd.items() if k.startswith("predictor.rnn.")})
            nb = min(args.baseline_utts, B)
            run = lambda: [baseline_one(dsd, cfg, rnn, enc[b * T: (b + 1) * T], nbest[b]) for b in range(nb)]   # noqa: E731
            run()
            bl = [timed(run) for _ in range(args.iters)]
            out["baseline_torch_f32"] = dict(spread(bl), utterances=nb,
                                             scaled_to_case_ms=statistics.median(bl) * B / nb,
                                             covers="predictor, joint tensor, log_softmax, gather; not the loss recursion")
            for dtype in ("fp32", "bf16"):
                out[dtype]["speedup_vs_baseline"] = out["baseline_torch_f32"]["scaled_to_case_ms"] / out[dtype]["whole"]["median_ms"]
        if args.predictor != "rnn":
            out["predictor"] = predictor_share(args.predictor, rnnt, enc, starts, lens, nbest, args.iters)
        res["cases"][name] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
