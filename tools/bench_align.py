"""Measure CTC forced alignment: the trellis + backtrace kernels against the host restatement.

    python tools/bench_align.py [--iters 5] [--host-fraction 1.0] [--out profiles/NAME.json]

(a) The 240-minute batch geometry in one call: 70 utterances x 2,601 frames, V = 5,000, targets of
    0.25 tokens per frame (650 tokens, S = 1,301 states).  The log-probs are the one-block d512 head's
    (cfm_ctc_logprobs, bf16 model), whose time is reported separately; the two calls alternate in one
    process.
(b) One one-hour utterance: 45,000 frames, 12,000 tokens (S = 24,001: three strips, alpha rows in the
    workspace, a 270 MB trellis), with its microseconds per frame.

Times are device events around each call after a warm-up; every repeat is listed, with median, min and
max.  The baseline is align.force_align_host (numpy f64, one core) on the same inputs: every utterance
of (a), and the first --host-fraction of (b)'s frames and tokens (1.0 = all of them; the fraction is
recorded).  Frames, spans and scores of the host runs are compared with the device's, bit for bit.
torchaudio is not part of this build, so the reference's own forced_align is not measured.

Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

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


class AlignCall:
    """cfm_ctc_align with every buffer allocated once: run() is the two kernel launches only."""

    def __init__(self, logp, starts, lens, targets):
        from chunkformer_amd import _lib
        self._lib = _lib
        dev = logp.device
        self.logp, self.B = logp, len(starts)
        self.rows, self.V = logp.shape
        tl = [len(t) for t in targets]
        ts = [sum(tl[:b]) for b in range(self.B)]
        self.n_t = sum(tl)
        self.rl_h = torch.tensor(lens, dtype=torch.int32)
        self.tl_h = torch.tensor(tl, dtype=torch.int32)
        off = torch.zeros(self.B, dtype=torch.int64)
        self.nbytes = int(_lib.cfm_ctc_align_plan(self.rl_h.data_ptr(), self.tl_h.data_ptr(), self.B, off.data_ptr()))
        self.d = [t.to(dev) for t in (torch.tensor(starts, dtype=torch.int32), self.rl_h,
                                      torch.tensor([v for t in targets for v in t], dtype=torch.int32),
                                      torch.tensor(ts, dtype=torch.int32), self.tl_h, off)]
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.frames = torch.full((self.rows,), -7, dtype=torch.int32, device=dev)
        self.flp = torch.empty(self.rows, dtype=torch.float32, device=dev)
        self.spans = torch.full((self.n_t, 2), -7, dtype=torch.int32, device=dev)
        self.score = torch.zeros(self.B, dtype=torch.float64, device=dev)
        self.status = torch.full((self.B,), -1, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.tstart = ts

    def run(self):
        d = self.d
        self._lib.check(self._lib.cfm_ctc_align(
            self.logp.data_ptr(), self.rows, self.V, d[0].data_ptr(), d[1].data_ptr(), self.B, 0, d[2].data_ptr(),
            self.n_t, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), self.rl_h.data_ptr(), self.tl_h.data_ptr(),
            self.frames.data_ptr(), self.flp.data_ptr(), self.spans.data_ptr(), self.score.data_ptr(),
            self.status.data_ptr(), -1, 0, self.ws.data_ptr(), self.nbytes, self.stream))


def random_targets(B, L, V, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(1, V, (L,), generator=g).tolist() for _ in range(B)]


def host_compare(align, call, logp, starts, lens, targets, which, fraction=1.0):
    """force_align_host on utterances `which` (the first `fraction` of frames and tokens), timed on one
    core; with fraction 1 the result is compared with the device's."""
    fr, sp, sc = call.frames.cpu(), call.spans.cpu(), call.score.cpu()
    secs, same = [], True
    for b in which:
        n, y = int(lens[b] * fraction), targets[b][: int(len(targets[b]) * fraction)]
        lp = logp[starts[b]: starts[b] + n].cpu()
        t0 = time.perf_counter()
        r = align.force_align_host(lp, y)
        secs.append(time.perf_counter() - t0)
        if fraction == 1.0:
            t0_ = call.tstart[b]
            same = same and r.frames == fr[starts[b]: starts[b] + n].tolist() and r.score == float(sc[b]) and \
                [list(p) for p in r.spans] == sp[t0_: t0_ + len(y)].tolist()
    return secs, (same if fraction == 1.0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-fraction", type=float, default=1.0, help="part of case (b) the host baseline runs")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align.py measures on the GPU")
    torch.set_num_threads(1)
    from chunkformer_amd import _lib, align
    from chunkformer_amd.config import LARGE
    from chunkformer_amd.encoder import ChunkFormerEncoder
    from chunkformer_amd.weights import synthetic_state_dict
    cfg = dataclasses.replace(LARGE, num_blocks=1)
    enc = ChunkFormerEncoder(cfg, synthetic_state_dict(cfg, 0), dtype="bf16")
    dev, V, d = enc.device, cfg.vocab, cfg.d_model
    st = torch.cuda.current_stream(dev).cuda_stream
    res = {"device": torch.cuda.get_device_name(0), "V": V, "iters": a.iters}

    def logprobs_call(rows, seed):
        hs = torch.randn(rows, d, generator=torch.Generator().manual_seed(seed)).to(dev)
        logp = torch.empty(rows, V, device=dev)
        nb = int(_lib.cfm_ctc_workspace_bytes(enc._h, rows))
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)

        def run():
            _lib.check(_lib.cfm_ctc_logprobs(enc._h, hs.data_ptr(), rows, logp.data_ptr(), None, ws.data_ptr(), nb, st))
        return logp, run

    # (a) the 240-minute batch
    B, T, L = 70, 2601, 650
    logp, lsm = logprobs_call(B * T, 1)
    lsm()
    starts, lens, targets = [b * T for b in range(B)], [T] * B, random_targets(B, L, V, 2)
    call = AlignCall(logp, starts, lens, targets)
    call.run()
    torch.cuda.synchronize()
    t_al, t_ls = [], []
    for _ in range(a.iters):      # alternate the two
        t_al.append(timed(call.run))
        t_ls.append(timed(lsm))
    assert call.status.cpu().tolist() == [0] * B
    ra = {"utterances": B, "frames_per_utterance": T, "tokens_per_utterance": L, "states": 2 * L + 1,
          "align": spread(t_al), "log_softmax": spread(t_ls), "workspace_bytes": call.nbytes,
          "us_per_frame_of_one_utterance": statistics.median(t_al) * 1e3 / T}
    if not a.skip_host:
        secs, same = host_compare(align, call, logp, starts, lens, targets, range(B))
        ra.update({"host_s_total": sum(secs), "host_s_per_utterance_median": statistics.median(secs),
                   "host_utterances": B, "host_equals_device": same,
                   "speedup_vs_host": sum(secs) * 1e3 / statistics.median(t_al)})
    res["batch_70_utterances"] = ra
    del call, logp, lsm

    # (b) one one-hour utterance
    T, L = 45000, 12000
    logp, lsm = logprobs_call(T, 3)
    lsm()
    targets = random_targets(1, L, V, 4)
    call = AlignCall(logp, [0], [T], targets)
    call.run()
    torch.cuda.synchronize()
    t_al, t_ls = [], []
    for _ in range(a.iters):
        t_al.append(timed(call.run))
        t_ls.append(timed(lsm))
    assert call.status.cpu().tolist() == [0]
    rb = {"frames": T, "tokens": L, "states": 2 * L + 1, "align": spread(t_al), "log_softmax": spread(t_ls),
          "workspace_bytes": call.nbytes, "us_per_frame": statistics.median(t_al) * 1e3 / T}
    if not a.skip_host:
        secs, same = host_compare(align, call, logp, [0], [T], targets, [0], a.host_fraction)
        rb.update({"host_s": secs[0], "host_fraction_of_frames_and_tokens": a.host_fraction,
                   "host_equals_device": same})
        if a.host_fraction == 1.0:
            rb["speedup_vs_host"] = secs[0] * 1e3 / statistics.median(t_al)
    res["one_hour_utterance"] = rb

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
