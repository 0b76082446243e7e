"""Measure the CTC prefix beam search: the per-frame top-k, the beam kernel, and the host fallback.

    python tools/bench_beam.py [--rows 182080] [--k 10] [--iters 5] [--out profiles/NAME.json]
    python tools/bench_beam.py --host-only [--reference PATH/TO/chunkformer]

1. cfm_ctc_topk against cfm_ctc_logprobs (log-probs written) on the same rows of the 240-minute batch
   (182,080 x 5,000, k = 10), alternating the two in one process.  The cfm_ctc_logprobs path is the
   parent commit's code (its head GEMM only moved into a helper), so this is the old-against-new
   comparison.  Times are device events around each call, after a warm-up; bytes are counted from the
   shapes (logits read once + [rows, k] written, against three reads and one write).
2. The beam kernel's time per frame for 70 utterances of rows / 70 frames each in one call, and for one
   16-hour utterance (720,000 frames), on top-k rows of a CTC-like random stream.
3. With --host-only (no GPU): the host fallback on one 2,570-frame utterance, and, when the
   reference's package directory is given, its own ctc_prefix_beam_search with score() patched as in
   tests/golden/gen_golden_beam.py.

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
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ctc_like_stream(T: int, V: int, seed: int) -> torch.Tensor:
    """Log-probs [T, V] of a peaked stream: blank runs, tokens of 1-3 frames, a rival now and then."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, V, generator=g)
    lab = torch.randint(1, V, (T,), generator=g)
    keep = torch.rand(T, generator=g) < 0.45
    lab = torch.where(keep, lab, torch.zeros_like(lab))
    x[torch.arange(T), lab] += 6.0
    return torch.log_softmax(x, -1)


def timed(fn, iters: int):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def bench_topk(rows: int, k: int, iters: int) -> dict:
    from chunkformer_amd import _lib
    from chunkformer_amd.config import LARGE
    from chunkformer_amd.encoder import ChunkFormerEncoder
    from chunkformer_amd.weights import synthetic_state_dict
    cfg = dataclasses.replace(LARGE, num_blocks=1)
    enc = ChunkFormerEncoder(cfg, synthetic_state_dict(cfg, 0), dtype="bf16")
    dev, V, d = enc.device, cfg.vocab, cfg.d_model
    hs = torch.randn(rows, d, generator=torch.Generator().manual_seed(1)).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    vals = torch.empty(rows, k, device=dev)
    ids = torch.empty(rows, k, dtype=torch.int32, device=dev)
    nb_t = int(_lib.cfm_ctc_topk_workspace_bytes(enc._h, rows, k))
    ws_t = torch.empty(nb_t, dtype=torch.uint8, device=dev)
    logp = torch.empty(rows, V, device=dev)
    nb_l = int(_lib.cfm_ctc_workspace_bytes(enc._h, rows))
    ws_l = torch.empty(nb_l, dtype=torch.uint8, device=dev)

    def new():
        _lib.check(_lib.cfm_ctc_topk(enc._h, hs.data_ptr(), rows, k, vals.data_ptr(), ids.data_ptr(), ws_t.data_ptr(),
                                     nb_t, st))

    def old():
        _lib.check(_lib.cfm_ctc_logprobs(enc._h, hs.data_ptr(), rows, logp.data_ptr(), None, ws_l.data_ptr(), nb_l, st))

    t_new, t_old = [], []
    for _ in range(iters):   # alternate the two
        t_new += timed(new, 1)
        t_old += timed(old, 1)
    order = torch.sort(logp[:4096], dim=-1, descending=True, stable=True).indices[:, :k]
    same = bool(torch.equal(ids[:4096].long(), order) and torch.equal(vals[:4096], torch.gather(logp[:4096], 1, order)))
    logit_bytes = rows * V * 4
    return {"rows": rows, "V": V, "k": k, "dtype": "bf16", "slab_rows": enc.ctc_topk_slab_rows(),
            "ctc_topk_ms": t_new, "ctc_logprobs_ms": t_old,
            "ctc_topk_ms_median": statistics.median(t_new), "ctc_logprobs_ms_median": statistics.median(t_old),
            "topk_workspace_bytes": nb_t, "logprobs_workspace_plus_output_bytes": nb_l + logit_bytes,
            "tail_bytes_new": logit_bytes + rows * k * 8, "tail_bytes_old": 4 * logit_bytes,
            "first_4096_rows_equal_stable_topk_of_logprobs": same}


def bench_beam(rows: int, k: int, iters: int) -> dict:
    from chunkformer_amd import _lib, search
    out = {}
    for name, T, B in (("batch_70_utterances", rows // 70, 70), ("one_16_hour_utterance", 720_000, 1)):
        logp = ctc_like_stream(T * B, 64, 3).cuda()
        vals, ids = search.topk_logp_device(logp, k)
        del logp
        n = T * B
        dev = vals.device
        rs = torch.arange(B, dtype=torch.int32, device=dev) * T
        rl = torch.full((B,), T, dtype=torch.int32, device=dev)
        nbytes = int(_lib.cfm_ctc_beam_workspace_bytes(n, B, k, 1, 0))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        tok = torch.empty(k, n, dtype=torch.int32, device=dev)
        tim = torch.empty(k, n, dtype=torch.int32, device=dev)
        ln = torch.zeros(B, k, dtype=torch.int32, device=dev)
        sc = torch.zeros(B, k, dtype=torch.float64, device=dev)
        nh = torch.zeros(B, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream

        def run():
            _lib.check(_lib.cfm_ctc_beam_search(vals.data_ptr(), ids.data_ptr(), n, k, rs.data_ptr(), rl.data_ptr(), B,
                                                0, None, tok.data_ptr(), tim.data_ptr(), ln.data_ptr(), sc.data_ptr(),
                                                nh.data_ptr(), ws.data_ptr(), nbytes, st))

        ts = timed(run, iters)
        assert int(ws[:4].view(torch.int32).item()) == 0
        out[name] = {"frames_per_utterance": T, "utterances": B, "k": k, "call_ms": ts,
                     "us_per_frame_of_one_utterance": statistics.median(ts) * 1e3 / T,
                     "workspace_bytes": nbytes, "hyps": nh[:2].tolist(), "best_len": ln[0, 0].item()}
    return out


def bench_host(k: int, reference: str | None) -> dict:
    import importlib.util
    spec = importlib.util.spec_from_file_location("cfm_search", os.path.join(ROOT, "chunkformer_amd", "search.py"))
    search = importlib.util.module_from_spec(spec)
    sys.modules["cfm_search"] = search
    spec.loader.exec_module(search)
    T = 2570
    logp = ctc_like_stream(T, 5000, 5)
    t0 = time.perf_counter()
    mine = search.ctc_prefix_beam_search(logp[None], [T], k)[0]
    out = {"frames": T, "V": 5000, "k": k, "host_fallback_s": time.perf_counter() - t0, "best_tokens": len(mine.tokens)}
    if reference:
        pkg = types.ModuleType("chunkformer")
        pkg.__path__ = [reference]
        sys.modules["chunkformer"] = pkg
        ta, taf = types.ModuleType("torchaudio"), types.ModuleType("torchaudio.functional")
        ta.functional = taf
        sys.modules.setdefault("torchaudio", ta)
        sys.modules.setdefault("torchaudio.functional", taf)
        from chunkformer.modules import search as ref
        from chunkformer.utils.common import log_add
        ref.PrefixScore.score = lambda self: log_add([self.s, self.ns])
        t0 = time.perf_counter()
        theirs = ref.ctc_prefix_beam_search(logp[None], torch.tensor([T]), k)[0]
        out["patched_reference_s"] = time.perf_counter() - t0
        out["same_nbest"] = theirs.nbest == mine.nbest
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=182080)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.host_only:
        res = {"host": bench_host(a.k, a.reference)}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench_beam.py measures on the GPU (or pass --host-only)")
        res = {"device": torch.cuda.get_device_name(0), "topk": bench_topk(a.rows, a.k, a.iters),
               "beam": bench_beam(a.rows, a.k, a.iters)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
