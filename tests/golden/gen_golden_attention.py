"""Generate tests/golden/attention.npz from the REFERENCE's attention_beam_search (CPU).

Runs only where the reference checkout is available (CHUNKFORMER_REF, default as gen_golden_rescore.py, whose
namespace shim, torchaudio stub and RefModel this script imports).

    python tests/golden/gen_golden_attention.py

Oracle: the reference's modules/search.py attention_beam_search, unmodified, one utterance per call, on an object
whose `.decoder` is a small adapter of ours.  As shipped the reference cannot run this mode (search.py:294-296 calls
.topk on the (y, cache) tuple forward_one_step returns; behind that DecoderLayer hands MultiHeadedAttention a tuple
cache where it expects a tensor, and search.py:311-317 indexes that tensor as a tuple).  The adapter's
forward_one_step(memory, memory_mask, hyps, hyps_mask, cache) repeats the memory once per beam, calls the
reference's own left_decoder.forward (teacher-forced, uncached) and returns log_softmax of the last row, leaving the
cache empty: the caches are an optimisation only, so this is the reference's semantics computed by the reference's
modules.  Nothing of the reference's text is copied.

Weights: chunkformer_amd.attention_decode.sharpened_decoder_state_dict(cfg, weight_seed, scale, eos_offset): the
plain synthetic head gives degenerate searches (the best hypothesis ends after 0-1 tokens), so the output layer is
scaled and the eos bias moved; the recipes (RECIPES, MODEL_RECIPES) are stored per shape, its name with every case.

Stored per case: the encoder rows (k / 64, k int8), beam size, length penalty, max_len (-1: none), the reference's
tokens, and from our float64 host restatement (which must reproduce the reference's tokens): the N final hypotheses
and final scores in final-score order, the trace (parent, token, score per step and beam), the decision margin, and
the largest deviation of the reference's last-row log-probs under torch.autocast("cpu", bf16 / fp16) from its fp32
values on the recorded prefixes (all V entries of the rows of running beams).

Conditions (seeds advance until they hold; tries are bounded and asserted):
  - every case: margin >= 2 (steps + 1) 1e-4;
  - per shape: >= 3 cases whose winner ended with eos before the limit, >= 3 that ran to the limit, >= 3 distinct
    result lengths, >= 1 case over 64 steps, >= 3 cases whose margin exceeds 2 (steps + 1) d_fp16 (d_fp16 the
    shape's recorded fp16 deviation); the count for bf16 is reported (it may be zero).
"""
from __future__ import annotations

import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_rescore as G  # noqa: E402  (shim + RefModel; its main() does not run on import)

from chunkformer_amd import attention_decode as A  # noqa: E402
from chunkformer_amd import rescore as R  # noqa: E402

ref_search = G.ref_search
OUT = os.path.join(HERE, "attention.npz")
FP32_BAR = 1e-4
RECIPES = {"early": (6.0, 2.5), "mid": (6.0, -0.5), "long": (6.0, -3.0)}   # (scale, eos bias offset)
# the one-directional model's head at scale 6 puts all mass on one token whatever the eos bias: a flatter head there
MODEL_RECIPES = {"uni_d64h4": {"early": (2.5, 2.5), "mid": (2.5, -0.5), "long": (2.5, -3.0)}}
# (rows, beam, length_penalty, max_len, recipe, want): want "early" = only seeds whose winner ended with eos before
# the limit; a number = only seeds whose margin reaches it (one-step cases for the 16-bit token-equality tests)
PLAN = [(0, 10, 0.6, None, "mid", None), (1, 1, 0.0, None, "mid", 0.5), (1, 3, 0.6, None, "mid", 0.5),
        (1, 2, 0.0, None, "mid", 0.5), (1, 10, 0.0, None, "mid", 0.5), (15, 2, 0.0, None, "mid", None),
        (15, 1, 0.6, None, "early", None), (16, 10, 0.0, None, "mid", None), (17, 3, 0.6, None, "early", "early"),
        (31, 16, 0.0, None, "mid", None), (32, 10, 0.6, None, "early", "early"), (33, 10, 0.0, None, "mid", None),
        (33, 16, 0.6, None, "early", "early"), (65, 2, 0.0, None, "long", None), (130, 1, 0.6, None, "long", None),
        (33, 10, 0.0, 12, "mid", None), (16, 2, 0.6, None, "early", "early"), (17, 1, 0.0, None, "long", None)]
MODELS = {name: (kw, seed) for name, (kw, seed, _) in G.MODELS.items()}
MODELS["uni_d64h4"] = (MODELS["uni_d64h4"][0], 15)   # (rescore.npz's seed 14 gives a decoder that never ranks eos high)
MAX_TRIES = 400


class Adapter:
    """forward_one_step for search.attention_beam_search: teacher-forced through the reference's own decoder."""
    use_sdpa = False

    def __init__(self, left):
        self.left = left

    def forward_one_step(self, memory, memory_mask, hyps, hyps_mask, cache):
        n = hyps.shape[0]
        lens = torch.full((n,), hyps.shape[1], dtype=torch.long)
        x, _, _ = self.left.forward(memory.repeat(n, 1, 1), memory_mask.repeat(n, 1, 1), hyps, lens)
        return torch.log_softmax(x[:, -1], dim=-1)


class SearchModel:
    def __init__(self, left, cfg, max_len):
        self.decoder = Adapter(left)
        self.sos, self.eos = cfg.sos, cfg.eos
        if max_len is not None:
            self.decode_maxlen = int(max_len)


def left_of(model: G.RefModel, cfg):
    return model.decoder.left_decoder if cfg.bidirectional else model.decoder


def autocast_dev(left, cfg, enc, trace, beam, dt) -> float:
    """max |autocast - fp32| of the last-row log-probs over the prefixes the trace recorded (running beams)."""
    hyps = [[cfg.sos] for _ in range(beam)]
    alive = [True] + [False] * (beam - 1)
    fin = [False] * beam
    worst = 0.0
    mem = enc.unsqueeze(0)
    mask = torch.ones(1, 1, enc.shape[0], dtype=torch.bool)
    for parents, toks, scores in trace:
        rows = [b for b in range(beam) if alive[b] and not fin[b]]
        if rows:
            ys = torch.tensor([hyps[b] for b in rows], dtype=torch.long)
            lens = torch.full((len(rows),), ys.shape[1], dtype=torch.long)
            m, k = mem.repeat(len(rows), 1, 1), mask.repeat(len(rows), 1, 1)
            with torch.no_grad():
                ref = torch.log_softmax(left.forward(m, k, ys, lens)[0][:, -1], dim=-1)
                with torch.autocast("cpu", dtype=dt):
                    low = torch.log_softmax(left.forward(m, k, ys, lens)[0][:, -1], dim=-1).float()
            worst = max(worst, float((low - ref).abs().max()))
        hyps = [hyps[p] + [t] for p, t in zip(parents, toks)]
        alive = [s > -1e30 for s in scores]
        fin = [t == cfg.eos for t in toks]
    return worst


def run_case(models, cfg, wseed, seed, rows, beam, lp, max_len, recipe, want):
    """One utterance; None when a condition fails (advance the seed)."""
    rng = np.random.default_rng(seed)
    enc_q = rng.integers(-127, 128, (rows, cfg.d_model)).astype(np.int8)
    enc = torch.from_numpy(enc_q.astype(np.float32) / 64.0)
    sd, model = models[recipe]
    limit = A.step_limits([rows], max_len)[0]
    W = {k: v.detach().to("cpu", torch.float64) for k, v in R.native_names(cfg, sd).items()}
    hs = A.HostSearch(cfg, W, R.positional_table(cfg.d_model, R.MAX_POSITIONS, torch.float64), enc.double(), beam,
                      torch.float64)
    for i in range(limit):
        if all(hs.fin):
            break
        hs.step()
        if hs.margin < 2.0 * (i + 2) * FP32_BAR:      # the final need is at least this
            return None
    h = hs.result(lp)
    steps = len(hs.trace)
    if h.margin < 2.0 * (steps + 1) * FP32_BAR:
        return None
    best_row = h.beam_rows[h.best_index]
    early = bool(cfg.eos in best_row and best_row.index(cfg.eos) + 1 < limit)
    if (want == "early" and not early) or (isinstance(want, float) and h.margin < want):
        return None
    left = left_of(model, cfg)
    with torch.no_grad():
        ref = ref_search.attention_beam_search(SearchModel(left, cfg, max_len), enc.unsqueeze(0),
                                               torch.ones(1, 1, rows, dtype=torch.bool), beam, lp)[0]
    if [int(t) for t in ref.tokens] != h.tokens:
        return None      # the reference's f32 run took another branch: a near-tie our margin did not see
    return {"enc_q": enc_q, "beam": beam, "lp": lp, "max_len": -1 if max_len is None else int(max_len),
            "recipe": recipe, "seed": seed, "tokens": h.tokens, "nbest": h.nbest, "nbest_scores": h.nbest_scores,
            "trace": hs.trace, "margin": h.margin, "steps": steps, "limit": limit,
            "early_eos": early,
            "to_limit": steps == limit and limit > 0,
            "d_bf16": autocast_dev(left, cfg, enc, hs.trace, beam, torch.bfloat16),
            "d_f16": autocast_dev(left, cfg, enc, hs.trace, beam, torch.float16)}


def build_model(name):
    kw, wseed = MODELS[name]
    cfg = R.AEDConfig(**kw)
    models = {}
    recipes = MODEL_RECIPES.get(name, RECIPES)
    for rname, (scale, off) in recipes.items():
        sd = A.sharpened_decoder_state_dict(cfg, wseed, scale, off)
        models[rname] = (sd, G.RefModel(cfg, sd))
    cases, seed, tries = [], 5000 * wseed, 0
    for rows, beam, lp, max_len, recipe, want in PLAN:
        k = 0
        while True:
            tries += 1
            k += 1
            assert k <= MAX_TRIES, f"{name}: no seed satisfies the conditions for {(rows, beam, lp, max_len, recipe, want)}"
            c = run_case(models, cfg, wseed, seed, rows, beam, lp, max_len, recipe, want)
            seed += 1
            if c is not None:
                cases.append(c)
                break
    d_bf16 = max(c["d_bf16"] for c in cases)
    d_f16 = max(c["d_f16"] for c in cases)
    n_early = sum(c["early_eos"] for c in cases)
    n_limit = sum(c["to_limit"] for c in cases)
    lens = {len(c["tokens"]) for c in cases}
    n_f16 = sum(c["margin"] > 2.0 * (c["steps"] + 1) * d_f16 for c in cases)
    n_bf16 = sum(c["margin"] > 2.0 * (c["steps"] + 1) * d_bf16 for c in cases)
    print(name, "tries", tries, "early-eos", n_early, "to-limit", n_limit, "lengths", sorted(lens), "steps",
          [c["steps"] for c in cases], f"d_bf16 {d_bf16:.3e} d_f16 {d_f16:.3e}", "16-bit token cases f16", n_f16, "bf16",
          n_bf16, "margins", [f"{c['margin']:.3g}" for c in cases], flush=True)
    assert n_early >= 3 and n_limit >= 3 and len(lens) >= 3 and n_f16 >= 3, (n_early, n_limit, lens, n_f16)
    assert max(c["steps"] for c in cases) > 64
    return cfg, wseed, cases, d_bf16, d_f16, tries, n_f16, n_bf16, recipes


def main():
    torch.set_num_threads(4)
    arrays, meta = {}, {}
    for name in MODELS:
        cfg, wseed, cases, d_bf16, d_f16, tries, n_f16, n_bf16, recipes = build_model(name)
        meta[name] = {"config": {k: getattr(cfg, k) for k in ("vocab", "d_model", "heads", "ff", "num_blocks",
                                                              "r_num_blocks", "eps", "sos", "eos", "bidirectional")},
                      "weight_seed": wseed, "recipes": {k: list(v) for k, v in recipes.items()},
                      "d_bf16": d_bf16, "d_f16": d_f16, "n_token_cases_f16": int(n_f16), "n_token_cases_bf16": int(n_bf16),
                      "cases": [{k: c[k] for k in ("beam", "lp", "max_len", "recipe", "seed", "margin", "steps", "limit",
                                                   "early_eos", "to_limit", "d_bf16", "d_f16")} for c in cases]}
        for u, c in enumerate(cases):
            p = f"{name}/c{u:02d}/"
            arrays[p + "enc_q"] = c["enc_q"]
            arrays[p + "tokens"] = np.array(c["tokens"], np.int32)
            arrays[p + "nbest_lens"] = np.array([len(h) for h in c["nbest"]], np.int32)
            arrays[p + "nbest"] = np.array([t for h in c["nbest"] for t in h], np.int32)
            arrays[p + "nbest_scores"] = np.array(c["nbest_scores"], np.float64)
            arrays[p + "tr_parent"] = np.array([t[0] for t in c["trace"]], np.int8).reshape(-1, c["beam"])
            arrays[p + "tr_token"] = np.array([t[1] for t in c["trace"]], np.int16).reshape(-1, c["beam"])
            arrays[p + "tr_score"] = np.array([t[2] for t in c["trace"]], np.float64).reshape(-1, c["beam"])
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
