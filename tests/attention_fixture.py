"""Reader of tests/golden/attention.npz (tests/golden/gen_golden_attention.py) shared by the attention decoding tests."""
import functools
import json
import os

import numpy as np
import torch

from conftest import GOLDEN

from chunkformer_amd.attention_decode import sharpened_decoder_state_dict
from chunkformer_amd.rescore import AEDConfig

FP32_BAR = 1e-4     # the project's fp32 bar on one log-prob; a score after i steps: i x that, a final score (steps + 1) x


@functools.lru_cache(maxsize=None)
def load_models():
    """{model name: dict(cfg, sds {recipe: state dict}, d_bf16, d_f16, cases)}; a case holds enc [rows, d] f32, beam,
    lp, max_len (None or int), recipe, the reference's tokens, and from the f64 host restatement nbest / nbest_scores
    (final-score order), the trace as (parent [steps, N], token [steps, N], score [steps, N] f64), margin, steps."""
    g = np.load(os.path.join(GOLDEN, "attention.npz"))
    meta = json.loads(bytes(g["meta"]).decode())
    out = {}
    for name, m in meta.items():
        cfg = AEDConfig(**m["config"])
        sds = {r: sharpened_decoder_state_dict(cfg, m["weight_seed"], s, o) for r, (s, o) in m["recipes"].items()}
        cases = []
        for u, cm in enumerate(m["cases"]):
            p = f"{name}/c{u:02d}/"
            cut = np.cumsum([0] + g[p + "nbest_lens"].tolist())
            flat = g[p + "nbest"].tolist()
            c = dict(cm)
            c.update(enc=torch.from_numpy(g[p + "enc_q"].astype(np.float32) / 64.0).reshape(-1, cfg.d_model),
                     max_len=None if cm["max_len"] < 0 else int(cm["max_len"]), tokens=g[p + "tokens"].tolist(),
                     nbest=[flat[a:b] for a, b in zip(cut[:-1], cut[1:])], nbest_scores=g[p + "nbest_scores"].tolist(),
                     tr_parent=g[p + "tr_parent"].astype(np.int64), tr_token=g[p + "tr_token"].astype(np.int64),
                     tr_score=g[p + "tr_score"])
            cases.append(c)
        out[name] = {"cfg": cfg, "sds": sds, "d_bf16": m["d_bf16"], "d_f16": m["d_f16"], "cases": cases}
    return out


def case_ids():
    return [(name, k) for name, m in load_models().items() for k in range(len(m["cases"]))]


def check_against_fixture(r, c, score_bar_per_step):
    """A DecodeResult (with trace) against a fixture case: tokens, trace parents and tokens equal, the finite trace
    scores within i x the bar at step i, the chosen final score within (steps + 1) x the bar.  -> the largest score
    error seen, as a multiple of its bar."""
    assert r.tokens == c["tokens"], (r.tokens, c["tokens"])
    assert r.steps == c["steps"]
    worst = 0.0
    for i, (par, tok, sc) in enumerate(r.trace):
        assert list(par) == c["tr_parent"][i].tolist() and list(tok) == c["tr_token"][i].tolist(), f"step {i + 1}"
        for a, b in zip(sc, c["tr_score"][i].tolist()):
            if b == -np.inf:
                assert a == -np.inf
            else:
                bar = (i + 1) * score_bar_per_step
                assert abs(a - b) <= bar, (i + 1, a, b)
                worst = max(worst, abs(a - b) / bar)
    a, b = r.nbest_scores[0], c["nbest_scores"][0]
    if b != b:
        assert a != a
    elif abs(b) == np.inf:
        assert a == b
    else:
        assert abs(a - b) <= (c["steps"] + 1) * score_bar_per_step, (a, b)
    assert r.nbest[0] == c["nbest"][0] == c["tokens"]
    return worst
