"""Reader of tests/golden/rescore.npz (tests/golden/gen_golden_rescore.py) shared by the rescoring tests."""
import functools
import json
import os

import numpy as np
import torch

from conftest import GOLDEN

from chunkformer_amd.rescore import AEDConfig, synthetic_decoder_state_dict
from chunkformer_amd.search import DecodeResult

DIRS = ("l2r", "r2l")


def _split(flat, lens):
    cut = np.cumsum([0] + list(lens))
    return [flat[a:b] for a, b in zip(cut[:-1], cut[1:])]


@functools.lru_cache(maxsize=None)
def load_models():
    """{model name: dict(cfg, sd, combos, utts)}; an utterance holds enc [rows, d] f32, hyps, ctc, times, per
    hypothesis the reference's target log-probs l2r / r2l (rows n + 1; r2l None without a right decoder) in fp32 and
    as `l2r_bf16` .. from its autocast runs, exp [4, 3] = (index, total, confidence) per weight combination and
    tcs[k] the chosen hypothesis' token confidences."""
    g = np.load(os.path.join(GOLDEN, "rescore.npz"))
    meta = json.loads(bytes(g["meta"]).decode())
    out = {}
    for name, m in meta.items():
        cfg = AEDConfig(**m["config"])
        utts = []
        for u in range(m["n_utt"]):
            p = f"{name}/u{u:02d}/"
            lens = g[p + "lens"].tolist()
            c = {"enc": torch.from_numpy(g[p + "enc_q"].astype(np.float32) / 64.0), "lens": lens,
                 "hyps": [x.tolist() for x in _split(g[p + "tokens"], lens)],
                 "times": [x.tolist() for x in _split(g[p + "times"], lens)], "ctc": g[p + "ctc"].tolist(),
                 "exp": g[p + "exp"], "tcs": [g[p + f"tc{k}"] for k in range(len(m["combos"]))]}
            for k in ("l2r", "r2l", "l2r_bf16", "r2l_bf16", "l2r_f16", "r2l_f16"):
                c[k] = _split(g[p + k], [n + 1 for n in lens]) if p + k in g.files else None
            utts.append(c)
        out[name] = {"cfg": cfg, "sd": synthetic_decoder_state_dict(cfg, m["weight_seed"]),
                     "combos": [tuple(x) for x in m["combos"]], "utts": utts,
                     "autocast_max_dev": m["autocast_max_dev"]}
    return out


def packed(utts):
    """The utterances of one model as one call's inputs: (enc_rows, row_start, row_len, results)."""
    rows = [int(u["enc"].shape[0]) for u in utts]
    starts = np.cumsum([0] + rows[:-1]).tolist()
    enc = torch.cat([u["enc"] for u in utts]) if utts else torch.zeros(0, 1)
    res = [DecodeResult(u["hyps"][0], nbest=u["hyps"], nbest_scores=u["ctc"], nbest_times=u["times"]) for u in utts]
    return enc, starts, rows, res


def token_errors(scored, utts, suffix=""):
    """|got - reference| over every token row of every hypothesis, both directions -> 1-D float64 array."""
    errs = []
    for sc, u in zip(scored, utts):
        for i in range(len(u["hyps"])):
            for k, d in enumerate(DIRS):
                ref = u[d]   # the fp32 reference values, whatever run `suffix` names
                if ref is None or sc[i][k] is None:
                    continue
                errs.append(np.abs(np.asarray(sc[i][k], np.float64) - ref[i].astype(np.float64)))
    return np.concatenate(errs)


def reference_deviation(utts, suffix):
    """The reference's own |autocast - fp32| over the same rows (the 16-bit yardstick)."""
    errs = []
    for u in utts:
        for d in DIRS:
            if u[d] is None:
                continue
            for a, b in zip(u[d + "_" + suffix], u[d]):
                errs.append(np.abs(a.astype(np.float64) - b.astype(np.float64)))
    return np.concatenate(errs)
