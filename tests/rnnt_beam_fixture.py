"""tests/golden/rnnt_beam.npz (gen_golden_rnnt_beam.py) for the transducer beam search tests: models, cases and
the conditions the generator guarantees."""
import functools
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rnnt_beam.npz")


@functools.lru_cache(maxsize=None)
def archive():
    g = np.load(GOLDEN)
    return g, json.loads(bytes(g["meta"]).decode())


@functools.lru_cache(maxsize=None)
def model(name: str, recipe: str):
    """(RNNTConfig, state dict) of a fixture model under a recipe ("dense" / "blank")."""
    from chunkformer_amd.transducer import RNNTConfig, synthetic_transducer_state_dict
    _, meta = archive()
    mm = meta["models"][name]
    cfg = RNNTConfig(**mm["config"])
    return cfg, synthetic_transducer_state_dict(cfg, seed=mm["weight_seed"], blank_bias=mm["recipes"][recipe])


@functools.lru_cache(maxsize=None)
def host_model(name: str, recipe: str):
    from chunkformer_amd.transducer_beam import HostTransducer
    return HostTransducer(*model(name, recipe))


def cases():
    return archive()[1]["cases"]


def case(i: int) -> dict:
    """Inputs and recorded results of case i: enc [rows, enc_dim] f32, ctc [rows, V] f32, beam, cw, tw, the
    reference's final beam (tokens, scores) and the restatement's trace."""
    g, meta = archive()
    c = dict(meta["cases"][i])
    p = f"c{i:03d}/"
    c["enc"] = torch.from_numpy(g[p + "enc_q"].astype(np.float32) / 64.0)
    ctc_all = torch.from_numpy(g[c["model"] + "/ctc"])
    c["ctc"] = torch.roll(ctc_all, -c["ctc_off"], 0)[: c["rows"]].contiguous()
    lens = g[p + "lens"].tolist()
    flat = g[p + "tokens"].tolist()
    c["tokens"], at = [], 0
    for n in lens:
        c["tokens"].append(flat[at: at + n])
        at += n
    c["scores"] = g[p + "scores"].tolist()
    c["trace"] = {k: g[p + "tr_" + k] for k in ("parent", "token", "score")}
    return c
