"""tests/golden/rnnt_stateless.npz (gen_golden_stateless.py) for the stateless-predictor tests: models, recorded
reference results and the conditions the generator guarantees."""
import functools
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rnnt_stateless.npz")


@functools.lru_cache(maxsize=None)
def archive():
    g = np.load(GOLDEN)
    return g, json.loads(bytes(g["meta"]).decode())


def names():
    return sorted(archive()[1]["models"])


@functools.lru_cache(maxsize=None)
def model(name: str):
    """(RNNTConfig, state dict) of a fixture model."""
    from chunkformer_amd.transducer import RNNTConfig, synthetic_transducer_state_dict
    mm = archive()[1]["models"][name]
    cfg = RNNTConfig(**mm["config"])
    return cfg, synthetic_transducer_state_dict(cfg, seed=mm["weight_seed"], blank_bias=mm["blank_bias"])


@functools.lru_cache(maxsize=None)
def host_model(name: str):
    from chunkformer_amd.transducer_beam import HostTransducer
    return HostTransducer(*model(name))


def _split(flat, lens):
    out, at = [], 0
    for n in lens:
        out.append([int(t) for t in flat[at: at + n]])
        at += n
    return out


def _enc(g, p):
    return torch.from_numpy(g[p + "enc_q"].astype(np.float32) / 64.0)


def predictor_points(name: str):
    """(windows [n, K] int64, the reference's f32 forward_step outputs [n, E], its own error e_ref against f64)."""
    g, meta = archive()
    return g[name + "/win"].astype(np.int64), g[name + "/pred"], float(meta["models"][name]["e_ref"])


def greedy_cases(name: str):
    g, meta = archive()
    out = []
    for i, c in enumerate(meta["models"][name]["greedy"]):
        p = f"{name}/g{i}/"
        c = dict(c)
        c["enc"] = _enc(g, p)
        c["starts"] = np.concatenate([[0], np.cumsum(c["lens"])[:-1]]).astype(int).tolist()
        c["dense"] = g[p + "dense"].astype(np.int32)
        c["ref_tokens"] = _split(g[p + "ref_tokens"].tolist(), g[p + "ref_lens"].tolist())
        out.append(c)
    return out


def beam_cases(name: str):
    g, meta = archive()
    ctc_all = torch.from_numpy(g[name + "/ctc"])
    out = []
    for i, c in enumerate(meta["models"][name]["beam"]):
        p = f"{name}/b{i}/"
        c = dict(c)
        c["enc"] = _enc(g, p)
        c["ctc"] = torch.roll(ctc_all, -c["ctc_off"], 0)[: c["rows"]].contiguous()
        c["tokens"] = _split(g[p + "tokens"].tolist(), g[p + "lens"].tolist())
        c["scores"] = g[p + "scores"].tolist()
        c["trace"] = {k: g[p + "tr_" + k] for k in ("parent", "token", "score")}
        c["td"] = g[p + "td"].tolist()
        c["totals"] = g[p + "totals"].tolist()
        out.append(c)
    return out


def td_cases(name: str):
    g, meta = archive()
    out = []
    for i, c in enumerate(meta["models"][name]["td"]):
        p = f"{name}/t{i}/"
        c = dict(c)
        c["enc"] = _enc(g, p)
        c["hyps"] = _split(g[p + "tokens"].tolist(), g[p + "lens"].tolist())
        c["td_ref"] = g[p + "td_ref"].tolist()
        c["td"] = g[p + "td"].tolist()
        out.append(c)
    return out
