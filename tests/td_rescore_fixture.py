"""tests/golden/td_rescore.npz (gen_golden_td_rescore.py) for the transducer rescoring tests: the cases over the
models and beams of rnnt_beam.npz, the seeded attention decoders, and the recorded scores and choices."""
import functools
import json
import os

import numpy as np

import rnnt_beam_fixture as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "td_rescore.npz")


@functools.lru_cache(maxsize=None)
def archive():
    g = np.load(GOLDEN)
    return g, json.loads(bytes(g["meta"]).decode())


def cases():
    return archive()[1]["cases"]


@functools.lru_cache(maxsize=None)
def decoder(kind: str, vocab: int):
    """(AEDConfig, state dict) of the fixture's `transformer` ("uni") / `bitransformer` ("bi") decoder."""
    from chunkformer_amd import rescore as R
    cfg = R.AEDConfig(vocab=vocab, d_model=32, heads=2, ff=64, num_blocks=1, r_num_blocks=1 if kind == "bi" else 0,
                      bidirectional=kind == "bi")
    return cfg, R.synthetic_decoder_state_dict(cfg, archive()[1]["decoder_seed"][kind])


def case(i: int) -> dict:
    """Case i: its meta, enc [rows, enc_dim] f32, the n-best (tokens, search scores) as a DecodeResult, and the
    recorded td / attn / totals per hypothesis."""
    from chunkformer_amd.search import DecodeResult
    g, meta = archive()
    c = dict(meta["cases"][i])
    p = f"c{i:03d}/"
    c["enc"] = F.case(c["src"])["enc"]
    flat, at, nbest = g[p + "tokens"].tolist(), 0, []
    for n in g[p + "lens"].tolist():
        nbest.append(flat[at: at + n])
        at += n
    scores = g[p + "search"].tolist()
    c["result"] = DecodeResult(list(nbest[0]), scores[0], nbest=nbest, nbest_scores=scores)
    for k in ("td", "attn", "totals"):
        c[k] = g[p + k].tolist()
    return c
