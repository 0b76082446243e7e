"""Reader of tests/golden/beam.npz (tests/golden/gen_golden_beam.py) shared by the beam-search tests."""
import functools
import json
import os

import numpy as np

from conftest import GOLDEN


def score_tol(k: int, T: int, score: float) -> float:
    """Derived, not measured: s and ns each pass through at most k + 1 log_adds and a few additions
    per frame; 16 ulp for each of these (k + 2) operations over T frames."""
    return 16.0 * (k + 2) * max(T, 1) * 2.0 ** -53 * max(1.0, abs(score))


@functools.lru_cache(maxsize=None)
def load_cases():
    """{name: case}; a case holds k, vals / ids [T, k], phrases / context_score (or None), the expected
    nbest / scores / times, and for context cases graph_steps [n, 4] / graph_final."""
    g = np.load(os.path.join(GOLDEN, "beam.npz"))
    meta = json.loads(bytes(g["meta"]).decode())
    cases = {}
    for name, m in meta.items():
        lens = g[name + "/lens"].tolist()
        cut = np.cumsum([0] + lens)
        tok, tim = g[name + "/tokens"].tolist(), g[name + "/times"].tolist()
        c = dict(m)
        c.update(vals=g[name + "/vals"], ids=g[name + "/ids"], scores=g[name + "/scores"].tolist(),
                 nbest=[tok[a:b] for a, b in zip(cut[:-1], cut[1:])],
                 times=[tim[a:b] for a, b in zip(cut[:-1], cut[1:])])
        if name + "/graph_steps" in g.files:
            c["graph_steps"], c["graph_final"] = g[name + "/graph_steps"], g[name + "/graph_final"]
        cases[name] = c
    return cases


def check_result(name, case, r):
    """Tokens, times and hypothesis counts equal; scores within the derived tolerance."""
    T, k = case["vals"].shape[0], case["k"]
    assert r.nbest == case["nbest"], name
    assert r.nbest_times == case["times"], name
    assert len(r.nbest_scores) == len(case["scores"]), name
    for got, exp in zip(r.nbest_scores, case["scores"]):
        assert abs(got - exp) <= score_tol(k, T, exp), (name, got, exp)
    assert r.tokens == case["nbest"][0] and r.times == case["times"][0] and r.score == r.nbest_scores[0], name
