"""Generate tests/golden/beam.npz from the REFERENCE CTC prefix beam search (CPU).

Runs only in the build container: it imports the reference through the same namespace shim as
gen_golden.py, with an empty `torchaudio` stub (modules/search.py pulls utils/model_utils.py, which
imports torchaudio.functional at module level and does not use it here).

    python tests/golden/gen_golden_beam.py

The one deviation from the reference as shipped: `PrefixScore.score()` calls `log_add(self.s, self.ns)`
while utils/common.py defines `log_add(arr)`, so the shipped function raises TypeError on its first
frame.  This script sets `PrefixScore.score = lambda self: log_add([self.s, self.ns])` at run time;
nothing else of the reference is changed and none of its text is copied.  The reference ContextGraph
reads a phrase file; a subclass here skips that constructor and calls its `build_graph` on token lists.

The fixture stores only what the search consumes and produces: per case the [T, k] values and
indices that the reference's own `logp.topk(k)` returned, the lengths, the phrases, the expected
n-best (tokens, total scores, times), and for the context graphs the reference's `forward_one_step`
/ `finalize` results on every node and a sample of tokens.  Full log-prob tensors are not stored.

Seeds advance until, for every case: no exact ties among the first k + 1 log-probs of any frame; the
first k + 1 ranked candidates of every frame differ pairwise (neighbours) by at least 100 x the
score tolerance of the tests; no candidate at -inf is ever kept; at least one context case changes
the 1-best; and the churn set holds at least 10 re-entries of a prefix while a descendant is live.
The last three are measured with the project's host restatement, which this script first requires
to reproduce the reference's n-best exactly on the same case.

The archive is written with fixed zip timestamps so that it regenerates bit-identically.
"""
from __future__ import annotations

import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

REF = "/root/reference/chunkformer"
m = types.ModuleType("chunkformer")
m.__path__ = [REF]
sys.modules["chunkformer"] = m
ta = types.ModuleType("torchaudio")
taf = types.ModuleType("torchaudio.functional")
ta.functional = taf
sys.modules.setdefault("torchaudio", ta)
sys.modules.setdefault("torchaudio.functional", taf)

from chunkformer.modules import search as ref_search  # noqa: E402
from chunkformer.utils import context_graph as ref_cg  # noqa: E402
from chunkformer.utils.common import log_add  # noqa: E402

ref_search.PrefixScore.score = lambda self: log_add([self.s, self.ns])   # the one deviation (see above)

# the host restatement only (no libcfm needed): load search.py as a stand-alone module
import importlib.util  # noqa: E402

_spec = importlib.util.spec_from_file_location("cfm_search", os.path.join(ROOT, "chunkformer_amd", "search.py"))
host = importlib.util.module_from_spec(_spec)
sys.modules["cfm_search"] = host
_spec.loader.exec_module(host)

torch.set_num_threads(4)
OUT = os.path.join(HERE, "beam.npz")


def score_tol(k: int, T: int, score: float) -> float:
    """The tests' derived score tolerance: 16 ulp for each of (k + 2) operations per frame."""
    return 16.0 * (k + 2) * max(T, 1) * 2.0 ** -53 * max(1.0, abs(score))


def _record(stats: dict, prev, ranked, k: int, node_parent) -> None:
    """Statistics of one frame's prune for the fixture generator: candidates kept at -inf, the smallest
    relative gap among the first k + 1 totals, and prefixes that re-enter the beam (their node exists,
    they were not in the previous beam) while a descendant of theirs was live."""
    tot = [c.total() for c in ranked[:k + 1]]
    stats["kept_neg_inf"] = stats.get("kept_neg_inf", 0) + sum(1 for x in tot[:k] if x == float("-inf"))
    for a, b in zip(tot, tot[1:]):
        if b > float("-inf"):
            stats["min_gap"] = min(stats.get("min_gap", np.inf), (a - b) / max(1.0, abs(a), abs(b)))
    live = {h.node for h in prev}
    for c in ranked[:k]:
        if c.node is None or c.node in live:
            continue
        for h in prev:
            n = node_parent[h.node] if h.node > 0 else -1
            while n > 0 and n != c.node:
                n = node_parent[n]
            if n > 0:
                stats["reentries"] = stats.get("reentries", 0) + 1
                break


class RefGraph(ref_cg.ContextGraph):
    def __init__(self, phrases, context_score):
        self.context_score = context_score
        self.context_list = phrases
        self.num_nodes = 0
        self.root = ref_cg.ContextState(id=0, token=-1, token_score=0, node_score=0, output_score=0, is_end=False)
        self.root.fail = self.root
        self.build_graph(phrases)

    def states(self):
        out, stack = {0: self.root}, [self.root]
        while stack:
            for n in stack.pop().next.values():
                out[n.id] = n
                stack.append(n)
        return [out[i] for i in range(len(out))]


def run_ref(logp: torch.Tensor, k: int, phrases, cscore):
    cg = RefGraph(phrases, cscore) if phrases is not None else None
    r = ref_search.ctc_prefix_beam_search(logp[None], torch.tensor([logp.shape[0]]), k, cg, 0)[0]
    return r.nbest, r.nbest_scores, r.nbest_times


def make_case(logits: torch.Tensor, k: int, phrases=None, cscore=0.0):
    """Returns the case dict, or None when a generator condition fails (advance the seed)."""
    logp = torch.log_softmax(logits, dim=-1)
    T, V = logp.shape
    if T:
        vals1, ids1 = logp.topk(min(k + 1, V), dim=-1)
        if bool((vals1[:, :-1] == vals1[:, 1:]).any()):
            return None
        vals, ids = logp.topk(k, dim=-1)
    else:
        vals, ids = torch.zeros(0, k), torch.zeros(0, k, dtype=torch.int64)
    nbest, scores, times = run_ref(logp, k, phrases, cscore)
    stats: dict = {}
    cg = host.ContextGraph(phrases, cscore) if phrases is not None else None
    h_nbest, h_scores, h_times = host._search_one(vals.tolist(), ids.tolist(), k, 0, cg,
                                                  lambda *frame: _record(stats, *frame))
    assert h_nbest == nbest and h_times == times, "host restatement differs from the reference"
    assert all(abs(a - b) <= score_tol(k, T, b) for a, b in zip(h_scores, scores))
    if stats.get("kept_neg_inf", 0):
        return None
    if stats.get("min_gap", np.inf) < 100 * score_tol(k, T, 0.0):   # min_gap is relative to max(1, |score|)
        return None
    return {"k": k, "vals": vals.numpy().astype(np.float32), "ids": ids.numpy().astype(np.int32), "nbest": nbest,
            "scores": scores, "times": times, "phrases": phrases, "context_score": cscore,
            "reentries": stats.get("reentries", 0), "min_gap": stats.get("min_gap", None)}


def random_logits(V, T, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, V, generator=g) * sigma
    x[:, 0] += 1.5 * sigma
    return x


def peaked(V, L, seed):
    """CTC-like logits of a target with immediate repeats and 1-3 frame durations; every third
    token or so gets a close competitor so that a context bonus can change the 1-best."""
    rng = np.random.default_rng(seed)
    target = []
    while len(target) < L:
        tok = int(rng.integers(1, V))
        target.append(tok)
        if rng.random() < 0.25:
            target.append(tok)                      # "a a": needs a blank between
    frames, owner = [], []
    for i, tok in enumerate(target):
        nb = int(rng.integers(0, 3))
        if i > 0 and target[i - 1] == tok:
            nb = max(nb, 1)
        frames += [0] * nb + [tok] * int(rng.integers(1, 4))
        owner += [-1] * nb + [i] * (len(frames) - len(owner) - nb)
    frames += [0] * int(rng.integers(0, 3))
    owner += [-1] * (len(frames) - len(owner))
    T = len(frames)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(T, V, generator=g)
    rivals = {i: int(rng.integers(1, V)) for i in range(len(target)) if rng.random() < 0.35}
    for t, tok in enumerate(frames):
        x[t, tok] += 6.0
        i = owner[t]
        if i in rivals and rivals[i] != tok:
            x[t, rivals[i]] += 6.0 + float(rng.uniform(-0.5, 1.0))
    return x, target


def phrases_for(target, V):
    """Nested (x y, x y z), overlapping (x y z, y z w), a single token, and a phrase whose proper
    prefix ends the target (finalize removes the partial match)."""
    n = len(target)
    a, b = n // 5, n // 2
    extra = 1 + (target[-1] % (V - 1))
    return [target[a:a + 2], target[a:a + 3], target[b:b + 3], target[b + 1:b + 4], [target[n // 3]],
            target[-2:] + [extra]]


def graph_records(phrases, cscore, V, seed):
    g = RefGraph(phrases, cscore)
    states = g.states()
    rng = np.random.default_rng(seed)
    toks = sorted({t for p in phrases for t in p} | {int(t) for t in rng.integers(0, V, 6)})
    rec = []
    for s in states:
        for t in toks:
            sc, nx = g.forward_one_step(s, t)
            rec.append([s.id, t, float(sc), nx.id])
    fin = [float(g.finalize(s)[0]) for s in states]
    return rec, fin


def first_ok(build, seed, tries=400):
    for s in range(seed, seed + tries):
        c = build(s)
        if c is not None:
            c["seed"] = s
            return c
    raise RuntimeError("no seed satisfies the generator's conditions")


def main():
    cases = {}
    for V, T, k, sigma in ((40, 60, 4, 2.0), (200, 400, 10, 2.0), (5000, 300, 10, 1.5), (5000, 120, 16, 1.5)):
        cases[f"random_V{V}_T{T}_k{k}"] = first_ok(lambda s: make_case(random_logits(V, T, sigma, s), k), 100)
    changed = 0
    for (V, L, k), cs in zip(((64, 38, 5), (512, 110, 10), (64, 38, 8)), (2.0, 3.0, 6.0)):
        def both(s):
            x, target = peaked(V, L, s)
            plain = make_case(x, k)
            ph = phrases_for(target, V)
            ctx = make_case(x, k, ph, cs)
            if plain is None or ctx is None:
                return None
            rec, fin = graph_records(ph, cs, V, s)
            ctx["graph_steps"], ctx["graph_final"] = rec, fin
            return {"plain": plain, "ctx": ctx}
        c = first_ok(both, 300)
        T = c["plain"]["vals"].shape[0]
        c["plain"]["seed"] = c["ctx"]["seed"] = c["seed"]
        cases[f"peaked_V{V}_T{T}_k{k}"] = c["plain"]
        cases[f"context_V{V}_T{T}_k{k}"] = c["ctx"]
        changed += c["plain"]["nbest"][0] != c["ctx"]["nbest"][0]
    assert changed >= 1, "no context case changes the 1-best"
    # churn: tiny vocabularies, flat logits (the re-creation trap)
    rng = np.random.default_rng(5)
    seed, re_total = 1000, 0
    for i in range(200):
        V = int(rng.integers(4, 8))
        k = int(rng.integers(2, min(4, V) + 1))
        c = first_ok(lambda s: make_case(torch.randn(24, V, generator=torch.Generator().manual_seed(s)), k), seed)
        seed = c["seed"] + 1
        re_total += c["reentries"]
        cases[f"churn_{i:03d}"] = c
    assert re_total >= 10, f"only {re_total} re-entries in the churn set"
    # edges
    for T in (0, 1, 2):
        cases[f"edge_T{T}"] = first_ok(lambda s: make_case(random_logits(12, T, 2.0, s), 3), 2000)
    cases["edge_k1"] = first_ok(lambda s: make_case(random_logits(12, 30, 2.0, s), 1), 2100)
    cases["edge_kV"] = first_ok(lambda s: make_case(random_logits(6, 30, 1.0, s), 6), 2200)
    for i, T in enumerate((17, 0, 1, 40, 5, 23, 2, 31, 9)):
        cases[f"packed_{i}"] = first_ok(lambda s: make_case(random_logits(30, T, 2.0, s), 4), 2300 + 10 * i)

    arrays, meta = {}, {}
    for name, c in cases.items():
        arrays[name + "/vals"] = c["vals"]
        arrays[name + "/ids"] = c["ids"]
        arrays[name + "/scores"] = np.array(c["scores"], np.float64)
        arrays[name + "/lens"] = np.array([len(x) for x in c["nbest"]], np.int32)
        arrays[name + "/tokens"] = np.array([t for x in c["nbest"] for t in x], np.int32)
        arrays[name + "/times"] = np.array([t for x in c["times"] for t in x], np.int32)
        assert [len(x) for x in c["times"]] == [len(x) for x in c["nbest"]]
        meta[name] = {"k": c["k"], "seed": c["seed"], "phrases": c["phrases"], "context_score": c["context_score"],
                      "reentries": c["reentries"]}
        if "graph_steps" in c:
            arrays[name + "/graph_steps"] = np.array(c["graph_steps"], np.float64)
            arrays[name + "/graph_final"] = np.array(c["graph_final"], np.float64)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes;", len(cases), "cases; churn re-entries", re_total,
          "; 1-best changed by context in", changed, "cases")


if __name__ == "__main__":
    main()
