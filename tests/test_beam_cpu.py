"""CTC prefix beam search on the host (chunkformer_amd/search.py) against tests/golden/beam.npz, which
the reference's own ctc_prefix_beam_search produced (tests/golden/gen_golden_beam.py): the plain-Python
restatement, the ContextGraph tables, argument errors and the exported symbols.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from beam_fixture import check_result, load_cases


@pytest.fixture(scope="module")
def search():
    from chunkformer_amd import build
    build.build()
    from chunkformer_amd import search
    return search


def _graph(search, case):
    return None if case["phrases"] is None else search.ContextGraph(case["phrases"], case["context_score"])


def test_host_fallback_matches_reference_on_every_case(search):
    cases = load_cases()
    assert len(cases) >= 220
    for name, c in cases.items():
        T, k = c["vals"].shape
        r = search.beam_search_topk_host(c["vals"], c["ids"], [0], [T], k, _graph(search, c))[0]
        check_result(name, c, r)


def test_host_packed_batch_equals_per_utterance(search):
    cases = load_cases()
    packed = [cases[f"packed_{i}"] for i in range(9)]
    k = packed[0]["k"]
    starts, rows = [], 3
    for c in packed:
        starts.append(rows)
        rows += c["vals"].shape[0] + 5
    vals = torch.full((rows, k), float("nan"))
    ids = torch.full((rows, k), -7, dtype=torch.int32)
    for s0, c in zip(starts, packed):
        T = c["vals"].shape[0]
        vals[s0:s0 + T] = torch.from_numpy(c["vals"])
        ids[s0:s0 + T] = torch.from_numpy(c["ids"])
    res = search.beam_search_topk_host(vals, ids, starts, [c["vals"].shape[0] for c in packed], k)
    for i, (c, r) in enumerate(zip(packed, res)):
        check_result(f"packed_{i}", c, r)
    empty = res[1]
    assert empty.nbest == [[]] and empty.nbest_scores == [0.0] and empty.nbest_times == [[]]


def test_reference_signature_on_cpu_tensors(search):
    """ctc_prefix_beam_search(ctc_probs [B, T, V], ctc_lens, beam_size): the stable host top-k feeds the
    same search; exact ties take the lower index."""
    g = torch.Generator().manual_seed(3)
    logp = torch.log_softmax(torch.randn(2, 30, 9, generator=g) * 2, -1)
    res = search.ctc_prefix_beam_search(logp, torch.tensor([30, 11]), 4)
    for b, n in enumerate((30, 11)):
        v, i = search.topk_host(logp[b, :n], 4)
        one = search.beam_search_topk_host(v, i, [0], [n], 4)[0]
        assert res[b].nbest == one.nbest and res[b].nbest_scores == one.nbest_scores
        assert len(res[b].nbest) == 4 and res[b].times is not None
    tie = torch.tensor([[0.5, 1.0, 1.0, -2.0, 1.0]])
    v, i = search.topk_host(tie, 4)
    assert i.tolist() == [[1, 2, 4, 0]] and v.tolist() == [[1.0, 1.0, 1.0, 0.5]]


def test_context_graph_tables_match_reference(search):
    cases = load_cases()
    ctx = {n: c for n, c in cases.items() if c["phrases"] is not None}
    assert len(ctx) == 3 and sorted(c["context_score"] for c in ctx.values()) == [2.0, 3.0, 6.0]
    for name, c in ctx.items():
        cg = search.ContextGraph(c["phrases"], c["context_score"])
        assert len(c["graph_final"]) == cg.num_nodes + 1
        for state, tok, score, nxt in c["graph_steps"].tolist():
            got = cg.forward_one_step(int(state), int(tok))
            assert got == (score, int(nxt)), (name, state, tok)
        for state, score in enumerate(c["graph_final"].tolist()):
            assert cg.finalize(state) == (score, 0)
        t = cg.device_tables()
        n = cg.num_nodes + 1
        assert all(t[key].numel() == n for key in ("fail", "token_score", "node_score", "output_score"))
        tr = list(zip(t["trans_node"].tolist(), t["trans_token"].tolist(), t["trans_next"].tolist()))
        assert tr == sorted(tr) and len(tr) == cg.num_nodes
        assert all(cg.next[a][tok] == b for a, tok, b in tr)


def test_context_changes_the_best_hypothesis(search):
    cases = load_cases()
    changed = 0
    for name, c in cases.items():
        if name.startswith("context_"):
            changed += cases["peaked_" + name[len("context_"):]]["nbest"][0] != c["nbest"][0]
    assert changed >= 1


def test_context_graph_from_file(search, tmp_path):
    table = {"a": 1, "b": 2, "▁": 3, "<unk>": 4}
    p = tmp_path / "phrases.txt"
    p.write_text("ab\na b\nazb\n", encoding="utf-8")
    cg = search.ContextGraph.from_file(str(p), table, context_score=2.0)
    assert cg.context_list == [[1, 2], [1, 3, 2], [1, 4, 2]]
    no_unk = search.ContextGraph.from_file(str(p), {"a": 1, "b": 2})
    assert no_unk.context_list == [[1, 2], [1, 2], [1, 2]]


def test_context_graph_from_file_with_bpe_model(search, tmp_path, monkeypatch):
    """With a bpe_model (text/tokenize_utils.py:26-63): CJK ideographs are tokens of their own, the runs
    between them go through the sentencepiece model.  A stand-in module records what it is asked."""
    import types
    seen = []

    class Processor:
        def load(self, path):
            seen.append(("load", path))

        def encode_as_pieces(self, text):
            seen.append(("encode", text))
            return ["▁" + w for w in text.split()]

    fake = types.ModuleType("sentencepiece")
    fake.SentencePieceProcessor = Processor
    monkeypatch.setitem(sys.modules, "sentencepiece", fake)
    table = {"▁hello": 5, "▁world": 6, "你": 7, "好": 8, "<unk>": 9}
    p = tmp_path / "phrases.txt"
    p.write_text("hello world\n你好 hello 的\n", encoding="utf-8")
    cg = search.ContextGraph.from_file(str(p), table, bpe_model="bpe.model", context_score=2.0)
    assert cg.context_list == [[5, 6], [7, 8, 5, 9]]
    assert seen == [("load", "bpe.model"), ("encode", "hello world"), ("encode", " hello ")]


def test_non_finite_scores_raise(search):
    """A NaN or +inf log-prob makes a total NaN, which has no rank: the host raises (the kernel ranks it
    as -inf, so that its ranks stay distinct, and sets the error word the Python side raises on)."""
    vals = torch.log_softmax(torch.randn(6, 3, generator=torch.Generator().manual_seed(1)), -1)
    ids = torch.tensor([[0, 1, 2]] * 6, dtype=torch.int32)
    for bad in (float("nan"), float("inf")):
        v = vals.clone()
        v[3, 1] = bad
        with pytest.raises(RuntimeError, match="NaN"):
            search.beam_search_topk_host(v, ids, [0], [6], 3)
    v = vals.clone()
    v[3, 1] = float("-inf")      # -inf is an ordinary log-prob
    assert len(search.beam_search_topk_host(v, ids, [0], [6], 3)[0].nbest) == 3


def test_argument_errors(search, tmp_path, monkeypatch):
    logp = torch.zeros(1, 4, 5)
    with pytest.raises(ValueError):
        search.ctc_prefix_beam_search(logp, [4], 6)          # k > V
    with pytest.raises(ValueError):
        search.ctc_prefix_beam_search(torch.zeros(1, 4, 40), [4], 17)   # k > 16
    with pytest.raises(ValueError):
        search.ctc_prefix_beam_search(logp, [4], 0)
    with pytest.raises(ValueError):
        search.ctc_prefix_beam_search(logp, [5], 2)          # a length beyond T
    with pytest.raises(ValueError):
        search.beam_search_topk_host(torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.int32), [2], [3], 2)
    p = tmp_path / "phrases.txt"
    p.write_text("ab\n", encoding="utf-8")
    monkeypatch.setitem(sys.modules, "sentencepiece", None)   # import sentencepiece -> ImportError
    with pytest.raises(ImportError):
        search.ContextGraph.from_file(str(p), {"a": 1, "b": 2}, bpe_model=str(tmp_path / "bpe.model"))


def test_new_symbols_are_exported(search):
    from chunkformer_amd import _lib
    for name in ("cfm_ctc_topk_workspace_bytes", "cfm_ctc_topk", "cfm_ctc_topk_logp", "cfm_ctx_create",
                 "cfm_ctx_destroy", "cfm_ctc_beam_workspace_bytes", "cfm_ctc_beam_search"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
    for name in ("DecodeResult", "ContextGraph", "ctc_prefix_beam_search"):
        assert hasattr(search, name)
    r = search.DecodeResult([1, 2], score=-1.0)
    assert (r.tokens, r.score, r.confidence, r.tokens_confidence, r.times, r.nbest, r.nbest_scores, r.nbest_times) \
        == ([1, 2], -1.0, 0.0, None, None, None, None, None)
    # the beam workspace is sized from k * rows, and an undersized one is refused on the host
    need = _lib.cfm_ctc_beam_workspace_bytes(100, 2, 4, 1, 0)
    assert need >= 4 * (6 * 4 * 100) and _lib.cfm_ctc_beam_workspace_bytes(100, 2, 4, 0, 0) < need


def test_fixture_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "beam.npz")) < 1 << 20
    assert np.load(os.path.join(golden_dir, "beam.npz"))["meta"].dtype == np.uint8
