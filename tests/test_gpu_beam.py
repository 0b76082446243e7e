"""CTC prefix beam search on the device (csrc/ctc_beam.hip) against tests/golden/beam.npz (the
reference's own ctc_prefix_beam_search, tests/golden/gen_golden_beam.py) and against the host fallback.

Top-k: indices and values bit for bit the stable (-value, index) top-k of ctc_log_softmax on the same
rows.  Beam kernel: tokens, times, lengths and counts equal, scores within the derived tolerance
(beam_fixture.score_tol), two runs bit-identical.  Model level: batch_decode / endless_decode in beam
mode equal the host fallback run on the device's own log-probs; the defaults return what they did.
The peaked CTC head of the model-level tests is the one fixture that records it (small256.npz, config
SMALL256)."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from beam_fixture import check_result, load_cases, score_tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def search():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import search
    return search


def _graph(search, case):
    return None if case["phrases"] is None else search.ContextGraph(case["phrases"], case["context_score"])


# ------------------------------------------------------------------------------------ top-k
def _topk_model(which, dtype):
    from chunkformer_amd.config import LARGE, SMALL
    from chunkformer_amd.encoder import ChunkFormerEncoder
    from chunkformer_amd.weights import synthetic_state_dict
    cfg = SMALL if which == "small" else dataclasses.replace(LARGE, num_blocks=1)
    return cfg, ChunkFormerEncoder(cfg, synthetic_state_dict(cfg, 5), dtype=dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("which", ["small", "d512_v5000"])
def test_topk_equals_stable_topk_of_log_softmax(search, which, dtype):
    cfg, enc = _topk_model(which, dtype)
    assert cfg.vocab == (48 if which == "small" else 5000)
    slab = enc.ctc_topk_slab_rows()
    assert 0 < slab <= 16384
    g = torch.Generator().manual_seed(11)
    for rows in (1, 63, 257, slab + 1):
        hs = (torch.randn(rows, cfg.d_model, generator=g) * 2).to(enc.device)
        logp, _ = enc.ctc_log_softmax(hs, want_logp=True, want_ids=False)
        order = torch.sort(logp, dim=-1, descending=True, stable=True).indices
        for k in (1, 4, 10, 16):
            vals, ids = enc.ctc_topk(hs, k)
            assert torch.equal(ids.long(), order[:, :k]), (rows, k)
            assert torch.equal(vals, torch.gather(logp, 1, order[:, :k])), (rows, k)
            if rows in (257, slab + 1) and k == 10:
                v2, i2 = enc.ctc_topk(hs, k)
                assert torch.equal(v2, vals) and torch.equal(i2, ids)
                # the entry that takes log-probs directly selects the same
                v3, i3 = search.topk_logp_device(logp, k)
                assert torch.equal(v3, vals) and torch.equal(i3, ids)
        del logp, order
    with pytest.raises(ValueError):
        enc.ctc_topk(hs[:4], 17)
    if cfg.vocab < 64:
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=enc.device)
        from chunkformer_amd import _lib
        out_v = torch.empty(4, 16, device=enc.device)
        out_i = torch.empty(4, 16, dtype=torch.int32, device=enc.device)
        for bad_k in (0, 17):
            st = _lib.cfm_ctc_topk(enc._h, hs.data_ptr(), 4, bad_k, out_v.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                                   ws.numel(), 0)
            assert st == _lib.CFM_ERR_VALUE


def test_topk_logp_ties_take_the_lower_index(search):
    x = torch.tensor([[0.5, 1.0, 1.0, -2.0, 1.0], [3.0, 3.0, 3.0, 3.0, 3.0]], device="cuda")
    v, i = search.topk_logp_device(x, 4)
    assert i.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]] and v.tolist() == [[1.0, 1.0, 1.0, 0.5], [3.0] * 4]
    wide = torch.randn(5, 6001, generator=torch.Generator().manual_seed(2)).cuda()   # the re-read path (V > 5120)
    v, i = search.topk_logp_device(wide, 16)
    hv, hi = search.topk_host(wide.cpu(), 16)
    assert torch.equal(v.cpu(), hv) and torch.equal(i.cpu(), hi)
    with pytest.raises(ValueError):
        search.topk_logp_device(x, 6)


@pytest.mark.parametrize("V", [64, 65, 200, 256, 257, 700, 1024, 1025, 5120, 5121])
def test_topk_logp_every_vocabulary_path(search, V):
    """Every dispatch branch of the top-k kernel (1, 4, 16 and 80 registers per lane, and the re-read
    path) at its edges, over more than one block of rows, with exact ties in every row."""
    x = torch.randn(37, V, generator=torch.Generator().manual_seed(V))
    x[:, V // 2] = x[:, 3]                      # a tie across lanes
    x[5] = torch.round(x[5] * 2) / 2            # many ties: the candidate list overflows on wide rows
    x[6] = 0.25                                 # all equal
    for k in (1, 7, 16):
        v, i = search.topk_logp_device(x.cuda(), k)
        hv, hi = search.topk_host(x, k)
        assert torch.equal(i.cpu(), hi) and torch.equal(v.cpu(), hv), (V, k)


# ------------------------------------------------------------------------------------ beam kernel
def _pack(cases, k, gap=0, lead=0):
    starts, rows = [], lead
    for c in cases:
        starts.append(rows)
        rows += c["vals"].shape[0] + gap
    vals = torch.full((max(rows, 1), k), float("nan"))
    ids = torch.full((max(rows, 1), k), -7, dtype=torch.int32)
    for s0, c in zip(starts, cases):
        T = c["vals"].shape[0]
        vals[s0:s0 + T] = torch.from_numpy(c["vals"])
        ids[s0:s0 + T] = torch.from_numpy(c["ids"])
    return vals.cuda(), ids.cuda(), starts, [c["vals"].shape[0] for c in cases]


def _same(a, b):
    return all(x.nbest == y.nbest and x.nbest_times == y.nbest_times and x.nbest_scores == y.nbest_scores
               for x, y in zip(a, b)) and len(a) == len(b)


def test_beam_kernel_matches_reference_on_every_case(search):
    cases = load_cases()
    single = {n: c for n, c in cases.items() if not n.startswith(("churn_", "packed_"))}
    assert len(single) >= 15
    for name, c in single.items():
        vals, ids, starts, lens = _pack([c], c["k"])
        cg = _graph(search, c)
        r = search.beam_search_topk_device(vals, ids, starts, lens, c["k"], cg)
        check_result(name, c, r[0])
        assert _same(r, search.beam_search_topk_device(vals, ids, starts, lens, c["k"], cg)), name
        if name.startswith("random_V40"):
            no_t = search.beam_search_topk_device(vals, ids, starts, lens, c["k"], cg, with_times=False)[0]
            assert no_t.nbest == c["nbest"] and no_t.nbest_times is None and no_t.nbest_scores == r[0].nbest_scores


def test_beam_kernel_churn_cases_packed(search):
    """The 200 re-creation cases, one call per beam size: a prefix that leaves the beam while a
    descendant stays alive must come back as the same node."""
    cases = load_cases()
    churn = [(n, c) for n, c in cases.items() if n.startswith("churn_")]
    assert len(churn) == 200 and sum(c["reentries"] for _, c in churn) >= 10
    for k in sorted({c["k"] for _, c in churn}):
        grp = [(n, c) for n, c in churn if c["k"] == k]
        vals, ids, starts, lens = _pack([c for _, c in grp], k)
        res = search.beam_search_topk_device(vals, ids, starts, lens, k)
        for (name, c), r in zip(grp, res):
            check_result(name, c, r)
        assert _same(res, search.beam_search_topk_device(vals, ids, starts, lens, k))


def test_beam_kernel_packed_batch_with_gaps(search):
    cases = load_cases()
    packed = [cases[f"packed_{i}"] for i in range(9)]
    k = packed[0]["k"]
    vals, ids, starts, lens = _pack(packed, k, gap=5, lead=3)
    assert 0 in lens and 1 in lens
    res = search.beam_search_topk_device(vals, ids, starts, lens, k)
    for i, (c, r) in enumerate(zip(packed, res)):
        check_result(f"packed_{i}", c, r)
    # regions in another order give the same per-utterance results
    perm = [4, 0, 8, 2, 6, 1, 3, 7, 5]
    res_p = search.beam_search_topk_device(vals, ids, [starts[i] for i in perm], [lens[i] for i in perm], k)
    assert _same(res_p, [res[i] for i in perm])


def test_beam_undersized_workspace_is_refused_before_launch(search):
    from chunkformer_amd import _lib
    c = load_cases()["random_V40_T60_k4"]
    vals, ids, starts, lens = _pack([c], 4)
    need = int(_lib.cfm_ctc_beam_workspace_bytes(vals.shape[0], 1, 4, 1, 0))
    with pytest.raises(ValueError, match="workspace too small"):
        search.beam_search_topk_device(vals, ids, starts, lens, 4, workspace_bytes=need - 1)
    with pytest.raises(ValueError):
        search.beam_search_topk_device(vals, ids, [10], [60], 4)      # rows beyond the arrays
    check_result("random_V40_T60_k4", c, search.beam_search_topk_device(vals, ids, starts, lens, 4)[0])


# ------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def small_model(search, golden_dir):
    from chunkformer_amd.config import SMALL256
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.weights import synthetic_state_dict
    from conftest import with_fixture_ctc_head
    g = np.load(os.path.join(golden_dir, "small256.npz"))
    sd = with_fixture_ctc_head(synthetic_state_dict(SMALL256, int(g["seed"])), g)
    return ChunkFormerModel(SMALL256, sd, dtype="fp32")


def _host_expected(search, m, eo_rows, starts, lens, k, cg):
    logp, _ = m.encoder.ctc_log_softmax(eo_rows, want_logp=True, want_ids=False)
    v, i = search.topk_host(logp.cpu(), k)
    return search.beam_search_topk_host(v, i, starts, lens, k, cg)


def _check_equal(res, exp, k, lens):
    assert len(res) == len(exp) == len(lens)
    for r, e, T in zip(res, exp, lens):
        assert r.nbest == e.nbest and r.nbest_times == e.nbest_times
        assert len(r.nbest_scores) == len(e.nbest_scores)
        for a, b in zip(r.nbest_scores, e.nbest_scores):
            assert abs(a - b) <= score_tol(k, T, b)


def test_batch_decode_beam_equals_host_fallback(search, small_model):
    from chunkformer_amd.weights import synthetic_features
    m, k, C, L, R = small_model, 5, 16, 32, 16
    xs = synthetic_features([611, 97, 350, 1203], 31)
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int)
    eo, el, n_chunks, _, _, _ = m.encoder.forward_parallel_chunk(xs, lens, C, L, R, offset=torch.zeros(4, dtype=torch.int))
    starts = (np.cumsum([0] + list(n_chunks[:-1])) * C).tolist()
    rl = [int(n) for n in el.tolist()]
    rows = eo.reshape(-1, eo.shape[-1]).clone()
    greedy = m.batch_decode(xs, C, L, R)
    phrases = [h.tolist() for h in greedy]
    phrases = [[int(t) for t in dict.fromkeys(p) if t != 0][:3] for p in phrases if len(p)]
    for cg in (None, search.ContextGraph([p for p in phrases if p], 3.0)):
        res = m.batch_decode(xs, C, L, R, decoding_method="ctc_prefix_beam_search", beam_size=k, context_graph=cg)
        exp = _host_expected(search, m, rows, starts, rl, k, cg)
        assert any(len(e.nbest[0]) > 0 for e in exp)
        _check_equal(res, exp, k, rl)
    # the default is the greedy path, unchanged
    again = m.batch_decode(xs, C, L, R, decoding_method="ctc_greedy_search")
    assert all(torch.equal(a, b) for a, b in zip(greedy, again))
    with pytest.raises(ValueError):
        m.batch_decode(xs, C, L, R, decoding_method="attention")


def test_endless_decode_beam_equals_host_fallback(search, small_model):
    from chunkformer_amd.model import endless_segments
    from chunkformer_amd.weights import synthetic_features
    m, k, C, L, R, tbd = small_model, 6, 16, 32, 16, 20
    T = 3000
    assert len(endless_segments(T, C, L, R, tbd, m.config.num_blocks, m.config.kernel_size)[1]) == 3
    x = synthetic_features([T], 47)[0]
    ids0 = m.endless_decode(x, C, L, R, total_batch_duration=tbd)
    best, eo = m.endless_decode(x, C, L, R, total_batch_duration=tbd, return_encoder_out=True,
                                decoding_method="ctc_prefix_beam_search", beam_size=k)
    n = eo.shape[1]
    assert n == ids0.shape[1]
    exp = _host_expected(search, m, eo[0], [0], [n], k, None)
    _check_equal([best], exp, k, [n])
    assert torch.equal(m.endless_decode(x, C, L, R, total_batch_duration=tbd), ids0)   # the default, unchanged


def test_beam_text_outputs_and_defaults_match_text_json(search, golden_dir):
    """With a char_dict: the default calls return exactly the reference's strings (text.json), the
    beam calls return text / n-best texts / timestamp items of the same format."""
    from chunkformer_amd.config import LARGE_4H
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict, synthetic_vocab
    g = np.load(os.path.join(golden_dir, "large_4h.npz"))
    with open(os.path.join(golden_dir, "text.json"), encoding="utf8") as f:
        text = json.load(f)
    m = ChunkFormerModel(LARGE_4H, synthetic_state_dict(LARGE_4H, int(g["seed"])), dtype="fp32",
                         char_dict=synthetic_vocab(LARGE_4H.vocab))
    xs = synthetic_features(g["lens"].tolist(), int(g["feat_seed"]))
    assert m.batch_decode(xs, 64, 128, 128) == text["large_4h_decode"]
    beam = m.batch_decode(xs, 64, 128, 128, decoding_method="ctc_prefix_beam_search", beam_size=4)
    nbest = m.batch_decode(xs, 64, 128, 128, decoding_method="ctc_prefix_beam_search", beam_size=4, return_nbest=True)
    assert len(beam) == len(xs) and all(isinstance(t, str) for t in beam)
    assert [n[0] for n in nbest] == beam and all(1 <= len(n) <= 4 for n in nbest)
    plain = m.endless_decode(xs[0], 64, 128, 128, total_batch_duration=1800, return_timestamps=True)
    assert "".join(it["decode"] for it in plain).replace(" ", "") == text["large_4h_decode"][0].replace(" ", "")
    items = m.endless_decode(xs[0], 64, 128, 128, decoding_method="ctc_prefix_beam_search", beam_size=4)
    assert isinstance(items, list) and all(set(it) == {"decode", "start", "end"} for it in items)
    assert "".join(it["decode"] for it in items).replace(" ", "") == \
        m.endless_decode(xs[0], 64, 128, 128, decoding_method="ctc_prefix_beam_search", beam_size=4,
                         return_timestamps=False).replace(" ", "")


def test_beam_rejected_on_transducer_checkpoints(search, golden_dir):
    from chunkformer_amd.config import LARGE
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.transducer import RNNTConfig, synthetic_transducer_state_dict
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    g = np.load(os.path.join(golden_dir, "rnnt.npz"))
    c = RNNTConfig(vocab=int(g["vocab"]))
    cfg = dataclasses.replace(LARGE, num_blocks=1)
    sd = synthetic_state_dict(cfg, 1)
    sd.update(synthetic_transducer_state_dict(c, int(g["seed"])))
    m = ChunkFormerModel(cfg, sd, dtype="fp32", model_type="transducer", rnnt_config=c)
    x = synthetic_features([200], 3)
    with pytest.raises(ValueError, match="transducer"):
        m.batch_decode(x, 16, 32, 16, decoding_method="ctc_prefix_beam_search")
    with pytest.raises(ValueError, match="transducer"):
        m.endless_decode(x[0], 16, 32, 16, decoding_method="ctc_prefix_beam_search")


def test_beam_rejected_on_classification_checkpoints(search):
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    cfg = dataclasses.replace(SMALL, vocab=0)
    sd = synthetic_state_dict(cfg, 1)
    g = torch.Generator().manual_seed(0)
    sd["classification_heads.gender.linear.weight"] = torch.randn(2, cfg.d_model, generator=g)
    sd["classification_heads.gender.linear.bias"] = torch.zeros(2)
    m = ChunkFormerModel(cfg, sd, dtype="fp32", model_type="classification", tasks={"gender": 2})
    x = synthetic_features([200], 3)
    with pytest.raises(ValueError, match="classification model"):
        m.batch_decode(x, 16, 32, 16, decoding_method="ctc_prefix_beam_search")
    with pytest.raises(ValueError, match="classification model"):
        m.endless_decode(x[0], 16, 32, 16, decoding_method="ctc_prefix_beam_search")
