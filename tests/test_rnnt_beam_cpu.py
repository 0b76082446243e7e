"""CPU: the transducer prefix beam search's restatement (chunkformer_amd/transducer_beam.py) against the reference's
recorded beams (tests/golden/rnnt_beam.npz), its single step on hand-made states, the greedy oracle, and the model's
dispatch and argument errors."""
import math
import os
import re

import numpy as np
import pytest
import torch

import rnnt_beam_fixture as fx
from chunkformer_amd import transducer_beam as TB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_size_and_conditions():
    assert os.path.getsize(fx.GOLDEN) < 1 << 20
    _, meta = fx.archive()
    cases = meta["cases"]
    assert {c["rows"] for c in cases} == {0, 1, 2, 9, 17, 33, 65, 130}
    assert {c["beam"] for c in cases} == {1, 2, 5, 10, 16}
    assert {(c["cw"], c["tw"]) for c in cases} == {(0.3, 0.7), (0.0, 1.0), (1.0, 0.0)}
    assert any(c["beam"] == meta["models"][c["model"]]["config"]["vocab"] - 1 for c in cases)
    assert {(m["config"]["vocab"], m["config"]["hidden"], m["config"]["num_layers"]) for m in meta["models"].values()} >= \
        {(37, 32, 1), (130, 64, 2), (1024, 64, 2)}
    for c in cases:
        if c["equality"]:
            assert c["margin"] >= 2 * (c["rows"] + 1) * meta["dev"]
    assert {(c["rows"], c["beam"]) for c in cases if not c["equality"]} >= {(65, 10), (33, 16), (130, 5)}
    for name in meta["models"]:
        for recipe in ("dense", "blank"):
            eq = [fx.case(i) for i, c in enumerate(cases) if c["equality"] and (c["model"], c["recipe"]) == (name, recipe)]
            assert sum(1 for c in eq if c["fusions"] > 0) >= 3, (name, recipe)
            assert len({len(c["tokens"][0]) for c in eq}) >= 3, (name, recipe)
            bias, V = meta["models"][name]["recipes"][recipe], meta["models"][name]["config"]["vocab"]
            if bias >= math.log(V - 1):   # below that the tokens outweigh the blank at every frame (the generator's note)
                assert sum(1 for c in eq if c["rows"] and len(c["tokens"][0]) < c["rows"] / 2) >= 3, (name, recipe)


def test_restatement_reproduces_every_recorded_beam():
    for i in range(len(fx.cases())):
        c = fx.case(i)
        r = TB.prefix_beam_search_host(fx.host_model(c["model"], c["recipe"]), c["enc"], c["ctc"], [0], [c["rows"]],
                                       c["beam"], c["cw"], c["tw"])[0]
        what = (c["model"], c["recipe"], c["rows"], c["beam"], c["cw"], c["tw"])
        assert r.nbest == c["tokens"], what
        np.testing.assert_allclose(r.nbest_scores, c["scores"], rtol=0, atol=1e-4, err_msg=str(what))
        np.testing.assert_array_equal(r.trace["parent"], c["trace"]["parent"])
        np.testing.assert_array_equal(r.trace["token"], c["trace"]["token"])
        np.testing.assert_allclose(r.trace["score"], c["trace"]["score"], rtol=0, atol=1e-4)
        assert r.tokens == r.nbest[0] and len(r.times) == len(r.tokens) and r.times == sorted(set(r.times))


def test_beam_step_host_on_hand_made_states():
    f32 = np.float32
    # exact ties keep creation order: (hypothesis ascending, rank ascending)
    kept, gap = TB.beam_step_host([(), (3,)], [-1.0, -1.0], [[-0.5, -0.5], [-0.5, -0.5]], [[1, 2], [0, 4]], 2)
    assert [k[0] for k in kept] == [(1,), (2,)] and gap == 0.0 and [k[2:] for k in kept] == [(0, 1, True), (0, 2, True)]
    # an extension folds into the unchanged prefix ranked below it: the extension's position and new state are kept
    kept, _ = TB.beam_step_host([(), (1,)], [-0.25, -0.5], [[-0.25, -0.5], [-0.25, -0.75]], [[1, 0], [0, 1]], 2)
    assert kept[0][0] == (1,) and kept[0][2:] == (0, 1, True)
    m = max(-0.5, -0.75)
    assert kept[0][1] == m + math.log(0 + math.exp(-0.5 - m) + math.exp(-0.75 - m))
    assert kept[1][0] == () and kept[1][1] == -0.75
    # ... and into one ranked above it: the unchanged hypothesis' position and old state are kept
    kept, _ = TB.beam_step_host([(1,), ()], [-0.25, -0.5], [[-0.25, -0.5], [-0.25, -0.75]], [[0, 1], [1, 0]], 2)
    assert kept[0][0] == (1,) and kept[0][2:] == (0, 0, False)
    assert kept[0][1] == -0.5 + math.log(0 + 1.0 + math.exp(-0.75 + 0.5))
    # n < K, and K = V: every id of the vocabulary in every row
    kept, gap = TB.beam_step_host([()], [0.0], [[-0.5, -1.0, -2.0]], [[2, 0, 1]], 3)
    assert [k[0] for k in kept] == [(2,), (), (1,)] and [k[1] for k in kept] == [-0.5, -1.0, -2.0] and gap == 0.5
    # the candidate score is f32(score) + logp in f32
    s = -100.123456789
    kept, _ = TB.beam_step_host([()], [s], [[-0.3]], [[0]], 1)
    assert kept[0][1] == float(f32(f32(s) + f32(-0.3))) and kept[0][1] != s + float(f32(-0.3))


def test_beam_one_without_ctc_is_the_oracle_greedy_search():
    from oracle import rnnt_ref
    n = 0
    for i, c in enumerate(fx.cases()):
        if c["beam"] != 1 or c["cw"] != 0.0 or c["rows"] < 9:
            continue
        c = fx.case(i)
        cfg, sd = fx.model(c["model"], c["recipe"])
        dense, _ = rnnt_ref.greedy_one(sd, cfg.num_layers, cfg.hidden, c["enc"], 1)
        dense = dense.numpy()[:, 0]
        assert c["tokens"][0] == dense[dense != 0].tolist()
        n += 1
    assert n >= 4


def _bare_model(model_type):
    from chunkformer_amd.model import ChunkFormerModel
    m = ChunkFormerModel.__new__(ChunkFormerModel)
    m.model_type = model_type
    m.is_classification = model_type == "classification"
    m.rescorer = None
    m.rnnt = None
    return m


def test_dispatch_and_argument_errors():
    import inspect

    from chunkformer_amd.model import ChunkFormerModel
    for mt in ("asr_model", "classification"):
        with pytest.raises(ValueError, match="transducer"):
            _bare_model(mt).batch_decode([], decoding_method="rnnt_beam_search")
        with pytest.raises(ValueError, match="transducer"):
            _bare_model(mt).endless_decode(torch.zeros(10, 80), decoding_method="rnnt_beam_search")
    t = _bare_model("transducer")
    with pytest.raises(ValueError, match="RNN-T greedy search"):      # the CTC methods stay rejected as they were
        t.batch_decode([], decoding_method="ctc_prefix_beam_search")
    with pytest.raises(ValueError, match="unknown decoding_method"):
        t.batch_decode([], decoding_method="rnnt_beam")
    with pytest.raises(ValueError, match="unknown decoding_method"):
        _bare_model("asr_model").batch_decode([], decoding_method="rnnt_beam")

    class FakeGreedy:
        cfg, device = None, None
    t.rnnt = FakeGreedy()
    s = t._rnnt_beam_search()
    assert isinstance(s, TB.RNNTBeamSearch) and t._rnnt_beam_search() is s and s.rnnt is t.rnnt
    assert t.batch_decode([], decoding_method="rnnt_beam_search") == []
    for fn in (ChunkFormerModel.batch_decode, ChunkFormerModel.endless_decode):
        p = inspect.signature(fn).parameters
        # the tail of the signature is pinned by test_attention_decode_cpu.py, so the new argument stands before it
        assert p["transducer_weight"].default is None and p["ctc_weight"].default is None
        assert list(p)[-5:] == ["transducer_weight", "ctc_weight", "reverse_weight", "length_penalty", "max_len"]

    cfg, sd = fx.model("v37", "dense")
    host = fx.host_model("v37", "dense")
    enc, ctc = torch.zeros(4, cfg.enc_dim), torch.zeros(4, cfg.vocab)
    for beam in (0, 17):
        with pytest.raises(ValueError, match="beam_size"):
            TB.prefix_beam_search_host(host, enc, ctc, [0], [4], beam)
    with pytest.raises(ValueError, match="beam_size"):
        TB._check_args(16, 15, 0.3, 0.7, True)
    with pytest.raises(ValueError, match="weight"):
        TB.prefix_beam_search_host(host, enc, ctc, [0], [4], 2, -1.0, 1.0)
    with pytest.raises(ValueError, match="weight"):
        TB.prefix_beam_search_host(host, enc, ctc, [0], [4], 2, 0.0, 0.0)
    with pytest.raises(ValueError, match="ctc_logp"):
        TB.prefix_beam_search_host(host, enc, None, [0], [4], 2, 0.3, 0.7)
    with pytest.raises(ValueError, match="row ranges"):
        TB.prefix_beam_search_host(host, enc, ctc, [1], [4], 2)
    assert TB.prefix_beam_search_host(host, enc, None, [0, 0], [0, 4], 2, 0.0, 1.0)[0].nbest == [[]]


def test_beam_symbols_are_exported():
    from chunkformer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cfm.h")).read()
    declared = set(re.findall(r"\b(cfm_rnnt_beam_[a-z_]+)\s*\(", hdr))
    assert declared == {"cfm_rnnt_beam_workspace_bytes", "cfm_rnnt_beam_search", "cfm_rnnt_beam_error"}
    for name in declared:
        assert hasattr(_lib.lib, name) and name in _lib.EXPORTED
    ops = open(os.path.join(ROOT, "include", "cfm_ops.h")).read()
    for name in re.findall(r"\b(cfm_op_rnnt_[a-z_]+)\s*\(", ops):
        assert hasattr(_lib.lib, name) and name in _lib.EXPORTED_OPS
