"""The `attention` decoding mode on the CPU: the host restatement (chunkformer_amd/attention_decode.py) against the
reference's recorded searches (tests/golden/attention.npz), the properties DESIGN §9e fixes, the model's method
dispatch and the C-ABI exports.

Bars: a trace score after i steps within i x 1e-4 and the chosen final score within (steps + 1) x 1e-4 of the fixture's
float64 values (1e-4 is the project's fp32 bar on one log-prob); tokens, trace parents and trace tokens equal -- the
generator admits only cases whose decision margin is at least twice that bar.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import attention_fixture as fx

from chunkformer_amd import attention_decode as A
from chunkformer_amd import rescore as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(m, c, dtype=torch.float32, **kw):
    args = dict(beam_size=c["beam"], length_penalty=c["lp"], max_len=c["max_len"])
    args.update(kw)
    return A.attention_beam_search_host(m["cfg"], m["sds"][c["recipe"]], c["enc"], [0], [c["enc"].shape[0]], dtype=dtype,
                                        **args)[0]


def _searcher(m, c, dtype=torch.float64):
    cfg = m["cfg"]
    W = {k: v.to(dtype) for k, v in R.native_names(cfg, m["sds"][c["recipe"]]).items()}
    return A.HostSearch(cfg, W, R.positional_table(cfg.d_model, R.MAX_POSITIONS, dtype), c["enc"].to(dtype), c["beam"], dtype)


def test_fixture_covers_what_it_promises():
    models = fx.load_models()
    assert set(models) == {"d128h2", "d256h2", "d64h4", "uni_d64h4"}
    assert os.path.getsize(os.path.join(fx.GOLDEN, "attention.npz")) < 1 << 20
    for name, m in models.items():
        cs = m["cases"]
        assert {c["beam"] for c in cs} == {1, 2, 3, 10, 16}
        assert {c["enc"].shape[0] for c in cs} == {0, 1, 15, 16, 17, 31, 32, 33, 65, 130}
        assert {c["lp"] for c in cs} == {0.0, 0.6}
        assert any(c["max_len"] is not None and c["max_len"] < c["enc"].shape[0] for c in cs)
        assert all(c["margin"] >= 2 * (c["steps"] + 1) * fx.FP32_BAR for c in cs)
        assert sum(c["early_eos"] for c in cs) >= 3 and sum(c["to_limit"] for c in cs) >= 3
        assert len({len(c["tokens"]) for c in cs}) >= 3 and max(c["steps"] for c in cs) > 64
        assert sum(c["margin"] > 2 * (c["steps"] + 1) * m["d_f16"] for c in cs) >= 3
    assert models["d64h4"]["cfg"].sos != models["d64h4"]["cfg"].eos
    assert not models["uni_d64h4"]["cfg"].bidirectional


@pytest.mark.parametrize("name, k", fx.case_ids())
def test_host_f32_reproduces_the_fixture(name, k):
    m = fx.load_models()[name]
    c = m["cases"][k]
    worst = fx.check_against_fixture(_host(m, c), c, fx.FP32_BAR)
    print(f"attention host f32 {name} case {k}: steps {c['steps']}, worst score error {worst:.3f} of its bar")


def test_steps_after_all_beams_finished_change_nothing():
    m = fx.load_models()["d128h2"]
    done = 0
    for c in m["cases"]:
        if c["recipe"] != "early" or c["beam"] > 3:
            continue
        hs = _searcher(m, c)
        for _ in range(200):
            if all(hs.fin):
                break
            hs.step()
        if not all(hs.fin):
            continue
        done += 1
        before = ([list(h) for h in hs.hyps], hs.scores.clone())
        n_eos = [sum(t == m["cfg"].eos for t in h[1:]) for h in hs.hyps]
        for _ in range(3):
            hs.step()
        strip = lambda h: [t for t in h[1:] if t != m["cfg"].eos]   # noqa: E731
        assert [strip(h) for h in hs.hyps] == [strip(h) for h in before[0]]          # same set, same order
        assert torch.equal(hs.scores, before[1])                                      # same scores
        assert hs.trace[-1][0] == list(range(c["beam"]))                              # every beam its own parent
        assert [sum(t == m["cfg"].eos for t in h[1:]) for h in hs.hyps] == [n + 3 for n in n_eos]
    assert done >= 1


def test_an_utterance_freezes_at_its_limit():
    m = fx.load_models()["d64h4"]
    c = next(c for c in m["cases"] if c["enc"].shape[0] == 33 and c["max_len"] is None and c["beam"] == 10)
    full = _host(m, c, torch.float64)
    for lim in (1, 5, 12):
        cut = _host(m, c, torch.float64, max_len=lim)
        assert cut.steps == min(lim, full.steps)
        assert cut.trace == full.trace[:lim]
    longer = _host(m, c, torch.float64, max_len=40)       # max_len replaces the row count, also upwards
    assert longer.trace[:full.steps] == full.trace and longer.steps >= full.steps


def test_result_does_not_depend_on_batch_composition():
    m = fx.load_models()["d128h2"]
    mid = [c for c in m["cases"] if c["recipe"] == "mid" and c["max_len"] is None]
    cs = [next(c for c in mid if c["enc"].shape[0] == n) for n in (0, 1, 15, 16, 33)]      # 5 utterances, 5 limits
    rows = [c["enc"].shape[0] for c in cs]
    starts = np.cumsum([0] + rows[:-1]).tolist()
    enc = torch.cat([c["enc"] for c in cs])
    sd = m["sds"]["mid"]
    together = A.attention_beam_search_host(m["cfg"], sd, enc, starts, rows, 3, 0.6)
    for c, t in zip(cs, together):
        alone = A.attention_beam_search_host(m["cfg"], sd, c["enc"], [0], [c["enc"].shape[0]], 3, 0.6)[0]
        assert alone.tokens == t.tokens and alone.trace == t.trace
        assert [repr(x) for x in alone.nbest_scores] == [repr(x) for x in t.nbest_scores]      # (NaN == NaN here)


def test_zero_rows_and_length_penalty_edges():
    models = fx.load_models()
    for name in ("d128h2", "d64h4"):
        m = models[name]
        cfg, sd = m["cfg"], m["sds"]["mid"]
        enc = torch.zeros(0, cfg.d_model)
        r = A.attention_beam_search_host(cfg, sd, enc, [0], [0], 3, 0.0)[0]
        assert r.tokens == [] and r.score == 0.0 and r.steps == 0 and r.nbest[0] == []
        r = A.attention_beam_search_host(cfg, sd, enc, [0], [0], 3, 0.6)[0]
        if cfg.sos == cfg.eos:      # no token counts: 0 / 0 ** 0.6 = NaN, which torch.max selects
            assert r.tokens == [] and math.isnan(r.score) and r.best_index == 0
        else:                       # the sos counts: 0 / 1
            assert r.tokens == [] and r.score == 0.0
    # penalty 0 leaves the scores as they are; a positive one divides by count ** penalty (IEEE, as torch)
    m = models["d128h2"]
    c = next(c for c in m["cases"] if c["steps"] == 15 and c["beam"] == 2)
    a, b = _host(m, c, length_penalty=0.0), _host(m, c, length_penalty=0.6)
    assert a.trace == b.trace
    eos = m["cfg"].eos
    for row, sa, sb in zip(a.beam_rows, a.beam_scores, b.beam_scores):
        cnt = sum(t != eos for t in row)
        if cnt:
            assert abs(sb - sa / cnt ** 0.6) <= 1e-5 * max(1.0, abs(sb))
        else:
            assert sb == -math.inf or math.isnan(sb)
    assert A._first_max([float("nan"), 1.0]) == 0 and A._first_max([1.0, float("nan"), 5.0]) == 1
    assert A._first_max([-1.0, -1.0]) == 0 and A._first_max([-math.inf, -2.0, -2.0]) == 1


def test_limits_and_arguments_raise():
    m = fx.load_models()["d64h4"]
    cfg, sd = m["cfg"], m["sds"]["mid"]
    assert A.step_limits([5000, 3], None) == [5000, 3] and A.step_limits([9000, 3], 40) == [40, 40]
    with pytest.raises(ValueError, match="max_len"):
        A.step_limits([5001], None)
    with pytest.raises(ValueError, match="max_len"):
        A.attention_beam_search_host(cfg, sd, torch.zeros(5001, cfg.d_model), [0], [5001], 2)
    with pytest.raises(ValueError, match="max_len"):
        A.step_limits([10], 5001)
    for beam in (0, 17, cfg.vocab + 1):
        with pytest.raises(ValueError, match="beam_size"):
            A.attention_beam_search_host(cfg, sd, torch.zeros(2, cfg.d_model), [0], [2], beam)
    with pytest.raises(ValueError, match="row ranges"):
        A.attention_beam_search_host(cfg, sd, torch.zeros(2, cfg.d_model), [0], [3], 2)


def test_sharpened_weights_change_only_the_left_output_layer():
    cfg = fx.load_models()["d128h2"]["cfg"]
    a, b = R.synthetic_decoder_state_dict(cfg, 4), A.sharpened_decoder_state_dict(cfg, 4, 6.0, -0.5)
    changed = {k for k in a if not torch.equal(a[k], b[k])}
    assert changed == {R.LEFT + "output_layer.weight", R.LEFT + "output_layer.bias"}
    assert torch.equal(b[R.LEFT + "output_layer.weight"], a[R.LEFT + "output_layer.weight"] * 6.0)


# ------------------------------------------------------------------------------------ model
def _bare_model(model_type, rescorer=None):
    from chunkformer_amd.model import ChunkFormerModel
    m = ChunkFormerModel.__new__(ChunkFormerModel)
    m.model_type = model_type
    m.is_classification = model_type == "classification"
    m.rescorer = rescorer
    return m


def test_attention_method_dispatch_on_a_bare_model():
    m = _bare_model("asr_model")
    with pytest.raises(ValueError, match="decoder"):
        m._attention_search()
    with pytest.raises(ValueError, match="decoder"):
        m.batch_decode([], decoding_method="attention")
    with pytest.raises(ValueError, match="decoder"):
        m.endless_decode(torch.zeros(10, 80), decoding_method="attention")
    t = _bare_model("transducer", rescorer=object())
    with pytest.raises(ValueError, match="transducer"):
        t.batch_decode([], decoding_method="attention")
    with pytest.raises(ValueError, match="classification"):
        _bare_model("classification").batch_decode([], decoding_method="attention")
    with pytest.raises(ValueError):                      # the CTC methods' gate is as it was
        _bare_model("asr_model", rescorer=object())._beam_method("attention")
    with pytest.raises(ValueError, match="unknown decoding_method"):
        m.batch_decode([], decoding_method="attention_beam")

    class FakeRescorer:
        cfg, device, dtype = None, None, None
    ok = _bare_model("asr_model", rescorer=FakeRescorer())
    dec = ok._attention_search()
    assert isinstance(dec, A.AttentionDecoder) and ok._attention_search() is dec and dec.rescorer is ok.rescorer


def test_signatures_append_the_new_arguments():
    import inspect

    from chunkformer_amd.model import ChunkFormerModel
    for fn in (ChunkFormerModel.batch_decode, ChunkFormerModel.endless_decode):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ["length_penalty", "max_len"] and names[-4:-2] == ["ctc_weight", "reverse_weight"]
        p = inspect.signature(fn).parameters
        assert p["length_penalty"].default == 0.0 and p["max_len"].default is None


# ------------------------------------------------------------------------------------ C-ABI
def test_attdec_symbols_are_exported():
    from chunkformer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cfm.h")).read()
    declared = set(re.findall(r"\b(cfm_attdec_[a-z_]+)\s*\(", hdr))
    assert declared == {"cfm_attdec_workspace_bytes", "cfm_attdec_begin", "cfm_attdec_steps", "cfm_attdec_finish"}
    for name in declared:
        assert hasattr(_lib.lib, name) and name in _lib.EXPORTED
    ops = open(os.path.join(ROOT, "include", "cfm_ops.h")).read()
    assert "cfm_op_decode_attention" in ops and hasattr(_lib.lib, "cfm_op_decode_attention")
    assert "cfm_op_decode_attention" in _lib.EXPORTED_OPS
    assert (_lib.DEC_ATTN_SELF_GATHER, _lib.DEC_ATTN_CROSS_GENERIC, _lib.DEC_ATTN_CROSS_MFMA) == (0, 1, 2)
    assert set(re.findall(r"\b(cfm_aed_[a-z_]+)\s*\(", hdr)) == {"cfm_aed_create", "cfm_aed_destroy",
                                                                 "cfm_aed_workspace_bytes", "cfm_aed_score"}
