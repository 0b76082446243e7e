"""Attention rescoring on the CPU: the host restatement (chunkformer_amd/rescore.py) against the reference's
recorded results (tests/golden/rescore.npz), config parsing, the model's method checks and the C-ABI exports.

Bars.  Per-token log-probs: 1e-5 (both sides are f32 torch on the CPU; the measured f32 floor of the project's
parity tests is 3e-6).  Totals: the reference accumulates them in f32 (search.py:406-421), each of its n + 1
additions rounding a partial sum of magnitude <= |total| to 2^-24 relative, so a total may differ by
(n + 1) (1e-5 + 2^-24 |total|); confidences exp(total / (n + 1)) and token confidences exp(logp) carry those
bounds through exp (relative error = the exponent's absolute error).
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import rescore_fixture as fx
from chunkformer_amd import rescore as R
from chunkformer_amd.search import DecodeResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKEN_BAR = 1e-5


def total_bar(n, total, token_bar=TOKEN_BAR):
    return (n + 1) * (token_bar + 2.0 ** -24 * abs(total))


def check_against_fixture(model, scored, token_bar, conf_slack=0.0):
    """Chosen index equal in every case and weight combination; totals, confidences and token confidences within
    the bars that `token_bar` propagates to."""
    cfg, utts = model["cfg"], model["utts"]
    enc, starts, rows, res = fx.packed(utts)
    for k, (rw, cw) in enumerate(model["combos"]):
        out = R.combine(cfg, scored, res, cw, rw)
        for u, r in zip(utts, out):
            idx, total, conf = int(u["exp"][k][0]), float(u["exp"][k][1]), float(u["exp"][k][2])
            n = len(u["hyps"][idx])
            assert r.best_index == idx and r.tokens == u["hyps"][idx] and r.times == u["times"][idx]
            tb = total_bar(n, total, token_bar)
            assert abs(r.score - total) <= tb, (r.score, total, tb)
            assert abs(r.confidence - conf) <= conf * (tb / (n + 1) + 1e-6) + conf_slack
            assert len(r.tokens_confidence) == n
            for a, b in zip(r.tokens_confidence, u["tcs"][k]):
                assert abs(a - b) <= b * (token_bar + 1e-6) + conf_slack


@pytest.fixture(scope="module")
def host_scores():
    """score_host (f32) of every model of the fixture, computed once."""
    out = {}
    for name, m in fx.load_models().items():
        enc, starts, rows, res = fx.packed(m["utts"])
        out[name] = R.score_host(m["cfg"], m["sd"], enc, starts, rows, [u["hyps"] for u in m["utts"]])
    return out


@pytest.mark.parametrize("name", ["d128h2", "d256h2", "d64h4", "uni_d64h4"])
def test_host_matches_reference(name, host_scores):
    m = fx.load_models()[name]
    err = fx.token_errors(host_scores[name], m["utts"])
    print(f"{name}: {err.size} token rows, max |host - reference| = {err.max():.2e}")
    assert err.max() <= TOKEN_BAR
    check_against_fixture(m, host_scores[name], TOKEN_BAR)


def test_fixture_covers_the_edges():
    rows_seen, lens_seen, n_cases = set(), set(), 0
    for name, m in fx.load_models().items():
        for u in m["utts"]:
            rows_seen.add(int(u["enc"].shape[0]))
            lens_seen.update(u["lens"])
            n_cases += 1
            assert 1 <= len(u["hyps"]) <= 10
    assert {0, 1, 15, 16, 17, 63, 64, 65, 129, 200} <= rows_seen
    assert {0, 1, 15, 16, 17, 31, 32, 33, 64, 70} <= lens_seen
    assert n_cases >= 38
    assert os.path.getsize(os.path.join(fx.GOLDEN, "rescore.npz")) < 1 << 20
    for name in ("d128h2", "d256h2", "d64h4"):
        m = fx.load_models()[name]
        chosen = {int(e[0]) for u in m["utts"] for e in u["exp"]}
        odd = sum(1 for u in m["utts"] for e in u["exp"][1::2]
                  if int(e[0]) != 0 and int(e[0]) != int(np.argmin(u["lens"])))
        assert len(chosen) >= 3 and odd >= 5
        # an eos inside a hypothesis, hypotheses one token apart and of different lengths
        eos = m["cfg"].eos
        assert any(eos in h for u in m["utts"] for h in u["hyps"])
        assert any(len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 1
                   for u in m["utts"] for a in u["hyps"] for b in u["hyps"])


def test_fixture_margins():
    """The best total leads every other by at least twice the largest bar the tests put on them."""
    for name, m in fx.load_models().items():
        d16 = max(fx.reference_deviation(m["utts"], s).max() for s in ("bf16", "f16"))
        assert d16 <= m["autocast_max_dev"]
        for u in m["utts"]:
            res = [DecodeResult(u["hyps"][0], nbest=u["hyps"], nbest_scores=u["ctc"], nbest_times=u["times"])]
            sc = [[(torch.from_numpy(u["l2r"][i]), None if u["r2l"] is None else torch.from_numpy(u["r2l"][i]))
                   for i in range(len(u["hyps"]))]]
            for k, (rw, cw) in enumerate(m["combos"]):
                r = R.combine(m["cfg"], sc, res, cw, rw)[0]
                tot = dict(zip(map(tuple, r.nbest), r.nbest_scores))
                for i, h in enumerate(u["hyps"]):
                    if i != r.best_index:
                        need = 2.0 * (max(len(h), len(r.tokens)) + 1) * d16
                        assert r.score - tot[tuple(h)] >= need * (1 - 1e-6), (name, k)


def test_f64_restatement_agrees_with_f32(host_scores):
    m = fx.load_models()["d64h4"]
    utts = m["utts"][:4]
    enc, starts, rows, res = fx.packed(utts)
    s64 = R.score_host(m["cfg"], m["sd"], enc, starts, rows, [u["hyps"] for u in utts], dtype=torch.float64)
    for a, b in zip(s64, host_scores["d64h4"]):
        for (l64, r64), (l32, r32) in zip(a, b):
            assert l64.dtype == torch.float64
            assert (l64 - l32.double()).abs().max() <= TOKEN_BAR and (r64 - r32.double()).abs().max() <= TOKEN_BAR


def test_padded_formulation_equals_packed(host_scores):
    """The reference's layout (hypotheses padded to a common length, padded keys masked, one memory for all)
    against one causal segment per hypothesis."""
    m = fx.load_models()["d128h2"]
    cfg = m["cfg"]
    ui = max(range(len(m["utts"])), key=lambda i: len(set(m["utts"][i]["lens"])))
    u = m["utts"][ui]
    assert len(set(u["lens"])) > 1
    W = {k: v.float() for k, v in R.native_names(cfg, m["sd"]).items()}
    pe = R.positional_table(cfg.d_model)
    L = max(u["lens"]) + 1
    for p, nb, k in ((R.LEFT, cfg.num_blocks, 0), (R.RIGHT, cfg.r_num_blocks, 1)):
        seqs = [h if k == 0 else h[::-1] for h in u["hyps"]]
        ys = torch.tensor([[cfg.sos] + s + [cfg.eos] * (L - 1 - len(s)) for s in seqs], dtype=torch.long)
        lp = R.decoder_logp_padded(W, p, cfg, nb, ys, [len(s) + 1 for s in seqs], u["enc"], pe)
        for i, s in enumerate(seqs):
            tgt = torch.tensor(s + [cfg.eos])
            got = lp[i, torch.arange(len(s) + 1), tgt]
            assert (got - host_scores["d128h2"][ui][i][k]).abs().max() <= TOKEN_BAR


def test_right_decoder_is_ignored_without_one():
    m = fx.load_models()["uni_d64h4"]
    cfg = m["cfg"]
    assert not cfg.bidirectional and not R.use_right(cfg, 0.3)
    enc, starts, rows, res = fx.packed(m["utts"][:1])
    a = R.rescore_host(cfg, m["sd"], enc, starts, rows, res, ctc_weight=0.3, reverse_weight=0.3)[0]
    b = R.rescore_host(cfg, m["sd"], enc, starts, rows, res, ctc_weight=0.3, reverse_weight=0.0)[0]
    assert a.score == b.score and a.tokens == b.tokens and a.tokens_confidence == b.tokens_confidence


def test_zero_rows_and_empty_hypothesis():
    m = fx.load_models()["d64h4"]
    cfg = m["cfg"]
    sc = R.score_host(cfg, m["sd"], torch.zeros(0, cfg.d_model), [0], [0], [[[], [3, 4]]])
    (l0, r0), (l1, r1) = sc[0]
    assert l0.shape == (1,) and r0.shape == (1,) and l1.shape == (3,)
    assert all(torch.isfinite(t).all() for t in (l0, r0, l1, r1))
    r = R.combine(cfg, sc, [DecodeResult([], nbest=[[], [3, 4]], nbest_scores=[0.0, -1.0], nbest_times=[[], [0, 0]])],
                  0.0, 0.0)[0]
    assert r.tokens == [] and r.tokens_confidence == [] and r.score == pytest.approx(float(l0[0]))
    assert r.confidence == pytest.approx(math.exp(float(l0[0])))


def test_first_strictly_larger_total_wins():
    cfg = R.AEDConfig(vocab=8, d_model=64, heads=4, ff=64, num_blocks=1, r_num_blocks=0)
    z = torch.tensor([-1.0, -1.0])
    res = [DecodeResult([1], nbest=[[1], [2], [3]], nbest_scores=[0.0, 0.0, 0.0], nbest_times=None)]
    r = R.combine(cfg, [[(z, None), (z, None), (z, None)]], res, 0.5, 0.0)[0]
    assert r.best_index == 0 and r.times is None
    with pytest.raises(ValueError):
        R.combine(cfg, [[]], [DecodeResult([1])], 0.5, 0.0)


def test_too_long_hypothesis_and_bad_token_raise():
    m = fx.load_models()["d64h4"]
    cfg = m["cfg"]
    with pytest.raises(ValueError):
        R.score_host(cfg, m["sd"], torch.zeros(1, cfg.d_model), [0], [1], [[[1] * R.MAX_POSITIONS]])
    with pytest.raises(ValueError):
        R.score_host(cfg, m["sd"], torch.zeros(1, cfg.d_model), [0], [1], [[[cfg.vocab]]])


# ------------------------------------------------------------------------------------ config
def _recipe(d, vocab, model="asr_model"):
    """The decoder part of the shipped recipes (examples/asr/*/conf/*.yaml): bitransformer, 3 + 3 blocks."""
    return {"model": model, "decoder": "bitransformer", "output_dim": vocab,
            "encoder_conf": {"output_size": d, "attention_heads": 4},
            "decoder_conf": {"attention_heads": 4, "linear_units": 2048, "num_blocks": 3, "r_num_blocks": 3,
                             "dropout_rate": 0.1, "positional_dropout_rate": 0.1, "self_attention_dropout_rate": 0.1,
                             "src_attention_dropout_rate": 0.1},
            "model_conf": {"ctc_weight": 0.3, "lsm_weight": 0.1, "length_normalized_loss": False,
                           "reverse_weight": 0.3},
            "tokenizer": "bpe", "tokenizer_conf": {"symbol_table_path": "units.txt"}}


@pytest.mark.parametrize("d, vocab", [(256, 1024), (256, 5000), (256, 5000), (512, 1024), (256, 1024)])
def test_shipped_recipe_shapes(d, vocab):
    c = R.AEDConfig.from_conf(_recipe(d, vocab), vocab, d)
    assert (c.d_model, c.heads, c.ff, c.num_blocks, c.r_num_blocks) == (d, 4, 2048, 3, 3)
    assert c.bidirectional and c.has_right and c.sos == c.eos == vocab - 1
    assert c.ctc_weight == 0.3 and c.reverse_weight == 0.3 and c.eps == 1e-5
    names = dict(R.schema(c))
    assert names["decoder.left_decoder.embed.0.weight"] == (vocab, d)
    assert names["decoder.right_decoder.decoders.2.src_attn.linear_k.weight"] == (d, d)
    assert names["decoder.left_decoder.decoders.0.feed_forward.w_1.weight"] == (2048, d)
    assert not any(k.endswith(".pe") for k in names)


def test_special_tokens_and_transformer_decoder():
    conf = _recipe(256, 1024)
    conf["tokenizer_conf"]["special_tokens"] = {"<sos>": 2, "<eos>": 3}
    c = R.AEDConfig.from_conf(conf, 1024, 256)
    assert (c.sos, c.eos) == (2, 3)
    conf["tokenizer_conf"]["special_tokens"] = {"<blank>": 0}
    c = R.AEDConfig.from_conf(conf, 1024, 256)
    assert (c.sos, c.eos) == (1023, 1023)
    conf = _recipe(256, 1024)
    conf["decoder"] = "transformer"
    c = R.AEDConfig.from_conf(conf, 1024, 256)
    assert not c.bidirectional and c.r_num_blocks == 0 and not c.has_right
    assert all(k.startswith("decoder.embed.") or k.startswith("decoder.decoders.") or k.startswith("decoder.after_norm.")
               or k.startswith("decoder.output_layer.") for k, _ in R.schema(c))
    sd = R.synthetic_decoder_state_dict(R.AEDConfig(vocab=16, d_model=64, heads=4, ff=64, num_blocks=1, r_num_blocks=0,
                                                    bidirectional=False))
    named = R.native_names(R.AEDConfig(vocab=16, d_model=64, heads=4, ff=64, num_blocks=1, r_num_blocks=0,
                                       bidirectional=False), sd)
    assert all(k.startswith(R.LEFT) for k in named)
    conf = _recipe(256, 1024)
    del conf["decoder"], conf["model_conf"]
    c = R.AEDConfig.from_conf(conf, 1024, 256)    # init_model.py:81 and the ASRModel defaults
    assert not c.bidirectional and c.ctc_weight == 0.5 and c.reverse_weight == 0.0


@pytest.mark.parametrize("key, value", [("normalize_before", False), ("layer_norm_type", "rms_norm"), ("use_sdpa", True),
                                        ("n_kv_head", 2), ("head_dim", 32), ("mlp_type", "moe"),
                                        ("activation_type", "gelu"), ("tie_word_embedding", True),
                                        ("src_attention", False)])
def test_unsupported_decoder_settings_raise(key, value):
    conf = _recipe(256, 1024)
    conf["decoder_conf"][key] = value
    with pytest.raises(AssertionError):
        R.AEDConfig.from_conf(conf, 1024, 256)


def test_unknown_decoder_type_raises():
    conf = _recipe(256, 1024)
    conf["decoder"] = "paraformer"
    with pytest.raises(AssertionError):
        R.AEDConfig.from_conf(conf, 1024, 256)


def test_missing_and_misshaped_weights_raise():
    c = R.AEDConfig(vocab=16, d_model=64, heads=4, ff=64, num_blocks=1, r_num_blocks=1)
    sd = R.synthetic_decoder_state_dict(c)
    sd["decoder.left_decoder.embed.1.pe"] = torch.zeros(1, 5000, 64)     # ignored: the table is computed
    assert "decoder.left_decoder.embed.1.pe" not in R.native_names(c, sd)
    bad = dict(sd)
    del bad["decoder.right_decoder.after_norm.bias"]
    with pytest.raises(KeyError):
        R.native_names(c, bad)
    bad = dict(sd)
    bad["decoder.left_decoder.output_layer.bias"] = torch.zeros(15)
    with pytest.raises(ValueError):
        R.native_names(c, bad)


def test_positional_table_is_the_references():
    pe = R.positional_table(64)
    assert pe.shape == (5000, 64) and pe.dtype == torch.float32
    pos, i = 4999.0, 10
    div = math.exp(2 * i * -(math.log(10000.0) / 64))
    assert abs(float(pe[4999, 2 * i]) - math.sin(pos * div)) < 1e-3     # f32 argument reduction at pos ~ 5000
    assert float(pe[0, 0]) == 0.0 and float(pe[0, 1]) == 1.0


# ------------------------------------------------------------------------------------ model
def _bare_model(model_type, rescorer=None):
    from chunkformer_amd.model import ChunkFormerModel
    m = ChunkFormerModel.__new__(ChunkFormerModel)
    m.model_type = model_type
    m.is_classification = model_type == "classification"
    m.rescorer = rescorer
    return m


def test_beam_method_accepts_attention_rescoring():
    m = _bare_model("asr_model", rescorer=object())
    assert m._beam_method("ctc_greedy_search") is False
    assert m._beam_method("ctc_prefix_beam_search") is True
    assert m._beam_method("attention_rescoring") is True
    with pytest.raises(ValueError):
        m._beam_method("attention")
    with pytest.raises(ValueError):
        m._beam_method("transducer_attention_rescoring")


def test_attention_rescoring_needs_a_decoder():
    m = _bare_model("asr_model")
    assert m._beam_method("ctc_prefix_beam_search") is True      # unchanged without a decoder
    with pytest.raises(ValueError, match="decoder"):
        m._beam_method("attention_rescoring")
    with pytest.raises(ValueError, match="transducer"):
        _bare_model("transducer", rescorer=object())._beam_method("attention_rescoring")
    m = _bare_model("classification")
    with pytest.raises(ValueError, match="classification"):
        m._require_asr("batch_decode")


# ------------------------------------------------------------------------------------ C-ABI
def test_aed_symbols_are_exported():
    from chunkformer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cfm.h")).read()
    declared = set(re.findall(r"\b(cfm_aed_[a-z_]+)\s*\(", hdr))
    assert declared == {"cfm_aed_create", "cfm_aed_destroy", "cfm_aed_workspace_bytes", "cfm_aed_score"}
    for name in declared:
        assert hasattr(_lib.lib, name) and name in _lib.EXPORTED
    ops = open(os.path.join(ROOT, "include", "cfm_ops.h")).read()
    assert "cfm_op_seg_attention" in ops and hasattr(_lib.lib, "cfm_op_seg_attention")
    assert "cfm_op_seg_attention" in _lib.EXPORTED_OPS
    assert ctypes_sizeof_config(_lib) == 40


def ctypes_sizeof_config(_lib):
    import ctypes
    return ctypes.sizeof(_lib.CfmAedConfig)
