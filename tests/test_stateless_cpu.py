"""CPU: the stateless transducer predictors (embedding, conv) -- configuration, schema, synthetic weights and the host
restatements against the reference's recorded results (tests/golden/rnnt_stateless.npz, gen_golden_stateless.py)."""
import hashlib

import numpy as np
import pytest
import torch

import stateless_fixture as fx
from chunkformer_amd import transducer_beam as TB
from chunkformer_amd import transducer_rescore as TR
from chunkformer_amd.transducer import RNNTConfig, schema, synthetic_transducer_state_dict

JOINT = {"enc_output_size": 32, "pred_output_size": 64, "join_dim": 96}


def _conf(kind, **pc):
    base = {"embed_size": 64, "output_size": 64, "embed_dropout": 0.1}
    if kind == "embedding":
        base["n_head"] = 4
    base.update(pc)
    return {"predictor": kind, "predictor_conf": base, "joint": "transducer_joint", "joint_conf": dict(JOINT)}


def test_from_conf_schema_validate():
    c = RNNTConfig.from_conf(_conf("embedding", history_size=3, bias=True, layer_norm_epsilon=1e-3), 100, 32)
    assert (c.predictor, c.history_size, c.context, c.n_head, c.act, c.ln_eps) == ("embedding", 3, 4, 4, "swish", 1e-3)
    assert c.pos_bias and not c.conv_bias and c.stateless and (c.embed_size, c.pred_out, c.join_dim) == (64, 64, 96)
    c.validate()
    assert dict(schema(c)) == {
        "predictor.embed.weight": (100, 64), "predictor.pos_embed.weight": (4, 256), "predictor.pos_embed.bias": (4,),
        "predictor.ffn.weight": (64, 64), "predictor.ffn.bias": (64,), "predictor.norm.weight": (64,),
        "predictor.norm.bias": (64,), "joint.enc_ffn.weight": (96, 32), "joint.enc_ffn.bias": (96,),
        "joint.pred_ffn.weight": (96, 64), "joint.pred_ffn.bias": (96,), "joint.ffn_out.weight": (100, 96),
        "joint.ffn_out.bias": (100,)}
    c = RNNTConfig.from_conf(_conf("conv", history_size=0, bias=True, activation="gelu"), 100, 32)
    assert (c.predictor, c.context, c.act, c.conv_bias, c.pos_bias) == ("conv", 1, "gelu", True, False)
    c.validate()
    assert dict(schema(c))["predictor.conv.weight"] == (64, 1, 1) and dict(schema(c))["predictor.conv.bias"] == (64,)
    c = RNNTConfig.from_conf(_conf("conv"), 100, 32)
    assert (c.history_size, c.act, c.conv_bias) == (2, "relu", False)
    assert "predictor.conv.bias" not in dict(schema(c)) and not any(k.startswith("predictor.rnn") for k, _ in schema(c))
    for act in ("relu", "swish", "tanh", "gelu"):
        assert RNNTConfig.from_conf(_conf("embedding", activation=act), 100, 32).act == act
    # the rnn form is parsed as before
    r = RNNTConfig.from_conf({"predictor": "rnn", "predictor_conf": {"embed_size": 32, "hidden_size": 64, "num_layers": 2,
                                                                     "output_size": 48}, "joint_conf": {"join_dim": 96}}, 50, 32)
    assert (r.predictor, r.hidden, r.num_layers, r.pred_out, r.stateless) == ("rnn", 64, 2, 48, False)


@pytest.mark.parametrize("conf", [
    _conf("embedding", activation="hardtanh"), _conf("conv", activation="selu"), _conf("conv", output_size=32),
    _conf("embedding", history_size=-1), {**_conf("conv"), "joint_conf": {**JOINT, "hat_joint": True}},
    {**_conf("embedding"), "joint_conf": {**JOINT, "postjoin_linear": True}}, {**_conf("conv"), "predictor": "gru"}])
def test_rejected_settings_still_raise(conf):
    with pytest.raises(AssertionError):
        RNNTConfig.from_conf(conf, 100, 32)


def test_validate_limits():
    ok = dict(vocab=20, enc_dim=32, embed_size=32, pred_out=32, join_dim=32, predictor="embedding")
    RNNTConfig(**ok, history_size=8, n_head=1).validate()
    for bad in (dict(history_size=9), dict(n_head=0), dict(embed_size=30, pred_out=30), dict(embed_size=2048, pred_out=2048),
                dict(pred_out=64)):
        with pytest.raises(AssertionError):
            RNNTConfig(**{**ok, **bad}).validate()


def _digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.numpy().tobytes())
    return h.hexdigest()


def test_rnn_synthetic_weights_unchanged():
    """sha256 over (key, bytes) of the rnn state dicts, computed on the commit before the stateless predictors."""
    assert _digest(synthetic_transducer_state_dict(RNNTConfig(), seed=0)) == \
        "13ed38433c666164153e705b0bd242ed2a3d511cbef8480fa381cd3e5bbc701a"
    small = RNNTConfig(vocab=37, enc_dim=32, embed_size=32, hidden=32, num_layers=1, pred_out=32, join_dim=32)
    assert _digest(synthetic_transducer_state_dict(small, seed=22)) == \
        "a33346609a50dc4e16fb2f83084c1bad630c3599d90ede0c4624cda75cd727e4"


def test_synthetic_stateless_weights():
    for name in fx.names():
        cfg, sd = fx.model(name)
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in schema(cfg)]
        assert torch.equal(sd["predictor.norm.weight"], torch.ones(cfg.embed_size))
        assert torch.equal(sd["predictor.norm.bias"], torch.zeros(cfg.embed_size))
        if cfg.predictor == "conv":
            assert float(sd["predictor.conv.weight"].abs().max()) <= cfg.context ** -0.5


@pytest.mark.parametrize("name", fx.names())
def test_predictor_against_the_reference(name):
    """step_windows (f32, the reference's shapes) reproduces the recorded forward_step outputs; the f64 context
    function is within the recorded e_ref of them, e_ref itself of f32 size."""
    host = fx.host_model(name)
    win, ref, e_ref = fx.predictor_points(name)
    assert (win[: host.cfg.history_size + 1, 0] == -1).sum() == host.cfg.history_size   # windows that start before the sos
    got = host.step_windows(win).reshape(ref.shape).numpy()
    assert float(np.abs(got - ref).max()) <= 1e-6
    f64 = host.predict_windows(win, torch.float64).numpy()
    assert float(np.abs(f64 - ref).max()) <= e_ref * (1 + 1e-9) and 0 < e_ref < 1e-5
    # positions before the sos are zero vectors, not the blank's embedding
    if host.cfg.history_size:
        blanked = np.where(win < 0, host.cfg.blank, win)
        assert float(np.abs(host.predict_windows(blanked[:1]).numpy() - f64[:1]).max()) > 1e-3


@pytest.mark.parametrize("name", fx.names())
def test_greedy_host_equals_the_reference(name):
    host = fx.host_model(name)
    cases = fx.greedy_cases(name)
    cnt = (cases[0]["dense"] != 0).sum(1)
    assert cases[0]["n_steps"] == 4 and (cnt == 0).any() and ((cnt >= 1) & (cnt <= 3)).any() and (cnt == 4).any()
    for c in cases:
        dense, gap = TB.greedy_host(host, c["enc"], c["starts"], c["lens"], c["n_steps"])
        assert gap >= 1e-3 and abs(gap - c["gap"]) <= 1e-5
        assert np.array_equal(dense, c["dense"])
        for s, n, ref in zip(c["starts"], c["lens"], c["ref_tokens"]):
            flat = dense[s: s + n].reshape(-1)
            assert flat[flat != 0].tolist() == ref


@pytest.mark.parametrize("name", fx.names())
def test_prefix_beam_search_host_reproduces_every_beam(name):
    host = fx.host_model(name)
    for c in fx.beam_cases(name):
        res = TB.prefix_beam_search_host(host, c["enc"], c["ctc"], [0], [c["rows"]], c["beam"], c["cw"], c["tw"])[0]
        assert res.nbest == c["tokens"]
        np.testing.assert_allclose(res.nbest_scores, c["scores"], rtol=0, atol=1e-9)
        assert np.array_equal(res.trace["parent"], c["trace"]["parent"]) and res.fusions == c["fusions"]
        if c["equality"]:
            assert res.margin >= 2 * (c["rows"] + 1) * 1e-5


def test_fixture_conditions():
    fus = {"embedding": 0, "conv": 0}
    for name in fx.names():
        cfg, _ = fx.model(name)
        fus[cfg.predictor] += sum(1 for c in fx.beam_cases(name) if c["equality"] and c["fusions"] > 0)
        assert {c["beam"] for c in fx.beam_cases(name)} >= ({16} if cfg.vocab == 17 else {1, 5, 16})
        assert {tuple(c["lens"]) for c in fx.greedy_cases(name)} >= {(1,), (7,), (33,), (48,), (7, 33, 1)}
    assert min(fus.values()) >= 3


@pytest.mark.parametrize("name", fx.names())
def test_td_restatement(name):
    """The recorded td of the reference (its predictor's training form and joint) against lattice_logp_host +
    td_score_host, the recursion against the enumeration of every alignment on tiny lattices, and the recorded
    rescoring choices."""
    host = fx.host_model(name)
    K = host.cfg.context
    for c in fx.td_cases(name):
        assert [len(h) for h in c["hyps"]] == [0, 1, K - 1, K, K + 1]
        for h, want, ref in zip(c["hyps"], c["td"], c["td_ref"]):
            b, k = TR.lattice_logp_host(host, c["enc"], h)
            got = TR.td_score_host(b, k)
            assert abs(got - want) <= 1e-9 and abs(got - ref) <= (c["rows"] + len(h) + 1) * 1e-5
    c = fx.td_cases(name)[1]
    for h in c["hyps"]:
        b, k = TR.lattice_logp_host(host, c["enc"][:3], h[:3])
        assert abs(TR.td_score_host(b, k) - TR.td_score_enum(b, k)) <= 1e-9
    from chunkformer_amd.search import DecodeResult
    for c in fx.beam_cases(name)[:4]:
        res = DecodeResult(list(c["tokens"][0]), c["scores"][0], nbest=c["tokens"], nbest_scores=c["scores"])
        got = TR.rescore_host(host, None, c["enc"], [0], [c["rows"]], [res], 0.5, 0.0, 0.5)[0]
        np.testing.assert_allclose(got.td_scores, c["td"], rtol=0, atol=1e-9)
        assert got.best_index == c["best_index"]


def test_windows_never_cross_hypotheses():
    cfg, _ = fx.model("emb_v130")
    w = TB.hyp_windows(cfg, [5, 6])
    assert w.tolist() == [[-1, -1, -1, -1, 0], [-1, -1, -1, 0, 5], [-1, -1, 0, 5, 6]]
