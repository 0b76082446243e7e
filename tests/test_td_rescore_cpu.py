"""Transducer attention rescoring on the CPU: the restatement (chunkformer_amd.transducer_rescore) against brute-force
enumeration and against tests/golden/td_rescore.npz, the dispatch of the two decoding methods and their error cases,
and the workspace sizes that need no device."""
import numpy as np
import pytest
import torch

import rnnt_beam_fixture as F
import td_rescore_fixture as X
from chunkformer_amd import model as M
from chunkformer_amd import transducer_rescore as TR


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("U", [0, 1, 2, 3, 4])
def test_recursion_equals_enumeration(T, U):
    g = np.random.default_rng(100 * T + U)
    for _ in range(3):
        b, k = -4.0 * g.random((T, U + 1)), -6.0 * g.random((T, U))
        want = TR.td_score_enum(b, k)
        assert abs(TR.td_score_host(b, k) - want) <= 1e-12 * max(1.0, abs(want))


def test_one_frame_no_tokens_is_the_blank():
    assert TR.td_score_host([[-0.25]], np.zeros((1, 0))) == -0.25
    with pytest.raises(ValueError):
        TR.td_score_host(np.zeros((0, 1)), np.zeros((0, 0)))


def test_fixture_conditions():
    cases = X.cases()
    eq = [c for c in cases if c["equality"]]
    assert len(cases) >= 100 and len(eq) >= 0.9 * len(cases)
    assert 3 * sum(1 for c in eq if c["best_index"] != 0) >= len(eq)
    assert {c["mode"] for c in cases} == {"transducer", "ctc"} and {c["decoder"] for c in cases} == {"uni", "bi"}
    ran = [c for c in cases if c["ref_index"] >= 0]
    assert len(ran) >= 50 and all(c["ref_index"] == c["best_index"] for c in ran if c["equality"])


def _host_case(i):
    c = X.case(i)
    host = F.host_model(c["model"], c["recipe"])
    aed = X.decoder(c["decoder"], host.cfg.vocab)
    got = TR.rescore_host(host, aed, c["enc"], [0], [c["rows"]], [c["result"]], c["ctc_weight"], c["attn_weight"],
                          c["transducer_weight"], c["reverse_weight"])[0]
    return c, got


@pytest.mark.parametrize("part", range(6))
def test_rescore_host_reproduces_the_fixture(part):
    for i in range(part, len(X.cases()), 6):
        c, got = _host_case(i)
        assert np.allclose(got.td_scores, c["td"], rtol=0, atol=1e-9), i
        assert np.allclose(got.decoder_scores, c["attn"], rtol=0, atol=1e-9), i
        assert np.allclose(got.nbest_scores, c["totals"], rtol=0, atol=1e-9), i
        assert got.best_index == c["best_index"] and abs(got.score - c["score"]) <= 1e-9, i
        assert got.tokens == c["result"].nbest[c["best_index"]]


def test_td_score_host_against_the_recorded_values():
    for i in (0, 17, 40, 77, 111):
        c = X.case(i)
        host = F.host_model(c["model"], c["recipe"])
        for h, want in zip(c["result"].nbest, c["td"]):
            assert abs(TR.td_score_host(*TR.lattice_logp_host(host, c["enc"], h)) - want) <= 1e-9


def test_f32_lattice_is_close_to_f64():
    c = X.case(40)
    host = F.host_model(c["model"], c["recipe"])
    for h in c["result"].nbest[:4]:
        b64, k64 = TR.lattice_logp_host(host, c["enc"], h)
        b32, k32 = TR.lattice_logp_host(host, c["enc"], h, torch.float32)
        assert b32.dtype == np.float32 and np.abs(b64 - b32).max() <= 1e-5
        assert abs(TR.td_score_host(b64, k64) - TR.td_score_host(b32, k32)) <= (c["rows"] + len(h) + 1) * 1e-5


def test_zero_row_utterance_keeps_its_result_and_return_nbest_reranks():
    c = X.case(3)
    host = F.host_model(c["model"], c["recipe"])
    empty = X.case(3)["result"]
    out = TR.rescore_host(host, None, c["enc"], [0, 0], [0, c["rows"]], [empty, c["result"]], 0.5, None, 0.5,
                          return_nbest=True)
    assert out[0] is empty
    assert out[1].nbest_scores == sorted(out[1].nbest_scores, reverse=True) and out[1].decoder_scores == [0.0] * len(c["td"])
    assert out[1].nbest[0] == out[1].tokens
    with pytest.raises(ValueError):
        TR.rescore_host(host, None, c["enc"], [0], [c["rows"]], [c["result"]], 0.5, 0.5, 0.5)   # attn without decoder


def test_groups_respect_the_soft_cap():
    assert TR._groups([10, 10, 10], 8 * 20) == [[0, 1], [2]]
    assert TR._groups([100, 1, 1], 8 * 10) == [[0], [1, 2]]
    assert TR._groups([], 8) == []


# ----------------------------------------------------------------------------- dispatch on a bare model
def _bare(model_type, rnnt=None, rescorer=None):
    m = M.ChunkFormerModel.__new__(M.ChunkFormerModel)
    m.char_dict, m.model_type, m.is_classification = None, model_type, model_type == "classification"
    m.rnnt, m.rescorer, m.encoder, m._td_rescorer, m._dtype, m._aed_unsupported = rnnt, rescorer, object(), None, "fp32", None
    return m


class _Rnnt:
    cfg, device = F.model("v17", "dense")[0], torch.device("cpu")


def test_dispatch_of_the_two_methods():
    m = _bare("transducer", _Rnnt())
    a = m._resolve_decoding("rnnt_beam_attn_rescoring")
    b = m._resolve_decoding("ctc_beam_td_attn_rescoring")
    assert (a.method, a.lens, a.timed) == ("rnnt_beam_attn_rescoring", "rnnt", True)
    assert (b.method, b.lens, b.timed) == ("ctc_beam_td_attn_rescoring", "ctc", True)
    assert a.searcher is b.searcher and isinstance(a.searcher, TR.TransducerRescorer) and a.searcher.rescorer is None
    # the existing methods resolve as before
    assert m._resolve_decoding("ctc_greedy_search") is None
    assert m._resolve_decoding("rnnt_beam_search").method == "rnnt_beam_search"


@pytest.mark.parametrize("method", ["rnnt_beam_attn_rescoring", "ctc_beam_td_attn_rescoring"])
def test_errors_name_the_mode(method):
    for kind in ("asr_model", "classification"):
        with pytest.raises(ValueError, match=method):
            _bare(kind)._resolve_decoding(method)
    m = _bare("transducer", _Rnnt())
    mode = m._resolve_decoding(method)
    with pytest.raises(ValueError, match="attn_weight"):
        m._search_rows(mode, torch.zeros(0, 32), [], [], attn_weight=0.3)
    m._aed_unsupported = "decoder rms_norm is not supported"
    with pytest.raises(ValueError, match="rms_norm"):
        m._search_rows(mode, torch.zeros(0, 32), [], [], attn_weight=0.3)


def _decoder_checkpoint(**decoder_conf):
    from chunkformer_amd import rescore as R
    aed = R.AEDConfig(vocab=48, d_model=64, heads=2, ff=64, num_blocks=1, r_num_blocks=1)
    conf = {"model": "transducer", "decoder": "bitransformer",
            "decoder_conf": dict({"attention_heads": 2, "linear_units": 64, "num_blocks": 1, "r_num_blocks": 1},
                                 **decoder_conf)}
    return conf, dict(R.synthetic_decoder_state_dict(aed, 1)), aed


def test_transducer_checkpoint_decoder_config():
    """from_pretrained's decision for `model: transducer` checkpoints: a decoder the rescorer runs gives its config, one
    it cannot run gives the reason and no config (the checkpoint loads as it did without decoder.*), none gives
    neither."""
    conf, sd, aed = _decoder_checkpoint()
    cfg, why = M.transducer_decoder_config(conf, sd, 48, 64)
    assert why is None and (cfg.d_model, cfg.heads, cfg.ff, cfg.num_blocks, cfg.r_num_blocks, cfg.bidirectional) == \
        (64, 2, 64, 1, 1, True)
    assert M.transducer_decoder_config(conf, {"joint.ffn_out.bias": torch.zeros(48)}, 48, 64) == (None, None)
    conf_rms, _, _ = _decoder_checkpoint(layer_norm_type="rms_norm")
    cfg, why = M.transducer_decoder_config(conf_rms, sd, 48, 64)
    assert cfg is None and "rms_norm" in why
    short = {k: v for k, v in sd.items() if "output_layer.bias" not in k}
    cfg, why = M.transducer_decoder_config(conf, short, 48, 64)
    assert cfg is None and "output_layer.bias" in why
    cfg, why = M.transducer_decoder_config(dict(conf, decoder="paraformer"), sd, 48, 64)
    assert cfg is None and "paraformer" in why


def test_combine_td_takes_decoder_scores_formed_elsewhere():
    c = X.case(0)
    td = [c["td"]]
    got = TR.combine_td(None, None, td, [c["result"]], c["ctc_weight"], c["attn_weight"], c["transducer_weight"],
                        attn_scores=[c["attn"]])[0]
    assert got.best_index == c["best_index"] and np.allclose(got.nbest_scores, c["totals"], rtol=0, atol=1e-12)
    assert got.decoder_scores == c["attn"]
    with pytest.raises(ValueError):
        TR.combine_td(None, None, td, [c["result"]], 0.5, 0.5, 0.5, attn_scores=[c["attn"][:-1]])


def test_new_arguments_default_to_none_before_the_pinned_tail():
    """The tail of the two signatures is pinned by test_rnnt_beam_cpu.py and test_attention_decode_cpu.py, so the new
    arguments stand before it (they are meant to be passed by keyword)."""
    import inspect
    for fn in (M.ChunkFormerModel.batch_decode, M.ChunkFormerModel.endless_decode):
        p = inspect.signature(fn).parameters
        names = list(p)
        assert names[-8:-5] == ["attn_weight", "search_ctc_weight", "search_transducer_weight"]
        assert all(p[k].default is None for k in names[-8:-5])


def test_workspace_sizes_without_a_device():
    from chunkformer_amd import _lib
    assert int(_lib.cfm_rnnt_td_workspace_bytes(None, 10, 2, 6, 3, 60)) == 0   # no handle
    small = int(_lib.cfm_op_rnnt_alpha_workspace_bytes(4, 2048))
    big = int(_lib.cfm_op_rnnt_alpha_workspace_bytes(4, 2049))
    assert 0 < small < big and big >= 4 * 2 * 2049 * 8
    assert int(_lib.cfm_op_rnnt_alpha_workspace_bytes(0, 5)) == 0 and int(_lib.cfm_op_rnnt_alpha_workspace_bytes(3, 0)) == 0
