"""Transducer attention rescoring on the device, end to end: every case of tests/golden/td_rescore.npz through
TransducerRescorer, the group split, the workspace sizes, the bf16 lattice kernel against the f64 restatement, and
batch_decode / endless_decode with the two decoding methods.

The fixture's attention decoders have d_model 32 (the fixture models' enc_dim), which the device decoder does not take
(its widths are multiples of 64), so the fixture cases go through TransducerRescorer.rescore with td from the device
and attn handed in from the archive (`attn_scores`: the restatement's, which test_td_rescore_cpu.py reproduces), and the
shipped combination makes the choice; the device decoder's part of the mode is checked on a
synthetic transducer checkpoint with a d_model 64 decoder against the host restatement and through the model API.

bf16 lattice kernel (bf16 operands, ffn_out as two bf16 terms, f32 accumulation) against the f64 restatement,
measured on an MI355X: per total over the fixture (126 cases, 1,166 hypotheses) and the J = 512 / V = 1,024 /
T = 33 / U = 17 case, per node over the first four hypotheses of the last case of every model and recipe (v17, v37, v130, v1024; J = 32 and 64; V = 130 has a
partly padded vocabulary tile) and that J = 512 case:
    largest per-node deviation   1.096e-2   (BF16_NODE_MEASURED)
    largest per-total deviation  3.783e-2   (BF16_TOTAL_MEASURED; the J = 512 case alone: 1.7e-4)
The test asserts twice these (the margin covers the run-to-run and box-to-box spread of a deviation that depends on
rounding flips); choices must equal the fp32 ones wherever the recorded margin exceeds twice the measured total
deviation, and those must be at least 80% of the equality cases (0.0757 is exceeded by 114 of the 126 margins).

With ffn_out as one bf16 term the same measurement gave 1.374e-2 per node and 1.376e-1 per total, of which 0.10 came
from the weights' rounding alone (a fixed error that does not average out along a lattice; a CPU emulation of the
operand rounding reproduces both figures to four digits), and only 90 of the 126 margins exceeded twice that; hence
the second term."""
import functools

import numpy as np
import pytest
import torch

import rnnt_beam_fixture as F
import td_rescore_fixture as X
from test_gpu_td_rescore_ops import _lattice_case, _worst, device_model, wide_case

pytestmark = pytest.mark.gpu

BF16_NODE_MEASURED = 1.096e-2
BF16_TOTAL_MEASURED = 3.783e-2


def _by_model():
    out = {}
    for i, c in enumerate(X.cases()):
        out.setdefault((c["model"], c["recipe"]), []).append(i)
    return out


@functools.lru_cache(maxsize=None)
def device_td(dtype):
    """{case index: td list} of every fixture case, one packed call per model and recipe."""
    from chunkformer_amd.transducer_rescore import TransducerRescorer
    out = {}
    for (name, recipe), idx in _by_model().items():
        tr = TransducerRescorer(device_model(name, recipe).rnnt, None, dtype)
        cs = [X.case(i) for i in idx]
        enc = torch.cat([c["enc"] for c in cs])
        lens = [c["rows"] for c in cs]
        starts = np.cumsum([0] + lens[:-1]).tolist()
        td = tr.td_scores(enc, starts, lens, [c["result"].nbest for c in cs])
        assert tr.last_error == 0
        for i, t in zip(idx, td):
            out[i] = t
    return out


def _choice(c, td):
    totals = [a * c["attn_weight"] + s * c["ctc_weight"] + t * c["transducer_weight"]
              for a, s, t in zip(c["attn"], c["result"].nbest_scores, td)]
    best = 0
    for i in range(1, len(totals)):
        if totals[i] > totals[best]:
            best = i
    return best, totals


def test_fixture_fp32():
    """Every fixture case through TransducerRescorer.rescore, one packed call per model and recipe and weight triple."""
    from chunkformer_amd.transducer_rescore import TransducerRescorer
    worst, n_eq = 0.0, 0
    for (name, recipe), idx in _by_model().items():
        tr = TransducerRescorer(device_model(name, recipe).rnnt, None, "fp32")
        by_w = {}
        for i in idx:
            m = X.cases()[i]
            by_w.setdefault((m["ctc_weight"], m["attn_weight"], m["transducer_weight"]), []).append(i)
        for (cw, aw, tw), ids in by_w.items():
            cs = [X.case(i) for i in ids]
            lens = [c["rows"] for c in cs]
            starts = np.cumsum([0] + lens[:-1]).tolist()
            res = tr.rescore([c["result"] for c in cs], torch.cat([c["enc"] for c in cs]), starts, lens, cw, aw, tw,
                             attn_scores=[c["attn"] for c in cs])
            assert tr.last_error == 0
            for i, c, r in zip(ids, cs, res):
                for h, got, want in zip(c["result"].nbest, r.td_scores, c["td"]):
                    worst = max(worst, abs(got - want) / ((c["rows"] + len(h) + 1) * 1e-5))
                    assert abs(got - want) <= (c["rows"] + len(h) + 1) * 1e-5, (i, got, want)
                assert r.decoder_scores == c["attn"]
                if c["equality"]:
                    n_eq += 1
                    assert r.best_index == c["best_index"] and r.tokens == c["result"].nbest[c["best_index"]], i
                    assert abs(r.score - c["score"]) <= (c["rows"] + len(r.tokens) + 1) * 1e-5 * tw, i
    print(f"fp32: largest |td - recorded| / ((T + U + 1) 1e-5) = {worst:.3f}; {n_eq} equality cases")
    assert n_eq >= 100


def test_rescore_results_without_decoder():
    """TransducerRescorer.rescore on the cases with attn_weight 0: the chosen index, tokens, totals and td of the
    result object."""
    from chunkformer_amd.transducer_rescore import TransducerRescorer
    n = 0
    for i, m in enumerate(X.cases()):
        if m["attn_weight"] != 0 or not m["equality"] or i % 4:
            continue
        c = X.case(i)
        tr = TransducerRescorer(device_model(c["model"], c["recipe"]).rnnt, None, "fp32")
        r = tr.rescore([c["result"]], c["enc"], [0], [c["rows"]], c["ctc_weight"], None, c["transducer_weight"])[0]
        assert r.best_index == c["best_index"] and r.tokens == c["result"].nbest[c["best_index"]]
        assert r.decoder_scores == [0.0] * len(c["td"]) and len(r.td_scores) == len(c["td"])
        assert abs(r.score - c["score"]) <= (c["rows"] + len(r.tokens) + 1) * 1e-5 * c["transducer_weight"]
        n += 1
    assert n >= 5


def test_group_split_is_bit_identical():
    from chunkformer_amd.transducer_rescore import TransducerRescorer
    idx = _by_model()[("v130", "dense")][:8]
    cs = [X.case(i) for i in idx]
    enc = torch.cat([c["enc"] for c in cs])
    lens = [c["rows"] for c in cs]
    starts = np.cumsum([0] + lens[:-1]).tolist()
    nbest = [c["result"].nbest for c in cs]
    rnnt = device_model("v130", "dense").rnnt
    one = TransducerRescorer(rnnt, None, "fp32")
    whole = one.td_scores(enc, starts, lens, nbest)
    assert one.last_groups == 1
    split = TransducerRescorer(rnnt, None, "fp32", max_lattice_bytes=1)   # every hypothesis alone
    parts = split.td_scores(enc, starts, lens, nbest)
    assert split.last_groups == sum(len(n) for n in nbest)
    assert parts == whole
    some = TransducerRescorer(rnnt, None, "fp32", max_lattice_bytes=8 * 3000)
    assert some.td_scores(enc, starts, lens, nbest) == whole and 1 < some.last_groups < split.last_groups


def test_workspace_bytes():
    from chunkformer_amd import _lib
    h = device_model("v37").rnnt._h
    a = int(_lib.cfm_rnnt_td_workspace_bytes(h, 65, 4, 200, 12, 2600))
    b = int(_lib.cfm_rnnt_td_workspace_bytes(h, 65, 4, 200, 12, 2601))
    c = int(_lib.cfm_rnnt_td_workspace_bytes(h, 65, 4, 200, 12, 2600 + 4096))
    assert 0 < a <= b < c and c - a >= 8 * 4096
    for bad in ((0, 4, 40, 12, 100), (65, 0, 40, 12, 100), (65, 4, 3, 12, 100), (65, 4, 40, 0, 100), (65, 4, 40, 41, 100),
                (65, 4, 40, 12, 3), (65, 4, 40, 12, 65 * 40 + 1)):
        assert int(_lib.cfm_rnnt_td_workspace_bytes(h, *bad)) == 0, bad


def test_bad_arguments():
    tr = device_model("v37")
    enc = torch.zeros(4, tr.cfg.enc_dim)
    with pytest.raises(ValueError):
        tr.td_scores(enc, [0], [4], [[[1, tr.cfg.vocab]]])
    with pytest.raises(ValueError):
        tr.td_scores(enc, [0], [5], [[[1]]])
    with pytest.raises(ValueError):
        tr.rescore([X.case(0)["result"]], enc, [0], [4], 0.5, 0.5, 0.5)    # attn_weight without a decoder
    assert tr.td_scores(enc, [0, 2], [0, 2], [[[1, 2]], [[]]])[0] is None


def test_bf16_against_the_restatement():
    td32, td16 = device_td("fp32"), device_td("bf16")
    total, flips, held = 0.0, 0, 0
    eq = [i for i, c in enumerate(X.cases()) if c["equality"]]
    for i in range(len(X.cases())):
        c = X.case(i)
        total = max(total, max(abs(a - b) for a, b in zip(td16[i], c["td"])))
    # per node: the op against the f64 lattice on a case of every model and recipe, and the J = 512 case
    node = 0.0
    for (name, recipe), idx in _by_model().items():
        tr = device_model(name, recipe)
        c = X.case(idx[-1])
        hyps = [(0, h) for h in c["result"].nbest[:4]]
        node = max(node, _worst(*_lattice_case(tr, F.host_model(name, recipe), [c["enc"]], hyps, "bf16")))
    tr, host, enc, hyps = wide_case()
    got, want = _lattice_case(tr, host, enc, hyps, "bf16")
    node = max(node, _worst(got, want))
    from chunkformer_amd import transducer_rescore as TR
    wide_total = abs(TR.td_score_host(*got[0]) - TR.td_score_host(*want[0]))
    total = max(total, wide_total)
    print(f"bf16: largest per-node deviation {node:.4e}, largest per-total deviation {total:.4e} (J = 512 total {wide_total:.4e})")
    for i in eq:
        c = X.case(i)
        if c["margin"] > 2 * BF16_TOTAL_MEASURED:
            held += 1
            b16, b32 = _choice(c, td16[i])[0], _choice(c, td32[i])[0]
            flips += b16 != b32
    print(f"bf16: {held} of {len(eq)} equality cases above the margin, {flips} choices differ from fp32")
    assert node <= 2 * BF16_NODE_MEASURED and total <= 2 * BF16_TOTAL_MEASURED
    assert held >= 0.8 * len(eq) and flips == 0


# ----------------------------------------------------------------------------- with a device decoder, and the model API
@pytest.fixture(scope="module")
def transducer_model():
    import dataclasses

    from chunkformer_amd import rescore as R
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.transducer import RNNTConfig, synthetic_transducer_state_dict
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    c = RNNTConfig(vocab=96, enc_dim=SMALL.d_model, embed_size=32, hidden=64, num_layers=1, pred_out=64, join_dim=64)
    cfg = dataclasses.replace(SMALL, vocab=c.vocab)
    sd = synthetic_state_dict(SMALL, 5)
    gen = torch.Generator().manual_seed(11)
    sd["ctc.ctc_lo.weight"] = torch.rand(c.vocab, cfg.d_model, generator=gen) - 0.5
    sd["ctc.ctc_lo.bias"] = torch.zeros(c.vocab)
    tsd = synthetic_transducer_state_dict(c, 9, blank_bias=5.0)
    sd.update(tsd)
    aed = R.AEDConfig(vocab=c.vocab, d_model=cfg.d_model, heads=2, ff=128, num_blocks=1, r_num_blocks=1)
    dsd = R.synthetic_decoder_state_dict(aed, 3)
    sd.update(dsd)
    m = ChunkFormerModel(cfg, sd, dtype="fp32", model_type="transducer", rnnt_config=c, aed_config=aed)
    return m, synthetic_features([420, 171, 300], 9), (c, tsd, aed, dsd)


def test_from_pretrained_transducer_with_decoder(tmp_path):
    """A `model: transducer` checkpoint directory with decoder.* tensors builds the rescorer; the same directory with a
    decoder the rescorer cannot run (rms_norm) still loads, decodes as a transducer and names the reason when a
    rescoring mode asks for attn_weight > 0."""
    import dataclasses
    import os

    import yaml

    from chunkformer_amd import rescore as R
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.transducer import RNNTConfig, synthetic_transducer_state_dict
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    c = RNNTConfig(vocab=96, enc_dim=SMALL.d_model, embed_size=32, hidden=64, num_layers=1, pred_out=64, join_dim=64)
    cfg = dataclasses.replace(SMALL, vocab=c.vocab, cmvn=False)
    sd = {k: v for k, v in synthetic_state_dict(SMALL, 5).items() if "global_cmvn" not in k}
    gen = torch.Generator().manual_seed(11)
    sd["ctc.ctc_lo.weight"] = torch.rand(c.vocab, cfg.d_model, generator=gen) - 0.5
    sd["ctc.ctc_lo.bias"] = torch.zeros(c.vocab)
    sd.update(synthetic_transducer_state_dict(c, 9, blank_bias=5.0))
    aed = R.AEDConfig(vocab=c.vocab, d_model=cfg.d_model, heads=2, ff=128, num_blocks=1, r_num_blocks=1)
    sd.update(R.synthetic_decoder_state_dict(aed, 3))
    conf = {"encoder": "chunkformer", "input_dim": 80, "output_dim": c.vocab, "model": "transducer",
            "encoder_conf": {"output_size": cfg.d_model, "attention_heads": cfg.n_heads, "linear_units": cfg.ffn_dim,
                             "num_blocks": cfg.num_blocks, "cnn_module_kernel": 15, "cnn_module_norm": "layer_norm",
                             "dynamic_conv": True},
            "predictor": "rnn", "predictor_conf": {"embed_size": 32, "hidden_size": 64, "num_layers": 1,
                                                   "output_size": 64, "rnn_type": "lstm"},
            "joint": "transducer_joint", "joint_conf": {"join_dim": 64, "enc_output_size": cfg.d_model,
                                                        "pred_output_size": 64},
            "decoder": "bitransformer", "decoder_conf": {"attention_heads": 2, "linear_units": 128, "num_blocks": 1,
                                                         "r_num_blocks": 1}}
    torch.save(sd, os.path.join(tmp_path, "pytorch_model.bin"))
    xs = synthetic_features([300], 9)

    def load(**decoder_conf):
        cf = dict(conf, decoder_conf=dict(conf["decoder_conf"], **decoder_conf))
        with open(os.path.join(tmp_path, "config.yaml"), "w") as f:
            yaml.safe_dump(cf, f)
        return ChunkFormerModel.from_pretrained(str(tmp_path), dtype="fp32")
    m = load()
    assert m.model_type == "transducer" and m.rescorer is not None and m._aed_unsupported is None
    greedy = m.batch_decode(xs, 64, 128, 128)
    r = m.batch_decode(xs, 64, 128, 128, decoding_method="rnnt_beam_attn_rescoring", beam_size=3)[0]
    assert len(r.decoder_scores) == len(r.nbest) and any(v != 0.0 for v in r.decoder_scores)
    m2 = load(layer_norm_type="rms_norm")
    assert m2.rescorer is None and "rms_norm" in m2._aed_unsupported
    assert [t.tolist() if hasattr(t, "tolist") else t for t in m2.batch_decode(xs, 64, 128, 128)] == \
        [t.tolist() if hasattr(t, "tolist") else t for t in greedy]
    r0 = m2.batch_decode(xs, 64, 128, 128, decoding_method="rnnt_beam_attn_rescoring", beam_size=3)[0]
    assert r0.decoder_scores == [0.0] * len(r0.nbest)   # attn_weight defaults to 0 without a usable decoder
    with pytest.raises(ValueError, match="rms_norm"):
        m2.batch_decode(xs, 64, 128, 128, decoding_method="rnnt_beam_attn_rescoring", beam_size=3, attn_weight=0.5)


def _rows(m, xs, C, L, R):
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int)
    eo, el, n_chunks, _, _, _ = m.encoder.forward_parallel_chunk(xs, lens, C, L, R, offset=torch.zeros(len(xs), dtype=torch.int))
    starts = (np.cumsum([0] + list(n_chunks[:-1])) * C).tolist()
    el_ctc = [len(range(int(nc) * C)[: int(n)]) for nc, n in zip(n_chunks, el.tolist())]
    return eo.reshape(-1, eo.shape[-1]), starts, [max(0, int(n)) for n in el.tolist()], el_ctc


def test_model_api_equals_the_packed_call_and_the_host(transducer_model):
    from chunkformer_amd import transducer_rescore as TR
    from chunkformer_amd.model import class2str
    from chunkformer_amd.transducer_beam import HostTransducer, RNNTBeamSearch
    from chunkformer_amd.weights import synthetic_vocab
    m, xs, (c, tsd, aed, dsd) = transducer_model
    assert m.rescorer is not None
    C, L, R, K = 64, 128, 128, 4
    rows, starts, el, el_ctc = _rows(m, xs, C, L, R)
    logp, _ = m.encoder.ctc_log_softmax(rows, want_logp=True, want_ids=False)
    tr = TR.TransducerRescorer(m.rnnt, m.rescorer, "fp32")
    beams = RNNTBeamSearch(m.rnnt).search_packed(rows, logp, starts, el, K, 0.3, 0.7)
    want_t = tr.rescore(beams, rows, starts, el, 0.5, 0.5, 0.5, 0.3)
    ctc_beams = m.encoder.ctc_prefix_beam_search(rows, starts, el_ctc, K, None)
    want_c = tr.rescore(ctc_beams, rows, starts, el_ctc, 0.5, 0.5, 0.5, 0.3)
    # the device mode against the host restatement (f64): scores within the fp32 bars, the choice where the host's
    # margin allows
    host = TR.rescore_host(HostTransducer(c, tsd), (aed, dsd), rows.cpu(), starts, el, beams, 0.5, 0.5, 0.5, 0.3)
    for w, h, T in zip(want_t, host, el):
        for a, b, hyp in zip(w.td_scores, h.td_scores, w.nbest):
            assert abs(a - b) <= (T + len(hyp) + 1) * 1e-5
        for a, b, hyp in zip(w.decoder_scores, h.decoder_scores, w.nbest):
            assert abs(a - b) <= (len(hyp) + 1) * 1e-4
        srt = sorted(h.nbest_scores, reverse=True)
        if len(srt) < 2 or srt[0] - srt[1] > 2 * ((T + len(h.tokens) + 1) * 1e-5 + (len(h.tokens) + 1) * 1e-4):
            assert w.best_index == h.best_index and w.tokens == h.tokens
    m.char_dict = None
    kw = dict(beam_size=K, reverse_weight=0.3)
    for method, want in (("rnnt_beam_attn_rescoring", want_t), ("ctc_beam_td_attn_rescoring", want_c)):
        got = m.batch_decode(xs, C, L, R, decoding_method=method, **kw)
        assert [r.tokens for r in got] == [r.tokens for r in want]
        assert [r.nbest_scores for r in got] == [r.nbest_scores for r in want]
        assert [r.td_scores for r in got] == [r.td_scores for r in want]
        assert [r.times for r in got] == [r.times for r in want]
    # other weights reach the search and the combination; attn_weight 0 leaves the decoder out
    w2 = tr.rescore(RNNTBeamSearch(m.rnnt).search_packed(rows, logp, starts, el, K, 0.0, 1.0), rows, starts, el, 0.2,
                    0.0, 0.9)
    got = m.batch_decode(xs, C, L, R, decoding_method="rnnt_beam_attn_rescoring", beam_size=K, ctc_weight=0.2,
                         attn_weight=0.0, transducer_weight=0.9, search_ctc_weight=0.0, search_transducer_weight=1.0)
    assert [r.nbest_scores for r in got] == [r.nbest_scores for r in w2]
    assert all(r.decoder_scores == [0.0] * len(r.nbest) for r in got)
    try:
        m.char_dict = cd = synthetic_vocab(c.vocab)
        assert m.batch_decode(xs, C, L, R, decoding_method="rnnt_beam_attn_rescoring", **kw) == \
            [class2str(r.tokens, cd).strip() for r in want_t]
        m.char_dict = None
        one = m.endless_decode(xs[0], C, L, R, decoding_method="ctc_beam_td_attn_rescoring", **kw)
        assert one.best_index is not None and len(one.td_scores) == len(one.nbest)
    finally:
        m.char_dict = None
