"""Attention rescoring on the GPU (cfm_aed_score, csrc/aed.hip; chunkformer_amd/rescore.py) against the reference's
recorded results (tests/golden/rescore.npz), the host restatement and, at model level, batch_decode / endless_decode.

fp32 bars: per-token log-probs 1e-4 (the project's fp32 bar on log-probs, test_gpu_parity.py); totals (n + 1) x 1e-4;
confidences exp(total / (n + 1)) and token confidences exp(logp): the same bounds through exp (a relative 1e-4, plus
1e-6 for the reference's own f32 exp); chosen index equal in every case and weight combination.

bf16 / fp16: the yardstick is the reference's own torch.autocast deviation stored in the fixture, per decoder shape:
max and rms over every token row of |autocast - fp32|.  Our deviation from the reference's fp32 values must not
exceed it, in max and in rms, with no extra margin; chosen index equal in every case (the fixture's margins are
twice the largest total deviation these bars allow, gen_golden_rescore.py).

Measured on an MI355X (ours / the reference's autocast, max and rms over the shape's token rows):
    d128h2 (head dim 64, MFMA)      bf16 1.82e-2 / 5.03e-2, 4.85e-3 / 1.22e-2    fp16 2.65e-3 / 6.00e-3, 6.11e-4 / 1.52e-3
    d256h2 (head dim 128, MFMA)     bf16 1.75e-2 / 4.56e-2, 4.57e-3 / 1.19e-2    fp16 2.48e-3 / 5.88e-3, 6.20e-4 / 1.49e-3
    d64h4 (head dim 16, generic)    bf16 2.33e-2 / 4.67e-2, 5.19e-3 / 1.17e-2    fp16 2.53e-3 / 6.18e-3, 6.18e-4 / 1.47e-3
    uni_d64h4 (decoder: transformer) bf16 1.52e-2 / 4.17e-2, 5.04e-3 / 1.26e-2   fp16 2.14e-3 / 5.85e-3, 6.75e-4 / 1.70e-3
i.e. 0.36 .. 0.50 of the yardstick; fp32: 3.8e-6 at most.
"""
import dataclasses
import os

import numpy as np
import pytest
import torch
import yaml

import rescore_fixture as fx

pytestmark = pytest.mark.gpu

MODELS = ["d128h2", "d256h2", "d64h4", "uni_d64h4"]
FP32_TOKEN_BAR = 1e-4


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import rescore
    return rescore


def _device_scores(R, name, dtype):
    m = fx.load_models()[name]
    enc, starts, rows, res = fx.packed(m["utts"])
    r = R.AttentionRescorer(m["cfg"], m["sd"], "cuda", dtype)
    return m, r.score(enc, starts, rows, [u["hyps"] for u in m["utts"]])


def _check_choices(R, m, scored, token_bar=None):
    enc, starts, rows, res = fx.packed(m["utts"])
    for k, (rw, cw) in enumerate(m["combos"]):
        for u, r in zip(m["utts"], R.combine(m["cfg"], scored, res, cw, rw)):
            idx, total, conf = int(u["exp"][k][0]), float(u["exp"][k][1]), float(u["exp"][k][2])
            assert r.best_index == idx and r.tokens == u["hyps"][idx] and r.times == u["times"][idx], (k, idx)
            if token_bar is not None:
                n = len(u["hyps"][idx])
                assert abs(r.score - total) <= (n + 1) * token_bar, (r.score, total)
                assert abs(r.confidence - conf) <= conf * (token_bar + 1e-6)
                for a, b in zip(r.tokens_confidence, u["tcs"][k]):
                    assert abs(a - b) <= b * (token_bar + 1e-6)


@pytest.mark.parametrize("name", MODELS)
def test_fp32_matches_reference(R, name):
    m, scored = _device_scores(R, name, "fp32")
    err = fx.token_errors(scored, m["utts"])
    print(f"rescore fp32 {name}: {err.size} token rows, max |device - reference| = {err.max():.2e}")
    assert err.max() <= FP32_TOKEN_BAR
    _check_choices(R, m, scored, FP32_TOKEN_BAR)


@pytest.mark.parametrize("dtype, suffix", [("bf16", "bf16"), ("fp16", "f16")])
@pytest.mark.parametrize("name", MODELS)
def test_16bit_within_the_references_own_deviation(R, name, dtype, suffix):
    m, scored = _device_scores(R, name, dtype)
    ours = fx.token_errors(scored, m["utts"])
    ref = fx.reference_deviation(m["utts"], suffix)
    assert ours.size == ref.size
    o_max, o_rms = ours.max(), float(np.sqrt(np.mean(ours ** 2)))
    r_max, r_rms = ref.max(), float(np.sqrt(np.mean(ref ** 2)))
    print(f"rescore {dtype} {name}: max {o_max:.3e} (reference's autocast {r_max:.3e}, ratio {o_max / r_max:.2f}), "
          f"rms {o_rms:.3e} ({r_rms:.3e}, ratio {o_rms / r_rms:.2f})")
    assert o_max <= r_max and o_rms <= r_rms
    _check_choices(R, m, scored)


def _seeded_batch(cfg, seed=5):
    """12 utterances of 1 .. 300 rows, up to 10 hypotheses of up to 80 tokens: nothing the fixture holds."""
    rng = np.random.default_rng(seed)
    rows = [1, 300] + [int(x) for x in rng.integers(1, 301, 10)]
    starts = np.cumsum([0] + rows[:-1]).tolist()
    enc = torch.from_numpy(rng.standard_normal((sum(rows), cfg.d_model)).astype(np.float32))
    nbest = []
    for b in range(12):
        n_h = 10 if b == 0 else int(rng.integers(1, 11))
        lens = [80, 0] if b == 0 else []
        lens += [int(x) for x in rng.integers(0, 81, n_h - len(lens))]
        nbest.append([[int(t) for t in rng.integers(0, cfg.vocab, n)] for n in lens])
    return enc, starts, rows, nbest


def test_device_equals_host_restatement(R):
    m = fx.load_models()["d128h2"]
    cfg = m["cfg"]
    enc, starts, rows, nbest = _seeded_batch(cfg)
    host = R.score_host(cfg, m["sd"], enc, starts, rows, nbest)
    r = R.AttentionRescorer(cfg, m["sd"], "cuda", "fp32")
    dev = r.score(enc, starts, rows, nbest)
    worst = 0.0
    for hb, db in zip(host, dev):
        for (hl, hr), (dl, dr) in zip(hb, db):
            assert hl.shape == dl.shape and hr.shape == dr.shape
            worst = max(worst, float((hl - dl).abs().max()), float((hr - dr).abs().max()))
            assert abs(float(hl.double().sum() - dl.double().sum())) <= hl.numel() * FP32_TOKEN_BAR
    print(f"rescore fp32 device vs host: max |diff| = {worst:.2e} over {sum(len(x) for x in nbest)} hypotheses")
    assert worst <= FP32_TOKEN_BAR
    # the left decoder alone gives the same left-to-right scores, and no right-to-left ones
    only = r.score(enc, starts, rows, nbest, right=False)
    assert all(b[1] is None and torch.equal(a[0], b[0]) for x, y in zip(dev, only) for a, b in zip(x, y))


def test_bad_token_and_bad_range_raise_and_spare_the_rest(R):
    m = fx.load_models()["d64h4"]
    cfg = m["cfg"]
    utts = m["utts"][:5]
    enc, starts, rows, res = fx.packed(utts)
    nbest = [[list(h) for h in u["hyps"]] for u in utts]
    r = R.AttentionRescorer(cfg, m["sd"], "cuda", "fp32")
    good = r.score(enc, starts, rows, nbest)
    ub = next(b for b, hyps in enumerate(nbest) if any(len(h) > 2 for h in hyps))
    hb = next(i for i, h in enumerate(nbest[ub]) if len(h) > 2)
    bad = [[list(h) for h in hyps] for hyps in nbest]
    bad[ub][hb][1] = cfg.vocab                                    # a token id outside [0, V)
    with pytest.raises(ValueError):
        r.score(enc, starts, rows, bad)                           # the host check
    with pytest.raises(ValueError, match="status 3"):
        r.score(enc, starts, rows, bad, check_host=False)         # the device's status word
    for b, (gb, sb) in enumerate(zip(good, r.last_scores)):
        for i, ((gl, gr), (sl, sr)) in enumerate(zip(gb, sb)):
            if (b, i) == (ub, hb):
                assert (sl == 0).all() and (sr == 0).all()        # skipped: its rows are untouched
            else:
                assert torch.allclose(gl, sl, atol=1e-6, rtol=0) and torch.allclose(gr, sr, atol=1e-6, rtol=0)
    bad_rows = list(rows)
    bad_rows[-1] += 1                                             # the last utterance runs past the encoder rows
    with pytest.raises(ValueError):
        r.score(enc, starts, bad_rows, nbest)
    with pytest.raises(ValueError, match="status 2"):
        r.score(enc, starts, bad_rows, nbest, check_host=False)
    for b, (gb, sb) in enumerate(zip(good, r.last_scores)):
        for (gl, gr), (sl, sr) in zip(gb, sb):
            if b == len(rows) - 1:
                assert (sl == 0).all() and (sr == 0).all()
            else:
                assert torch.allclose(gl, sl, atol=1e-6, rtol=0) and torch.allclose(gr, sr, atol=1e-6, rtol=0)
    with pytest.raises(ValueError):
        r.score(enc, starts, rows, [[[1] * R.MAX_POSITIONS]] + nbest[1:])


# ------------------------------------------------------------------------------------ model level
def _write_small_checkpoint(path, sd, cfg, decoder: bool):
    conf = {"encoder": "chunkformer", "input_dim": 80, "output_dim": cfg.vocab, "model": "asr_model",
            "encoder_conf": {"output_size": cfg.d_model, "attention_heads": cfg.n_heads, "linear_units": cfg.ffn_dim,
                             "num_blocks": cfg.num_blocks, "input_layer": "dw_striding", "cnn_module_kernel": 15,
                             "pos_enc_layer_type": "chunk_rel_pos", "selfattention_layer_type": "chunk_rel_seflattn",
                             "cnn_module_norm": "layer_norm", "dynamic_conv": True, "activation_type": "swish"},
            "ctc_conf": {"ctc_blank_id": 0}, "decoder": "bitransformer",
            "decoder_conf": {"attention_heads": 2, "linear_units": 256, "num_blocks": 2, "r_num_blocks": 2,
                             "dropout_rate": 0.1},
            "model_conf": {"ctc_weight": 0.3, "reverse_weight": 0.3}}
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.yaml"), "w") as f:
        yaml.safe_dump(conf, f)
    ckpt = {k: v for k, v in sd.items() if "global_cmvn" not in k and (decoder or not k.startswith("decoder."))}
    torch.save(ckpt, os.path.join(path, "pytorch_model.bin"))


@pytest.fixture(scope="module")
def small_models(R, tmp_path_factory):
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.weights import synthetic_state_dict
    cfg = dataclasses.replace(SMALL, cmvn=False)
    aed = R.AEDConfig(vocab=cfg.vocab, d_model=cfg.d_model, heads=2, ff=256, num_blocks=2, r_num_blocks=2,
                      ctc_weight=0.3, reverse_weight=0.3)
    sd = dict(synthetic_state_dict(cfg, 1))
    sd.update(R.synthetic_decoder_state_dict(aed, 3))
    sd["decoder.left_decoder.embed.1.pe"] = torch.zeros(1, 5000, cfg.d_model)   # a checkpoint carries the buffers
    sd["decoder.right_decoder.embed.1.pe"] = torch.zeros(1, 5000, cfg.d_model)
    root = tmp_path_factory.mktemp("aed_ckpt")
    _write_small_checkpoint(str(root / "with"), sd, cfg, True)
    _write_small_checkpoint(str(root / "without"), sd, cfg, False)
    with_dec = ChunkFormerModel.from_pretrained(str(root / "with"), dtype="fp32")
    without = ChunkFormerModel.from_pretrained(str(root / "without"), dtype="fp32")
    return with_dec, without, aed, sd


def test_batch_decode_rescoring_picks_what_the_host_picks(R, small_models):
    from chunkformer_amd.weights import synthetic_features
    m, plain, aed, sd = small_models
    assert m.rescorer is not None and plain.rescorer is None
    assert dataclasses.asdict(m.rescorer.cfg) == dataclasses.asdict(aed)
    C, L, Rc, k = 16, 32, 16, 5
    xs = synthetic_features([611, 97, 350, 1203], 31)
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int)
    eo, el, n_chunks, _, _, _ = m.encoder.forward_parallel_chunk(xs, lens, C, L, Rc, offset=torch.zeros(4, dtype=torch.int))
    starts = (np.cumsum([0] + list(n_chunks[:-1])) * C).tolist()
    rl = [int(n) for n in el.tolist()]
    rows = eo.reshape(-1, eo.shape[-1]).clone()
    beam = m.batch_decode(xs, C, L, Rc, decoding_method="ctc_prefix_beam_search", beam_size=k)
    assert any(len(b.nbest) > 1 for b in beam)
    for kw in ({}, {"ctc_weight": 0.0, "reverse_weight": 0.0}, {"ctc_weight": 1.5, "reverse_weight": 0.5}):
        got = m.batch_decode(xs, C, L, Rc, decoding_method="attention_rescoring", beam_size=k, **kw)
        exp = R.rescore_host(aed, sd, rows.cpu(), starts, rl, beam, **kw)
        for g, e in zip(got, exp):
            n = len(e.tokens)
            assert g.tokens == e.tokens and g.times == e.times and g.best_index == e.best_index
            assert abs(g.score - e.score) <= (n + 1) * FP32_TOKEN_BAR
            assert abs(g.confidence - e.confidence) <= e.confidence * (FP32_TOKEN_BAR + 1e-6)
            assert len(g.tokens_confidence) == n
    ranked = m.batch_decode(xs, C, L, Rc, decoding_method="attention_rescoring", beam_size=k, return_nbest=True)
    for r_, b in zip(ranked, beam):
        assert r_.nbest[0] == r_.tokens and sorted(r_.nbest) == sorted(b.nbest)
        assert all(a >= c for a, c in zip(r_.nbest_scores, r_.nbest_scores[1:]))
    # the two existing methods: exactly what the same checkpoint without its decoder tensors returns
    for a, b in zip(m.batch_decode(xs, C, L, Rc), plain.batch_decode(xs, C, L, Rc)):
        assert torch.equal(a, b)
    for a, b in zip(beam, plain.batch_decode(xs, C, L, Rc, decoding_method="ctc_prefix_beam_search", beam_size=k)):
        assert a.nbest == b.nbest and a.nbest_scores == b.nbest_scores and a.nbest_times == b.nbest_times
    with pytest.raises(ValueError, match="decoder"):
        plain.batch_decode(xs, C, L, Rc, decoding_method="attention_rescoring")
    with pytest.raises(ValueError, match="decoder"):
        plain.endless_decode(xs[0], C, L, Rc, decoding_method="attention_rescoring")


def test_endless_decode_rescoring_picks_what_the_host_picks(R, small_models):
    from chunkformer_amd.model import endless_segments
    from chunkformer_amd.weights import synthetic_features
    m, plain, aed, sd = small_models
    C, L, Rc, k, tbd, T = 16, 32, 16, 6, 20, 3000
    assert len(endless_segments(T, C, L, Rc, tbd, m.config.num_blocks, m.config.kernel_size)[1]) >= 3
    x = synthetic_features([T], 47)[0]
    beam, eo = m.endless_decode(x, C, L, Rc, total_batch_duration=tbd, return_encoder_out=True,
                                decoding_method="ctc_prefix_beam_search", beam_size=k)
    got = m.endless_decode(x, C, L, Rc, total_batch_duration=tbd, decoding_method="attention_rescoring", beam_size=k)
    n = eo.shape[1]
    exp = R.rescore_host(aed, sd, eo[0].cpu(), [0], [n], [beam])[0]
    assert got.tokens == exp.tokens and got.times == exp.times and got.best_index == exp.best_index
    assert abs(got.score - exp.score) <= (len(exp.tokens) + 1) * FP32_TOKEN_BAR
    ids = m.endless_decode(x, C, L, Rc, total_batch_duration=tbd)
    assert torch.equal(ids, plain.endless_decode(x, C, L, Rc, total_batch_duration=tbd))
    pb = plain.endless_decode(x, C, L, Rc, total_batch_duration=tbd, decoding_method="ctc_prefix_beam_search", beam_size=k)
    assert pb.nbest == beam.nbest and pb.nbest_scores == beam.nbest_scores


def test_unsupported_decoder_settings_raise_at_load(R, small_models, tmp_path):
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.model import ChunkFormerModel
    _, _, aed, sd = small_models
    cfg = dataclasses.replace(SMALL, cmvn=False)
    _write_small_checkpoint(str(tmp_path), sd, cfg, True)
    p = os.path.join(str(tmp_path), "config.yaml")
    with open(p) as f:
        conf = yaml.safe_load(f)
    conf["decoder_conf"]["activation_type"] = "gelu"
    with open(p, "w") as f:
        yaml.safe_dump(conf, f)
    with pytest.raises(AssertionError):
        ChunkFormerModel.from_pretrained(str(tmp_path), dtype="fp32")
