"""The `attention` decoding mode on the GPU (cfm_attdec_*, csrc/attdec.hip; chunkformer_amd/attention_decode.py) against
the reference's recorded searches (tests/golden/attention.npz), the host restatement and, at model level,
batch_decode / endless_decode.

fp32: tokens, trace parents and trace tokens equal in every fixture case; a trace score after i steps within i x 1e-4,
the chosen final score within (steps + 1) x 1e-4 of the fixture's float64 values (the generator admits only cases whose
decision margin is at least twice that).

Seeded batches nothing guarantees a margin for (the packed batch, the model-level runs) are compared step by step up
to the first step whose decision the HOST's own numbers leave open: a step whose gap between the last kept and the
best dropped candidate (host f32) is below 2 i x 1e-4 can legitimately fall either way, and nothing after it is
compared for that utterance.  How many utterances are compared to the end is computed from the host's numbers alone
and printed.

bf16 / fp16: d16 is the fixture's recorded deviation of the reference's own torch.autocast run for that shape and type
(largest |autocast - fp32| over the last-row log-probs of the recorded prefixes), with no extra margin:
  (a) every kept candidate's device score is within i x d16 of the float64 teacher-forced score of its token sequence;
  (b) every candidate the host, started from the device's own beam of step i - 1, ranks in its top N but the device
      dropped lies within 2 i x d16 of the device's N-th kept score;
  tokens equal on exactly the cases whose recorded margin exceeds 2 (steps + 1) x d16.
"""
import dataclasses
import math
import os

import numpy as np
import pytest
import torch
import yaml

import attention_fixture as fx

pytestmark = pytest.mark.gpu

MODELS = ["d128h2", "d256h2", "d64h4", "uni_d64h4"]
BAR = fx.FP32_BAR


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import attention_decode
    return attention_decode


_DECODERS = {}


def _decoder(A, name, recipe, dtype):
    from chunkformer_amd import rescore as R
    key = (name, recipe, dtype)
    if key not in _DECODERS:
        m = fx.load_models()[name]
        _DECODERS[key] = A.AttentionDecoder(R.AttentionRescorer(m["cfg"], m["sds"][recipe], "cuda", dtype))
    return _DECODERS[key]


def _device(A, name, c, dtype):
    return _decoder(A, name, c["recipe"], dtype).search(c["enc"], [0], [c["enc"].shape[0]], c["beam"], c["lp"], c["max_len"],
                                                        return_trace=True)[0]


@pytest.mark.parametrize("name", MODELS)
def test_fp32_matches_the_fixture(A, name):
    m = fx.load_models()[name]
    worst = 0.0
    for k, c in enumerate(m["cases"]):
        worst = max(worst, fx.check_against_fixture(_device(A, name, c, "fp32"), c, BAR))
    print(f"attention fp32 {name}: {len(m['cases'])} cases, worst score error {worst:.3f} of its bar (i x {BAR})")


@pytest.mark.parametrize("name", ["d64h4", "d128h2"])   # head dim 16 (the generic kernels) and 64
def test_search_score_equals_rescoring_of_its_own_hypothesis(A, name):
    """Both consumers of the decoder run the same blocks: where the device's best hypothesis ends with eos, the
    search's un-normalised score of it is the sum of AttentionRescorer.score's left-to-right log-probs of the same
    tokens.  Each side is held to (steps + 1) x BAR of float64 by the tests above, so the two agree within twice that."""
    m = fx.load_models()[name]
    n_cases, worst = 0, 0.0
    for c in m["cases"]:
        dec = _decoder(A, name, c["recipe"], "fp32")
        r = _device(A, name, c, "fp32")
        row = r.beam_rows[r.best_index] if r.steps else []
        if not row or row[-1] != m["cfg"].eos:
            continue
        n_cases += 1
        searched = r.trace[-1][2][r.best_index]
        l2r = dec.rescorer.score(c["enc"], [0], [c["enc"].shape[0]], [[r.tokens]], right=False)[0][0][0]
        rescored = math.fsum(float(v) for v in l2r.tolist())
        bar = 2 * (r.steps + 1) * BAR
        print(f"attention fp32 {name}: steps {r.steps}, search {searched:.6f}, rescoring {rescored:.6f}, "
              f"|difference| {abs(searched - rescored) / bar:.3f} of its bar")
        assert abs(searched - rescored) <= bar, (searched, rescored, bar)
        worst = max(worst, abs(searched - rescored) / bar)
    print(f"attention fp32 {name}: search score vs rescoring on {n_cases} cases, worst {worst:.3f} of "
          f"2 (steps + 1) x {BAR}")
    assert n_cases >= 1, "no fixture case whose best hypothesis ends with eos"


def _compare_until_open(dev, host):
    """-> (steps compared, compared to the end).  Equal parents / tokens and scores within i x BAR up to the first
    step the host's own gap leaves open."""
    for i, gap in enumerate(host.step_margins):
        if gap < 2 * (i + 1) * BAR:
            return i, False
        assert i < len(dev.trace), "the device stopped earlier than the host"
        assert dev.trace[i][0] == host.trace[i][0] and dev.trace[i][1] == host.trace[i][1], f"step {i + 1}"
        for a, b in zip(dev.trace[i][2], host.trace[i][2]):
            assert (a == b) if b == -math.inf else abs(a - b) <= (i + 1) * BAR, (i + 1, a, b)
    assert dev.steps == host.steps
    return host.steps, True


def test_device_equals_host_on_a_packed_batch(A):
    """12 utterances of 0 .. 130 rows, beam 10, one device call: they freeze at different steps."""
    m = fx.load_models()["d128h2"]
    cfg, sd = m["cfg"], m["sds"]["early"]
    rng = np.random.default_rng(7)
    rows = [0, 130, 1, 65] + [int(x) for x in rng.integers(2, 131, 8)]
    starts = np.cumsum([0] + rows[:-1]).tolist()
    enc = torch.from_numpy(rng.integers(-127, 128, (sum(rows), cfg.d_model)).astype(np.float32) / 64.0)
    host = A.attention_beam_search_host(cfg, sd, enc, starts, rows, 10, 0.6)
    dev = _decoder(A, "d128h2", "early", "fp32").search(enc, starts, rows, 10, 0.6, return_trace=True)
    assert len({h.steps for h in host}) >= 4, "the utterances should stop at different steps"
    full = steps = 0
    for b, (d, h) in enumerate(zip(dev, host)):
        n, to_end = _compare_until_open(d, h)
        steps += n
        if to_end:
            full += 1
            assert d.nbest_scores[0] == pytest.approx(h.nbest_scores[0], abs=(h.steps + 1) * BAR, nan_ok=True)
            if h.margin >= 2 * (h.steps + 1) * BAR:
                assert d.tokens == h.tokens
    print(f"attention fp32 packed batch: host steps {[h.steps for h in host]}, {steps} steps compared, "
          f"{full} of 12 utterances to the end")
    assert dev[0].tokens == [] and dev[0].steps == 0 and full >= 1
    # the same utterances one call each: the stop rules do not depend on the batch (the numbers may differ in the
    # last bits: other GEMM tiles and key splits for another row count), so each is held to the host the same way
    for b in (1, 3, 5):
        alone = _decoder(A, "d128h2", "early", "fp32").search(enc[starts[b]: starts[b] + rows[b]], [0], [rows[b]], 10, 0.6,
                                                             return_trace=True)[0]
        assert _compare_until_open(alone, host[b]) == _compare_until_open(dev[b], host[b])
        assert alone.steps == dev[b].steps or not _compare_until_open(dev[b], host[b])[1]


def _trace_consistency(A, m, c, dev, d16):
    """(a) and (b) of the module docstring -> (worst (a) error / its bar, worst (b) gap / its bar)."""
    from chunkformer_amd import rescore as R
    cfg, n = m["cfg"], c["beam"]
    W = {k: v.double() for k, v in R.native_names(cfg, m["sds"][c["recipe"]]).items()}
    hs = A.HostSearch(cfg, W, R.positional_table(cfg.d_model, R.MAX_POSITIONS, torch.float64), c["enc"].double(), n,
                      torch.float64)
    exact = [0.0] + [-math.inf] * (n - 1)         # float64 teacher-forced score of every kept sequence
    dev_scores = list(exact)
    wa = wb = 0.0
    for i, (par, tok, sc) in enumerate(dev.trace, start=1):
        hs.scores = torch.tensor(dev_scores, dtype=torch.float64)
        lp = hs.last_logp(hs.hyps)
        new_exact = []
        for j in range(n):
            p, t = par[j], tok[j]
            new_exact.append(exact[p] if hs.fin[p] else exact[p] + float(lp[p, t]))
            if sc[j] != -math.inf:
                assert abs(sc[j] - new_exact[j]) <= i * d16, ("(a)", i, j, sc[j], new_exact[j])
                wa = max(wa, abs(sc[j] - new_exact[j]) / (i * d16))
        val, ctok, _ = hs.candidates()
        sv, si = torch.sort(val.reshape(-1), descending=True, stable=True)
        kept = {(par[j], tok[j]) for j in range(n) if sc[j] != -math.inf}
        nth = min(s for s in sc if s != -math.inf)
        for v, k in zip(sv[:n].tolist(), si[:n].tolist()):
            cand = (k // n, int(ctok.reshape(-1)[k]))
            if v != -math.inf and cand not in kept:
                assert abs(v - nth) <= 2 * i * d16, ("(b)", i, cand, v, nth)
                wb = max(wb, abs(v - nth) / (2 * i * d16))
        hs.hyps = [hs.hyps[p] + [t] for p, t in zip(par, tok)]
        hs.fin = [t == cfg.eos for t in tok]
        exact, dev_scores = new_exact, list(sc)
    return wa, wb


@pytest.mark.parametrize("dtype, key", [("bf16", "d_bf16"), ("fp16", "d_f16")])
@pytest.mark.parametrize("name", MODELS)
def test_16bit_trace_is_consistent_and_clear_cases_agree(A, name, dtype, key):
    m = fx.load_models()[name]
    d16 = m[key]
    wa = wb = 0.0
    n_tok = 0
    for c in m["cases"]:
        dev = _device(A, name, c, dtype)
        a, b = _trace_consistency(A, m, c, dev, d16)
        wa, wb = max(wa, a), max(wb, b)
        if c["margin"] > 2 * (c["steps"] + 1) * d16:
            n_tok += 1
            assert dev.tokens == c["tokens"], (dev.tokens, c["tokens"])
    print(f"attention {dtype} {name}: d16 {d16:.3e}; (a) worst {wa:.3f} of i x d16, (b) worst {wb:.3f} of 2 i x d16; "
          f"tokens equal on the {n_tok} cases with a margin over 2 (steps + 1) d16")
    if dtype == "fp16":
        assert n_tok >= 3


def test_bad_ranges_raise_and_spare_the_rest(A):
    m = fx.load_models()["d64h4"]
    dec = _decoder(A, "d64h4", "mid", "fp32")
    a, b = m["cases"][5]["enc"], m["cases"][7]["enc"]        # 15 and 16 rows
    enc, starts, rows = torch.cat([a, b]), [0, a.shape[0]], [a.shape[0], b.shape[0]]
    good = dec.search(enc, starts, rows, 3, return_trace=True)
    bad_rows = [rows[0], rows[1] + 1]                        # the last utterance runs past the encoder rows
    with pytest.raises(ValueError, match="row ranges"):
        dec.search(enc, starts, bad_rows, 3)                 # the host check
    with pytest.raises(ValueError, match="status 2"):
        dec.search(enc, starts, bad_rows, 3, return_trace=True, check_host=False)      # the device's status word
    spared, skipped = dec.last_results
    assert spared.trace == good[0].trace and spared.tokens == good[0].tokens       # the others as without it
    assert skipped.steps == 0 and skipped.tokens == []                              # the rejected one never stepped
    with pytest.raises(ValueError, match="beam_size"):
        dec.search(enc, starts, rows, 17)
    with pytest.raises(ValueError, match="max_len"):
        dec.search(torch.zeros(5001, m["cfg"].d_model), [0], [5001], 2)


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
def small_model(A, tmp_path_factory):
    from chunkformer_amd import rescore as R
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.weights import synthetic_state_dict
    cfg = dataclasses.replace(SMALL, cmvn=False)
    aed = R.AEDConfig(vocab=cfg.vocab, d_model=cfg.d_model, heads=2, ff=256, num_blocks=2, r_num_blocks=2,
                      ctc_weight=0.3, reverse_weight=0.3)
    sd = dict(synthetic_state_dict(cfg, 1))
    sd.update(A.sharpened_decoder_state_dict(aed, 3, 6.0, 1.0))
    root = tmp_path_factory.mktemp("attdec_ckpt")
    _write_small_checkpoint(str(root / "with"), sd, cfg, True)
    _write_small_checkpoint(str(root / "without"), sd, cfg, False)
    return (ChunkFormerModel.from_pretrained(str(root / "with"), dtype="fp32"),
            ChunkFormerModel.from_pretrained(str(root / "without"), dtype="fp32"), aed, sd)


def test_batch_decode_attention_picks_what_the_host_picks(A, small_model):
    from chunkformer_amd.weights import synthetic_features
    m, plain, aed, sd = small_model
    C, L, Rc = 16, 32, 16
    xs = synthetic_features([611, 97, 350], 31)
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int)
    eo, el, n_chunks, _, _, _ = m.encoder.forward_parallel_chunk(xs, lens, C, L, Rc, offset=torch.zeros(3, dtype=torch.int))
    starts = (np.cumsum([0] + list(n_chunks[:-1])) * C).tolist()
    rl = [int(n) for n in el.tolist()]
    rows = eo.reshape(-1, eo.shape[-1]).clone().cpu()
    for kw in (dict(beam_size=3, max_len=12), dict(beam_size=2, length_penalty=0.6, max_len=20)):
        got = m.batch_decode(xs, C, L, Rc, decoding_method="attention", **kw)
        exp = A.attention_beam_search_host(aed, sd, rows, starts, rl, kw["beam_size"], kw.get("length_penalty", 0.0),
                                           kw["max_len"])
        dev = m._attention_search().search(rows, starts, rl, kw["beam_size"], kw.get("length_penalty", 0.0), kw["max_len"],
                                           return_trace=True)
        for g, d, e in zip(got, dev, exp):
            assert g.tokens == d.tokens and g.nbest == d.nbest
            n, to_end = _compare_until_open(d, e)
            assert n >= 1
            if to_end and e.margin >= 2 * (e.steps + 1) * BAR:
                assert g.tokens == e.tokens and abs(g.score - e.score) <= (e.steps + 1) * BAR
    assert m._attention_search().rescorer is m.rescorer          # one handle, one copy of the weights
    with pytest.raises(ValueError, match="decoder"):
        plain.batch_decode(xs, C, L, Rc, decoding_method="attention")
    with pytest.raises(ValueError, match="decoder"):
        plain.endless_decode(xs[0], C, L, Rc, decoding_method="attention")
    for a, b in zip(m.batch_decode(xs, C, L, Rc), plain.batch_decode(xs, C, L, Rc)):      # the default is untouched
        assert torch.equal(a, b)


def test_endless_decode_attention_picks_what_the_host_picks(A, small_model):
    from chunkformer_amd.weights import synthetic_features
    m, plain, aed, sd = small_model
    C, L, Rc, tbd = 16, 32, 16, 20
    x = synthetic_features([3000], 47)[0]
    got, eo = m.endless_decode(x, C, L, Rc, total_batch_duration=tbd, return_encoder_out=True, decoding_method="attention",
                               beam_size=3, max_len=16)
    n = eo.shape[1]
    exp = A.attention_beam_search_host(aed, sd, eo[0].cpu(), [0], [n], 3, 0.0, 16)[0]
    dev = m._attention_search().search(eo[0], [0], [n], 3, 0.0, 16, return_trace=True)[0]
    assert got.tokens == dev.tokens and got.score == dev.score
    k, to_end = _compare_until_open(dev, exp)
    assert k >= 1
    if to_end and exp.margin >= 2 * (exp.steps + 1) * BAR:
        assert got.tokens == exp.tokens and abs(got.score - exp.score) <= (exp.steps + 1) * BAR
