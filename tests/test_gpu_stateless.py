"""GPU: the stateless transducer predictors (embedding, conv) on the device -- the predictor op, the greedy
kernel, the prefix beam search, the full-sum score and the model API -- against the reference's recorded results
(tests/golden/rnnt_stateless.npz) and the host restatements.

Bars: the predictor output within 4 e_ref of the f64 restatement, e_ref the reference's own f32 forward_step error on
the same windows (stored in the fixture; the device sums the heads first and splits K in its products, so its
rounding differs from torch's but is of the same order); greedy decisions and token-equality beams identical; the
device's fused log-probs within DEV = 1e-5 of the restatement's for the same prefix; per lattice node 1e-5 (the bar the
LSTM handle's test holds this joint to), per td (T + U + 1) 1e-5; bf16 twice the deviations measured for the LSTM
handle's bf16 kernel (tests/test_gpu_td_rescore.py).

Measured on an MI355X (the tests print them): predictor output 0.54 .. 1.66 e_ref over the eight models; fused
log-probs at most 4.8e-6 from the restatement's; lattice nodes at most 1.8e-6; bf16 8.2e-3 per node, 2.0e-2 per td."""
import functools
import os

import numpy as np
import pytest
import torch

import stateless_fixture as fx

pytestmark = pytest.mark.gpu

DEV = 1e-5


@functools.lru_cache(maxsize=None)
def device_model(name):
    from chunkformer_amd.transducer import RNNTGreedy
    from chunkformer_amd.transducer_beam import RNNTBeamSearch
    cfg, sd = fx.model(name)
    return RNNTBeamSearch(RNNTGreedy(cfg, sd, "cuda:0"))


# ----------------------------------------------------------------------------- the predictor op
@pytest.mark.parametrize("name", fx.names())
def test_predictor_step_vs_f64(name):
    dev, host = device_model(name), fx.host_model(name)
    cfg = host.cfg
    win, _, e_ref = fx.predictor_points(name)
    y, pj = dev.predictor_step(win)
    y64 = host.predict_windows(win, torch.float64)
    err = float((y.cpu().double() - y64).abs().max())
    print(f"{name}: max |device - f64| = {err:.3e}, e_ref = {e_ref:.3e}, ratio {err / e_ref:.2f}")
    assert err <= 4 * e_ref
    # pred_ffn of it: the output's bar through the rows of the weight, plus the f32 rounding of an (E + 1)-term sum
    W, b = host.sd["joint.pred_ffn.weight"].double(), host.sd["joint.pred_ffn.bias"].double()
    pj64 = y64 @ W.t() + b
    mag = (y64.abs() @ W.abs().t() + b.abs()).max()
    bar = 4 * e_ref * float(W.abs().sum(1).max()) + 2.0 ** -23 * (cfg.embed_size + 1) * float(mag)
    perr = float((pj.cpu().double() - pj64).abs().max())
    print(f"{name}: pred_ffn max |device - f64| = {perr:.3e} (bar {bar:.3e})")
    assert perr <= bar
    # one window alone gives the same row as in the batch
    y1, pj1 = dev.predictor_step(win[3:4])
    assert torch.equal(y1[0], y[3]) and torch.equal(pj1[0], pj[3])


def test_predictor_step_needs_a_stateless_handle():
    from rnnt_beam_fixture import model
    from chunkformer_amd.transducer import RNNTGreedy
    from chunkformer_amd.transducer_beam import RNNTBeamSearch
    cfg, sd = model("v37", "dense")
    lstm = RNNTBeamSearch(RNNTGreedy(cfg, sd, "cuda:0"))
    with pytest.raises(ValueError):
        lstm.predictor_step([[1] * lstm.cfg.context])
    dev = device_model("conv_v37")
    with pytest.raises(ValueError):
        dev.lstm_step(torch.zeros(1, dtype=torch.int32), torch.zeros(0, 1, 0), torch.zeros(0, 1, 0))


# ----------------------------------------------------------------------------- greedy
@pytest.mark.parametrize("name", fx.names())
def test_greedy_equals_the_recorded_decisions(name):
    dev = device_model(name).rnnt
    assert dev.grid_blocks(1) == 0 and dev.grid_blocks(3) == 0
    dev.set_option("grid_blocks", 16)   # accepted, no effect
    assert dev.grid_blocks(1) == 0
    for c in fx.greedy_cases(name):
        out = dev.greedy_packed(c["enc"].cuda(), c["starts"], c["lens"], c["n_steps"]).cpu().numpy()
        np.testing.assert_array_equal(out, c["dense"], err_msg=str((name, c["lens"], c["n_steps"])))
        hyps = dev.batch_greedy_search(c["enc"][: c["lens"][0]].unsqueeze(0).cuda(), torch.tensor([c["lens"][0]]),
                                       c["n_steps"])
        assert hyps == [c["ref_tokens"][0]]


def test_lstm_handle_beside_stateless_handles(golden_dir):
    """An rnn handle created and searched in the process that ran the stateless ones still returns its recorded
    decisions on the one-workgroup kernel (the joint block is shared code)."""
    from chunkformer_amd.transducer import RNNTConfig, RNNTGreedy, synthetic_transducer_state_dict
    c0 = fx.greedy_cases("emb_v37")[0]
    sl = device_model("emb_v37").rnnt
    np.testing.assert_array_equal(sl.greedy_packed(c0["enc"].cuda(), c0["starts"], c0["lens"], 4).cpu().numpy(), c0["dense"])
    g = np.load(os.path.join(golden_dir, "rnnt_sparse.npz"))
    c = RNNTConfig(vocab=int(g["vocab"]))
    sd = synthetic_transducer_state_dict(c, int(g["seed"]), blank_bias=float(g["blank_bias"]), enc_scale=float(g["enc_scale"]))
    dec = RNNTGreedy(c, sd, "cuda")
    dec.set_option("grid_blocks", 0)
    ge = np.load(os.path.join(golden_dir, "large_endless.npz"))
    T = g["endless_out_steps3"].shape[1] // 3
    out = dec.optimized_search(torch.from_numpy(ge["out"][:T]).unsqueeze(0).cuda(), torch.tensor([T]), 3)
    np.testing.assert_array_equal(out.cpu().numpy(), g["endless_out_steps3"])
    np.testing.assert_array_equal(sl.greedy_packed(c0["enc"].cuda(), c0["starts"], c0["lens"], 4).cpu().numpy(), c0["dense"])


# ----------------------------------------------------------------------------- beam search
@functools.lru_cache(maxsize=None)
def beam_results(name):
    dev = device_model(name)
    out = []
    for c in fx.beam_cases(name):
        r = dev.search_packed(c["enc"].cuda(), c["ctc"].cuda() if c["cw"] > 0 else None, [0], [c["rows"]], c["beam"], c["cw"],
                              c["tw"], return_trace=True)[0]
        assert dev.last_error == 0
        out.append((c, r))
    return out


@pytest.mark.parametrize("name", fx.names())
def test_beam_equality_cases(name):
    """Tokens, scores, n-best and the frame at which each token was appended, against the reference's recorded beam
    and (the times: the reference records none) the host restatement of the same search."""
    from chunkformer_amd import transducer_beam as TB
    n = 0
    for c, r in beam_results(name):
        if not c["equality"]:
            continue
        n += 1
        what = (name, c["rows"], c["beam"], c["cw"], c["tw"])
        assert r.nbest == c["tokens"], what
        np.testing.assert_allclose(r.nbest_scores, c["scores"], rtol=0, atol=1e-4, err_msg=str(what))
        assert r.tokens == c["tokens"][0] and r.score == r.nbest_scores[0]
        host_res = TB.prefix_beam_search_host(fx.host_model(name), c["enc"], c["ctc"], [0], [c["rows"]], c["beam"], c["cw"],
                                              c["tw"])[0]
        assert r.nbest_times == host_res.nbest_times and r.times == host_res.times, what
        assert all(len(t) == len(h) and all(a < b for a, b in zip(t, t[1:])) and all(0 <= a < c["rows"] for a in t)
                   for t, h in zip(r.nbest_times, r.nbest)), what
    assert n >= 7


@pytest.mark.parametrize("name", fx.names())
def test_beam_trace_is_consistent(name):
    """Along the device's own trace, every case: each frame's kept beam is what beam_step_host makes of the device's
    previous beam and top-K values, and the top-K values are within DEV of the restatement's log-probs for that
    prefix (the id windows follow the device's parents)."""
    from chunkformer_amd import transducer_beam as TB
    host = fx.host_model(name)
    cfg = host.cfg
    worst = 0.0
    for c, r in beam_results(name):
        K, tr = c["beam"], r.trace
        what = (name, c["rows"], K, c["cw"], c["tw"])
        hyps, scores, times = [()], [0.0], [()]
        for t in range(c["rows"]):
            n = len(hyps)
            topv, topi = tr["topv"][t, :n], tr["topi"][t, :n]
            wins = [tuple(w) for w in np.stack([TB.hyp_windows(cfg, hy)[-1] for hy in hyps]).tolist()]
            pred = host.step_windows(wins)
            fused = TB.fuse_host(host.log_probs(c["enc"][t], pred), c["ctc"][t] if c["cw"] > 0 else None, c["cw"], c["tw"])
            assert ((topi >= 0) & (topi < cfg.vocab)).all(), what
            worst = max(worst, float(np.abs(np.take_along_axis(fused.numpy(), topi.astype(np.int64), 1) - topv).max()))
            kept, gap = TB.beam_step_host(hyps, scores, topv, topi, K, cfg.blank)
            dpar, dtok, dsc = tr["parent"][t], tr["token"][t], tr["score"][t]
            m = int((dpar >= 0).sum())
            assert m == len(kept) and (dpar[:m] < n).all(), (what, t)
            if gap >= 1e-9:
                assert dpar[:m].tolist() == [k[2] for k in kept] and dtok[:m].tolist() == [k[3] for k in kept], (what, t)
                np.testing.assert_allclose(dsc[:m], [k[1] for k in kept], rtol=1e-12, atol=0, err_msg=str((what, t)))
            times = [times[p] + (t,) if u != cfg.blank else times[p] for p, u in zip(dpar[:m], dtok[:m])]
            hyps = [hyps[p] + (int(u),) if u != cfg.blank else hyps[p] for p, u in zip(dpar[:m], dtok[:m])]
            scores = dsc[:m].tolist()
        assert r.nbest == [list(x) for x in hyps] and r.nbest_scores == scores, what
        assert r.nbest_times == [list(x) for x in times], what
    print(f"{name}: largest deviation of the device's fused log-probs from the restatement's: {worst:.3e}")
    assert worst <= DEV


def test_beam_ragged_batch_and_workspace():
    from chunkformer_amd import _lib
    from rnnt_beam_fixture import model
    from chunkformer_amd.transducer import RNNTGreedy
    dev = device_model("emb_v130")
    cfg = dev.cfg
    lens = [0, 1, 7, 33, 2]
    g = np.random.default_rng(7)
    rows = sum(lens)
    enc = torch.from_numpy(g.integers(-128, 128, size=(rows, cfg.enc_dim)).astype(np.float32) / 64.0).cuda()
    starts = np.cumsum([0] + lens[:-1]).tolist()
    batch = dev.search_packed(enc, None, starts, lens, 5, 0.0, 1.0)
    assert dev.last_error == 0
    for s, n, rb in zip(starts, lens, batch):
        alone = dev.search_packed(enc[s: s + n], None, [0], [n], 5, 0.0, 1.0)[0]
        assert rb.nbest == alone.nbest and rb.nbest_scores == alone.nbest_scores and rb.nbest_times == alone.nbest_times
    assert batch[0].nbest == [[]] and batch[0].score == 0.0
    # the state of a slot is a few ids: the workspace is smaller than an LSTM handle's of the same widths
    lcfg, lsd = model("v130", "dense")
    lstm = RNNTGreedy(lcfg, lsd, "cuda:0")
    a = int(_lib.cfm_rnnt_beam_workspace_bytes(dev.rnnt._h, 65, 4, 16))
    b = int(_lib.cfm_rnnt_beam_workspace_bytes(lstm._h, 65, 4, 16))
    assert 0 < a < b


# ----------------------------------------------------------------------------- the full-sum score
@functools.lru_cache(maxsize=None)
def rescorer(name, dtype="fp32"):
    from chunkformer_amd.transducer_rescore import TransducerRescorer
    return TransducerRescorer(device_model(name).rnnt, None, dtype)


def _node_case(name, dtype):
    """Per-node (b, k) of the td case's hypotheses from the DEVICE's predictor_step projections through the lattice
    kernel, beside the f64 restatement."""
    from chunkformer_amd import transducer_beam as TB
    from chunkformer_amd import transducer_rescore as TR
    host, dev = fx.host_model(name), device_model(name)
    c = fx.td_cases(name)[1]
    e = TR.joint_projections_host(host, c["enc"], [])[0]
    wins = np.concatenate([TB.hyp_windows(host.cfg, h) for h in c["hyps"]])
    _, q = dev.predictor_step(wins)
    got = rescorer(name).lattice(e.float(), q, [0], [c["rows"]], [(0, h) for h in c["hyps"]], dtype)
    want = [TR.lattice_logp_host(host, c["enc"], h) for h in c["hyps"]]
    worst = 0.0
    for (gb, gk), (wb, wk) in zip(got, want):
        assert gb.shape == wb.shape and np.isfinite(gb).all() and np.isfinite(gk).all()
        worst = max(worst, float(np.abs(gb - wb).max()), float(np.abs(gk - wk).max()) if gk.size else 0.0)
    return worst


@pytest.mark.parametrize("name", fx.names())
def test_td_fp32(name):
    tr = rescorer(name)
    node = _node_case(name, "fp32")
    print(f"{name}: max |device - f64| per node = {node:.3e}")
    assert node <= 1e-5
    # hypotheses of 0, 1, K - 1, K, K + 1 tokens packed back to back in one call: a window never reaches into the
    # previous hypothesis' tokens
    for c in fx.td_cases(name):
        td = tr.td_scores(c["enc"], [0], [c["rows"]], [c["hyps"]])[0]
        assert tr.last_error == 0
        for h, got, want in zip(c["hyps"], td, c["td"]):
            assert abs(got - want) <= (c["rows"] + len(h) + 1) * 1e-5, (name, len(h), got, want)
        for i, h in enumerate(c["hyps"]):   # ... and each alone gives the same bits
            assert tr.td_scores(c["enc"], [0], [c["rows"]], [[h]])[0][0] == td[i]
    # the recorded beams: td within the bar, the recorded choice wherever its margin exceeds twice the bar
    from chunkformer_amd.search import DecodeResult
    held = 0
    for c in fx.beam_cases(name):
        res = DecodeResult(list(c["tokens"][0]), c["scores"][0], nbest=c["tokens"], nbest_scores=c["scores"])
        r = tr.rescore([res], c["enc"], [0], [c["rows"]], 0.5, None, 0.5)[0]
        u_max = max(len(h) for h in c["tokens"])
        for h, got, want in zip(c["tokens"], r.td_scores, c["td"]):
            assert abs(got - want) <= (c["rows"] + len(h) + 1) * 1e-5
        if c["td_margin"] >= 2 * (c["rows"] + u_max + 1) * 1e-5 * 0.5:
            held += 1
            assert r.best_index == c["best_index"] and r.tokens == c["tokens"][c["best_index"]]
    assert held >= 4


@pytest.mark.parametrize("name", ["emb_v130", "conv_v1024"])
def test_td_bf16(name):
    from test_gpu_td_rescore import BF16_NODE_MEASURED, BF16_TOTAL_MEASURED
    node = _node_case(name, "bf16")
    tr = rescorer(name, "bf16")
    total = 0.0
    for c in fx.beam_cases(name)[:6]:
        td = tr.td_scores(c["enc"], [0], [c["rows"]], [c["tokens"]])[0]
        total = max(total, max(abs(a - b) for a, b in zip(td, c["td"])))
    print(f"{name} bf16: largest per-node deviation {node:.4e}, largest per-total deviation {total:.4e}")
    assert node <= 2 * BF16_NODE_MEASURED and total <= 2 * BF16_TOTAL_MEASURED


# ----------------------------------------------------------------------------- checkpoints through the model API
def _checkpoint(tmp_path, kind):
    import dataclasses

    import yaml

    from chunkformer_amd.config import SMALL
    from chunkformer_amd.transducer import RNNTConfig, synthetic_transducer_state_dict
    from chunkformer_amd.weights import synthetic_state_dict
    pc = {"embed_size": 64, "output_size": 64, "embed_dropout": 0.1, "history_size": 2, "bias": kind == "conv"}
    if kind == "embedding":
        pc["n_head"] = 4
    conf = {"encoder": "chunkformer", "input_dim": 80, "output_dim": 96, "model": "transducer",
            "encoder_conf": {"output_size": SMALL.d_model, "attention_heads": SMALL.n_heads, "linear_units": SMALL.ffn_dim,
                             "num_blocks": SMALL.num_blocks, "cnn_module_kernel": 15, "cnn_module_norm": "layer_norm",
                             "dynamic_conv": True},
            "predictor": kind, "predictor_conf": pc, "joint": "transducer_joint",
            "joint_conf": {"join_dim": 64, "enc_output_size": SMALL.d_model, "pred_output_size": 64}}
    c = RNNTConfig.from_conf(conf, 96, SMALL.d_model)
    cfg = dataclasses.replace(SMALL, vocab=c.vocab, cmvn=False)
    sd = {k: v for k, v in synthetic_state_dict(SMALL, 5).items() if "global_cmvn" not in k}
    gen = torch.Generator().manual_seed(11)
    sd["ctc.ctc_lo.weight"] = torch.rand(c.vocab, cfg.d_model, generator=gen) - 0.5
    sd["ctc.ctc_lo.bias"] = torch.zeros(c.vocab)
    tsd = synthetic_transducer_state_dict(c, 9, blank_bias=5.0)
    sd.update(tsd)
    torch.save(sd, os.path.join(tmp_path, "pytorch_model.bin"))
    with open(os.path.join(tmp_path, "config.yaml"), "w") as f:
        yaml.safe_dump(conf, f)
    return c, tsd


@pytest.mark.parametrize("kind", ["embedding", "conv"])
def test_from_pretrained_decodes_in_every_transducer_mode(tmp_path, kind):
    from chunkformer_amd import transducer_beam as TB
    from chunkformer_amd import transducer_rescore as TR
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.weights import synthetic_features
    from test_gpu_td_rescore import _rows
    c, tsd = _checkpoint(tmp_path, kind)
    m = ChunkFormerModel.from_pretrained(str(tmp_path), dtype="fp32")
    assert m.model_type == "transducer" and m.rnnt.cfg.predictor == kind and m.rnnt.grid_blocks(1) == 0
    host = TB.HostTransducer(c, tsd)
    xs = synthetic_features([420, 171, 300], 9)
    C, L, R, K = 64, 128, 128, 4
    rows, starts, el, el_ctc = _rows(m, xs, C, L, R)
    rows_h = rows.cpu()
    checked = {"greedy": 0, "beam": 0, "td": 0}
    # greedy: the host restatement's decisions wherever its smallest logit gap leaves them to f32
    got = m.batch_decode(xs, C, L, R)
    for s, n, g in zip(starts, el, got):
        dense, gap = TB.greedy_host(host, rows_h[s: s + n], [0], [n], 64)
        print(f"{kind} greedy: {n} rows, {len(g)} tokens, smallest gap {gap:.3e}")
        if gap >= 1e-3:
            checked["greedy"] += 1
            flat = dense.reshape(-1)
            assert list(g) == flat[flat != 0].tolist()
    one = m.endless_decode(xs[1], C, L, R)
    flat = one.reshape(-1).cpu().numpy()
    assert flat[flat != 0].tolist() == list(got[1])
    # rnnt_beam_search
    logp, _ = m.encoder.ctc_log_softmax(rows, want_logp=True, want_ids=False)
    beams = m.batch_decode(xs, C, L, R, decoding_method="rnnt_beam_search", beam_size=K)
    hb = TB.prefix_beam_search_host(host, rows_h, logp.cpu(), starts, el, K, 0.3, 0.7)
    for n, a, b in zip(el, beams, hb):
        print(f"{kind} beam: {n} rows, margin {b.margin:.3e}")
        if a.tokens == b.tokens:
            assert abs(a.nbest_scores[0] - b.nbest_scores[0]) <= (n + 1) * DEV
        if b.margin >= 2 * (n + 1) * DEV:
            checked["beam"] += 1
            assert a.nbest == b.nbest and a.nbest_times == b.nbest_times
    # the two rescoring modes (no decoder in the checkpoint: attn_weight 0)
    want_t = TR.rescore_host(host, None, rows_h, starts, el, beams, 0.5, 0.0, 0.5)
    got_t = m.batch_decode(xs, C, L, R, decoding_method="rnnt_beam_attn_rescoring", beam_size=K)
    ctc_beams = m.encoder.ctc_prefix_beam_search(rows, starts, el_ctc, K, None)
    want_c = TR.rescore_host(host, None, rows_h, starts, el_ctc, ctc_beams, 0.5, 0.0, 0.5)
    got_c = m.batch_decode(xs, C, L, R, decoding_method="ctc_beam_td_attn_rescoring", beam_size=K)
    for want, got2, lens in ((want_t, got_t, el), (want_c, got_c, el_ctc)):
        for w, g, T in zip(want, got2, lens):
            assert g.nbest == w.nbest or sorted(map(tuple, g.nbest)) == sorted(map(tuple, w.nbest))
            for a, b, hyp in zip(g.td_scores, w.td_scores, w.nbest):
                assert abs(a - b) <= (T + len(hyp) + 1) * 1e-5
            srt = sorted(w.nbest_scores, reverse=True)
            if len(srt) < 2 or srt[0] - srt[1] > 2 * (T + len(w.tokens) + 1) * 1e-5:
                checked["td"] += 1
                assert g.best_index == w.best_index and g.tokens == w.tokens
    print(f"{kind}: decisions checked against the host: {checked}")
    assert min(checked.values()) >= 1
