"""GPU: the transducer prefix beam search (csrc/rnnt_beam.hip, chunkformer_amd/transducer_beam.py) against the
reference's recorded beams (tests/golden/rnnt_beam.npz) and, step by step along the device's own trace, against the
CPU restatement.

Bars: tokens equal; scores within 1e-4 (the project's fp32 bar); the device's fused log-probs within 1e-5 of the
restatement's for the same prefix (the deviation the fixture's margins were sized for: margin >= 2 (rows + 1) 1e-5 in
every token-equality case).

Measured on an MI355X (printed by test_trace_is_consistent): the largest deviation over all cases is 3.3e-6."""
import numpy as np
import pytest
import torch

import rnnt_beam_fixture as fx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def searchers():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd.transducer import RNNTGreedy
    from chunkformer_amd.transducer_beam import RNNTBeamSearch
    out = {}
    for c in fx.cases():
        key = (c["model"], c["recipe"])
        if key not in out:
            cfg, sd = fx.model(*key)
            out[key] = RNNTBeamSearch(RNNTGreedy(cfg, sd, "cuda"))
    return out


@pytest.fixture(scope="module")
def device_results(searchers):
    """Every fixture case searched once on the device, with its trace."""
    res = []
    for i in range(len(fx.cases())):
        c = fx.case(i)
        dev = searchers[(c["model"], c["recipe"])]
        r = dev.search_packed(c["enc"].cuda(), c["ctc"].cuda(), [0], [c["rows"]], c["beam"], c["cw"], c["tw"],
                              return_trace=True)[0]
        res.append((c, r))
    return res


def test_equality_cases_reproduce_the_whole_beam(device_results):
    n = 0
    for c, r in device_results:
        if not c["equality"]:
            continue
        n += 1
        what = (c["model"], c["recipe"], c["rows"], c["beam"], c["cw"], c["tw"])
        assert r.nbest == c["tokens"], what
        np.testing.assert_allclose(r.nbest_scores, c["scores"], rtol=0, atol=1e-4, err_msg=str(what))
        assert r.tokens == c["tokens"][0] and r.score == r.nbest_scores[0]
        assert all(len(t) == len(h) and all(0 <= a < b < c["rows"] or a < b for a, b in zip(t, t[1:]))
                   for t, h in zip(r.nbest_times, r.nbest))
    assert n >= 100


def test_trace_is_consistent(device_results):
    """Along the device's own trace, every case (the trace-only ones included): each frame's kept beam is what
    beam_step_host makes of the device's previous beam and the device's top-K values (unless the host's own adjacent
    gap is under 1e-9), and each kept hypothesis' top-K values are within 1e-5 of the restatement's log-probs for
    that prefix."""
    from chunkformer_amd import transducer_beam as TB
    worst = 0.0
    for c, r in device_results:
        host = fx.host_model(c["model"], c["recipe"])
        cfg, K, tr = host.cfg, c["beam"], r.trace
        what = (c["model"], c["recipe"], c["rows"], K, c["cw"], c["tw"])
        hyps, scores, times = [()], [0.0], [()]
        h = torch.zeros(cfg.num_layers, 1, cfg.hidden)
        cs = torch.zeros(cfg.num_layers, 1, cfg.hidden)
        for t in range(c["rows"]):
            n = len(hyps)
            topv, topi = tr["topv"][t, :n], tr["topi"][t, :n]
            pred, hn, cn = host.step([hy[-1] if hy else cfg.blank for hy in hyps], h, cs)
            fused = TB.fuse_host(host.log_probs(c["enc"][t], pred), c["ctc"][t] if c["cw"] > 0 else None, c["cw"], c["tw"])
            assert ((topi >= 0) & (topi < cfg.vocab)).all(), what
            dev = float(np.abs(np.take_along_axis(fused.numpy(), topi.astype(np.int64), 1) - topv).max())
            worst = max(worst, dev)
            kept, gap = TB.beam_step_host(hyps, scores, topv, topi, K, cfg.blank)
            dpar, dtok, dsc = tr["parent"][t], tr["token"][t], tr["score"][t]
            m = int((dpar >= 0).sum())
            assert m == len(kept) and (dpar[:m] >= 0).all() and (dpar[:m] < n).all(), (what, t)
            if gap >= 1e-9:
                assert dpar[:m].tolist() == [k[2] for k in kept] and dtok[:m].tolist() == [k[3] for k in kept], (what, t)
                np.testing.assert_allclose(dsc[:m], [k[1] for k in kept], rtol=1e-12, atol=0, err_msg=str((what, t)))
            par = torch.as_tensor(dpar[:m].astype(np.int64))
            app = torch.as_tensor(dtok[:m] != cfg.blank).view(1, -1, 1)
            h, cs = torch.where(app, hn[:, par], h[:, par]), torch.where(app, cn[:, par], cs[:, par])
            times = [times[p] + (t,) if u != cfg.blank else times[p] for p, u in zip(dpar[:m], dtok[:m])]
            hyps = [hyps[p] + (int(u),) if u != cfg.blank else hyps[p] for p, u in zip(dpar[:m], dtok[:m])]
            scores = dsc[:m].tolist()
        assert r.nbest == [list(x) for x in hyps] and r.nbest_scores == scores, what
        assert r.nbest_times == [list(x) for x in times], what
    print(f"largest deviation of the device's fused log-probs from the restatement's: {worst:.3e}")
    assert worst <= 1e-5


def test_ragged_batch_equals_each_utterance_alone(searchers):
    dev = searchers[("v130", "dense")]
    cfg = dev.cfg
    lens = [0, 1, 2, 17, 65, 33]
    g = np.random.default_rng(7)
    rows = sum(lens)
    enc = torch.from_numpy(g.integers(-128, 128, size=(rows, cfg.enc_dim)).astype(np.float32) / 64.0).cuda()
    ctc = (torch.randn(rows, cfg.vocab, generator=torch.Generator().manual_seed(7)) * 2.0).log_softmax(-1).cuda()
    starts = np.cumsum([0] + lens[:-1]).tolist()
    for K, cw, tw in ((5, 0.3, 0.7), (16, 0.0, 1.0)):
        batch = dev.search_packed(enc, ctc, starts, lens, K, cw, tw)
        for s, n, rb in zip(starts, lens, batch):
            alone = dev.search_packed(enc[s: s + n], ctc[s: s + n], [0], [n], K, cw, tw)[0]
            assert rb.nbest == alone.nbest and rb.nbest_scores == alone.nbest_scores
            assert rb.nbest_times == alone.nbest_times and rb.tokens == alone.tokens and rb.times == alone.times
        assert batch[0].nbest == [[]] and batch[0].score == 0.0


def test_beam_one_without_ctc_is_the_greedy_search(searchers):
    """Beam 1 with (ctc_weight, transducer_weight) = (0, 1) takes the greedy search's decisions at n_steps = 1 (the
    fixture's (130, 1, (0, 1)) cases: their smallest decision margin is above 2.6e-3)."""
    n = 0
    for i, c in enumerate(fx.cases()):
        if c["beam"] != 1 or c["cw"] != 0.0 or c["rows"] < 9:
            continue
        n += 1
        c = fx.case(i)
        dev = searchers[(c["model"], c["recipe"])]
        r = dev.search_packed(c["enc"].cuda(), None, [0], [c["rows"]], 1, 0.0, 1.0)[0]
        dense = dev.rnnt.greedy_packed(c["enc"].cuda(), [0], [c["rows"]], n_steps=1).cpu().numpy()[:, 0]
        assert r.tokens == dense[dense != 0].tolist() and r.times == np.nonzero(dense)[0].tolist()
    assert n >= 4


def test_argument_errors(searchers):
    dev = searchers[("v37", "dense")]
    enc = torch.zeros(4, dev.cfg.enc_dim).cuda()
    ctc = torch.zeros(4, dev.cfg.vocab).cuda()
    for beam in (0, 17):
        with pytest.raises(ValueError, match="beam_size"):
            dev.search_packed(enc, ctc, [0], [4], beam)
    with pytest.raises(ValueError, match="weight"):
        dev.search_packed(enc, ctc, [0], [4], 2, -0.1, 1.0)
    with pytest.raises(ValueError, match="weight"):
        dev.search_packed(enc, ctc, [0], [4], 2, 0.0, 0.0)
    with pytest.raises(ValueError, match="ctc_logp"):
        dev.search_packed(enc, None, [0], [4], 2, 0.3, 0.7)
    with pytest.raises(ValueError, match="row ranges"):
        dev.search_packed(enc, ctc, [0], [5], 2)
    with pytest.raises(ValueError, match="row ranges"):
        dev.search_packed(enc, ctc, [-1], [2], 2)


@pytest.fixture(scope="module")
def transducer_model(golden_dir):
    import os
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd.config import LARGE
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.transducer import RNNTConfig, synthetic_transducer_state_dict
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    g = np.load(os.path.join(golden_dir, "rnnt.npz"))
    c = RNNTConfig(vocab=int(g["vocab"]))
    import dataclasses
    cfg = dataclasses.replace(LARGE, vocab=c.vocab)   # the CTC head over the transducer's vocabulary
    sd = synthetic_state_dict(LARGE, 5)
    gen = torch.Generator().manual_seed(11)
    sd["ctc.ctc_lo.weight"] = torch.rand(c.vocab, cfg.d_model, generator=gen) - 0.5
    sd["ctc.ctc_lo.bias"] = torch.zeros(c.vocab)
    sd.update(synthetic_transducer_state_dict(c, int(g["seed"]), blank_bias=6.0))
    m = ChunkFormerModel(cfg, sd, dtype="fp32", model_type="transducer", rnnt_config=c)
    return m, synthetic_features([420, 171, 300], 9)


def test_model_batch_and_endless_decode(transducer_model):
    """batch_decode and endless_decode with rnnt_beam_search equal search_packed over the model's own encoder rows and
    CTC log-probs, in text and in n-best; at ctc_weight 0 no CTC log-probs are computed."""
    from chunkformer_amd.model import class2str
    from chunkformer_amd.transducer_beam import RNNTBeamSearch
    from chunkformer_amd.weights import synthetic_vocab
    m, xs = transducer_model
    C, L, R, K = 64, 128, 128, 4
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int)
    eo, el, n_chunks, _, _, _ = m.encoder.forward_parallel_chunk(xs, lens, C, L, R, offset=torch.zeros(len(xs), dtype=torch.int))
    rows = eo.reshape(-1, eo.shape[-1])
    starts = (np.cumsum([0] + list(n_chunks[:-1])) * C).tolist()
    el = [max(0, int(n)) for n in el.tolist()]
    logp, _ = m.encoder.ctc_log_softmax(rows, want_logp=True, want_ids=False)
    search = RNNTBeamSearch(m.rnnt)
    want = search.search_packed(rows, logp, starts, el, K, 0.3, 0.7)
    assert any(len(w.tokens) > 0 for w in want)
    m.char_dict = None
    got = m.batch_decode(xs, C, L, R, decoding_method="rnnt_beam_search", beam_size=K)
    assert [r.nbest for r in got] == [r.nbest for r in want]
    assert [r.nbest_scores for r in got] == [r.nbest_scores for r in want]
    assert [r.times for r in got] == [r.times for r in want]
    cd = synthetic_vocab(m.rnnt.cfg.vocab)
    m.char_dict = cd
    try:
        assert m.batch_decode(xs, C, L, R, decoding_method="rnnt_beam_search", beam_size=K) == \
            [class2str(r.tokens, cd).strip() for r in want]
        assert m.batch_decode(xs, C, L, R, decoding_method="rnnt_beam_search", beam_size=K, return_nbest=True) == \
            [[class2str(h, cd).strip() for h in r.nbest] for r in want]
        # other weights reach the search
        w2 = search.search_packed(rows, logp, starts, el, K, 0.5, 0.25)
        assert m.batch_decode(xs, C, L, R, decoding_method="rnnt_beam_search", beam_size=K, ctc_weight=0.5,
                              transducer_weight=0.25) == [class2str(r.tokens, cd).strip() for r in w2]
        # endless_decode: the concatenated kept rows as one utterance
        m.char_dict = None
        res, eo1 = m.endless_decode(xs[0], C, L, R, return_encoder_out=True, decoding_method="rnnt_beam_search",
                                    beam_size=K)
        T = eo1.shape[1]
        lp1, _ = m.encoder.ctc_log_softmax(eo1[0], want_logp=True, want_ids=False)
        w1 = search.search_packed(eo1[0], lp1, [0], [T], K, 0.3, 0.7)[0]
        assert res.nbest == w1.nbest and res.nbest_scores == w1.nbest_scores and res.times == w1.times
        m.char_dict = cd
        assert m.endless_decode(xs[0], C, L, R, decoding_method="rnnt_beam_search", beam_size=K, return_nbest=True) == \
            [class2str(h, cd).strip() for h in w1.nbest]
        segs = m.endless_decode(xs[0], C, L, R, decoding_method="rnnt_beam_search", beam_size=K, max_silence_duration=-1)
        assert " ".join(s["decode"] for s in segs).strip() == class2str(w1.tokens, cd).strip()
        # ctc_weight 0: the CTC head is never called
        w0 = search.search_packed(rows, None, starts, el, K, 0.0, 1.0)
        real = m.encoder.ctc_log_softmax

        def boom(*a, **k):   # (endless_decode's segment runner takes the head's argmax ids, as for every model)
            if k.get("want_logp", True):
                raise AssertionError("CTC log-probs were computed at ctc_weight 0")
            return real(*a, **k)
        m.encoder.ctc_log_softmax = boom
        try:
            assert m.batch_decode(xs, C, L, R, decoding_method="rnnt_beam_search", beam_size=K, ctc_weight=0.0,
                                  transducer_weight=1.0) == [class2str(r.tokens, cd).strip() for r in w0]
            m.endless_decode(xs[0], C, L, R, decoding_method="rnnt_beam_search", beam_size=K, ctc_weight=0.0)
        finally:
            m.encoder.ctc_log_softmax = real
    finally:
        m.char_dict = None


@pytest.mark.parametrize("name,expected", [("v37", [7680, 40192, 2394112]), ("v130", [11264, 88064, 5496064])])
def test_workspace_bytes_are_pinned(name, expected):
    """cfm_rnnt_beam_workspace_bytes at (rows, B, beam) = (0, 1, 1), (65, 2, 5), (2601, 70, 10): the totals the library
    gave before the trie regions were carved by the searches' common function (csrc/beam.h); callers size their buffers
    from them."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import _lib
    from chunkformer_amd.transducer import RNNTGreedy
    g = RNNTGreedy(*fx.model(name, "dense"), "cuda")
    got = [int(_lib.cfm_rnnt_beam_workspace_bytes(g._h, *a)) for a in ((0, 1, 1), (65, 2, 5), (2601, 70, 10))]
    assert got == expected
