"""GPU: the kernels of the transducer prefix beam search (csrc/rnnt_beam.hip) one at a time, through the
operator entry points of include/cfm_ops.h.

Tolerances: fused log-probs and LSTM outputs are f32 values of magnitude <= ~20 formed from <= 1024-term f32 sums:
1e-5 absolute (the issue's bar).  The prune step works in f64 on its inputs: parents and tokens are integers and
must be equal, scores agree to 1e-12 relative (the device's and the host's f64 exp / log differ in the last place)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tb():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import transducer_beam
    return transducer_beam


def _fused_ref(logits, ctc, cw, tw):
    lp = logits.log_softmax(-1)
    second = cw * torch.exp(ctc) if ctc is not None else torch.zeros(1, 1)
    return torch.log(tw * torch.exp(lp) + second)


@pytest.mark.parametrize("V", [5, 37, 64, 65, 130, 1024, 5003, 8200])
def test_fused_topk_vs_torch(tb, V):
    """log-softmax + CTC fusion + top K against torch, K in {1, 2, 5, 16} and K = V, with two duplicated columns that
    are the row's largest (index-ascending order among equal values) and with cw = 0 and no CTC rows.  V = 8200 is
    past the kernel's LDS key cache: the keys are formed again in every round."""
    gen = torch.Generator().manual_seed(V)
    R = 7
    logits = torch.randn(R, V, generator=gen) * 3.0
    ctc = (torch.randn(R, V, generator=gen) * 2.0).log_softmax(-1)
    a, b = (3, 1) if V == 5 else (V - 2, V // 3)
    logits[:, a] = logits[:, b] = logits.max(1).values + 1.0
    ctc[:, a] = ctc[:, b] = ctc.max(1).values
    worst = 0.0
    for K in sorted({k for k in (1, 2, 5, 16) if k <= V} | ({V} if V <= 16 else set())):
        for cw, tw, use_ctc in ((0.3, 0.7, True), (1.0, 0.0, True), (0.0, 1.0, False)):
            ref = _fused_ref(logits, ctc if use_ctc else None, cw, tw)
            vals, ids = tb.fused_topk_device(logits.cuda(), ctc.cuda() if use_ctc else None, K, cw, tw)
            vals, ids = vals.cpu(), ids.cpu().long()
            assert ((ids >= 0) & (ids < V)).all()
            assert all(len(set(row.tolist())) == K for row in ids), "top-K ids must be distinct"
            want = ref.sort(-1, descending=True).values[:, :K]
            worst = max(worst, float((vals - want).abs().max()), float((vals - ref.gather(1, ids)).abs().max()))
            assert (vals[:, :-1] >= vals[:, 1:]).all()
            tie = vals[:, :-1] == vals[:, 1:]
            assert (ids[:, :-1][tie] < ids[:, 1:][tie]).all(), "equal values come index ascending"
            if K >= 2 and tw > 0:
                assert ids[:, 0].tolist() == [min(a, b)] * R and ids[:, 1].tolist() == [max(a, b)] * R
                assert (vals[:, 0] == vals[:, 1]).all()
    print(f"fused top-k V={V}: largest deviation {worst:.3e}")
    assert worst <= 1e-5


def _host_walk(tb, topv, topi, K, blank=0):
    T = topv.shape[0]
    hyps, scores = [()], [0.0]
    par = np.full((T, K), -1, np.int32)
    tok = np.full((T, K), -1, np.int32)
    sc = np.zeros((T, K))
    cnt = np.zeros(T, np.int32)
    fusions = ties = 0
    for t in range(T):
        n = len(hyps)
        kept, gap = tb.beam_step_host(hyps, scores, topv[t, :n], topi[t, :n], K, blank)
        ties += gap == 0.0
        seen = {}
        for j in range(n):
            for q in range(K):
                u = int(topi[t, j, q])
                new = hyps[j] if u == blank else hyps[j] + (u,)
                if new in seen:
                    fusions += 1
                else:
                    seen[new] = j
        for r, (hyp, s, p, u, _) in enumerate(kept):
            par[t, r], tok[t, r], sc[t, r] = p, u, s
        cnt[t] = len(kept)
        hyps, scores = [k[0] for k in kept], [k[1] for k in kept]
    return par, tok, sc, cnt, fusions, ties


@pytest.mark.parametrize("K,V,seed", [(1, 3, 0), (2, 3, 1), (5, 6, 2), (5, 5, 3), (16, 17, 4), (16, 16, 5)])
def test_prune_vs_beam_step_host(tb, K, V, seed):
    """T frames of expand / fuse / prune from the start state (so n < K at first) against beam_step_host iterated on
    the same inputs.  The ids of a row are a K-subset of a vocabulary of K or K + 1 (K = V included), so extensions
    fold into unchanged prefixes ranked above and below them all the time; the values are multiples of 1/4, so
    candidate scores tie exactly."""
    g = np.random.default_rng(seed)
    T = 14
    topv = -np.sort(g.integers(1, 24, size=(T, K, K)), axis=-1).astype(np.float32) / 4.0   # descending per row
    topi = np.stack([np.stack([g.permutation(V)[:K] for _ in range(K)]) for _ in range(T)]).astype(np.int32)
    par, tok, sc, cnt, fusions, ties = _host_walk(tb, topv, topi, K)
    dpar, dtok, dsc, dcnt = tb.beam_prune_device(torch.from_numpy(topv).cuda(), torch.from_numpy(topi).cuda(), 0)
    if K > 1:
        assert fusions > 0 and ties > 0, "the inputs must exercise fusion and exact ties"
    np.testing.assert_array_equal(dcnt, cnt)
    np.testing.assert_array_equal(dpar, par)
    np.testing.assert_array_equal(dtok, tok)
    live = par >= 0
    np.testing.assert_allclose(dsc[live], sc[live], rtol=1e-12, atol=0)


def test_prune_hand_made_fusion_order(tb):
    """Two frames by hand, K = 2, ids {0 = blank, 1}: after frame 0 the beam is [(), (1,)] or [(1,), ()]; in frame 1
    the extension () + 1 meets the unchanged (1,) -- above it in one order, below it in the other -- and the kept
    position is the earlier candidate's."""
    for first_blank in (True, False):
        v0 = [[-0.25, -0.5], [0, 0]]
        i0 = [[0, 1], [0, 0]] if first_blank else [[1, 0], [0, 0]]
        v1 = [[-0.25, -0.5], [-0.25, -0.75]]
        i1 = [[1, 0], [0, 1]] if first_blank else [[0, 1], [1, 0]]
        topv = np.array([v0, v1], np.float32)
        topi = np.array([i0, i1], np.int32)
        par, tok, sc, cnt, fusions, _ = _host_walk(tb, topv, topi, 2)
        assert fusions == 1
        dpar, dtok, dsc, dcnt = tb.beam_prune_device(torch.from_numpy(topv).cuda(), torch.from_numpy(topi).cuda(), 0)
        np.testing.assert_array_equal(dcnt, cnt)
        np.testing.assert_array_equal(dpar, par)
        np.testing.assert_array_equal(dtok, tok)
        np.testing.assert_allclose(dsc, sc, rtol=1e-12, atol=0)


def reentry_case():
    """Five frames by hand, K = 2, ids {0 = blank, 1, 2, 3}: (topv, topi, the host's beam after every frame).  The beams
    are [(), (1,)], [(), (1, 2)], [(1,), (1, 2)], [(1, 2), (1,)], [(1, 2), (1, 2, 3)]: the prefix (1,) leaves the beam at
    frame 1 while its extension (1, 2) stays, is created again from () at frame 2, and at frames 3 and 4 its extension
    by 2 meets the unchanged (1, 2) -- as the earlier candidate at frame 3, as the later one at frame 4."""
    from chunkformer_amd.transducer_beam import beam_step_host
    frames = [
        ([[-0.25, -0.5], [0, 0]], [[0, 1], [0, 0]]),
        ([[-0.25, -8.0], [-0.25, -6.0]], [[0, 3], [2, 0]]),
        ([[-0.25, -6.0], [-0.5, -8.0]], [[1, 0], [0, 3]]),
        ([[-0.25, -1.0], [-0.25, -8.0]], [[2, 0], [0, 3]]),
        ([[-0.25, -0.5], [-0.25, -0.5]], [[0, 3], [2, 0]]),
    ]
    topv = np.array([v for v, _ in frames], np.float32)
    topi = np.array([i for _, i in frames], np.int32)
    hyps, scores, beams = [()], [0.0], []
    for t in range(len(frames)):
        kept, _ = beam_step_host(hyps, scores, topv[t, :len(hyps)], topi[t, :len(hyps)], 2, 0)
        hyps, scores = [k[0] for k in kept], [k[1] for k in kept]
        beams.append(list(hyps))
    return topv, topi, beams


def test_prune_prefix_reenters_and_fuses(tb):
    """The map lives for the whole utterance, seen from the transducer prune kernel: a prefix that left the beam and
    is created again gets its old node back, so its next extension still meets the longer hypothesis that survived
    and fuses with it.  With a map that forgot the prefix, frame 3 would keep (1, 2) twice."""
    topv, topi, beams = reentry_case()
    gone = [t for t, b in enumerate(beams) if (1,) not in b]
    assert (1,) in beams[0] and (1,) in beams[2] and gone == [1, 4] and (1, 2) in beams[1], "no re-entry in the case"
    assert all(len(set(b)) == 2 for b in beams)
    par, tok, sc, cnt, fusions, _ = _host_walk(tb, topv, topi, 2)
    assert fusions == 2 and tok[3].tolist() == [2, 0] and tok[4].tolist() == [0, 3]
    dpar, dtok, dsc, dcnt = tb.beam_prune_device(torch.from_numpy(topv).cuda(), torch.from_numpy(topi).cuda(), 0)
    np.testing.assert_array_equal(dcnt, cnt)
    np.testing.assert_array_equal(dpar, par)
    np.testing.assert_array_equal(dtok, tok)
    np.testing.assert_allclose(dsc, sc, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["v37", "v130"])
def test_lstm_step_vs_torch(tb, name):
    """Embedding + LSTM layers + projection + pred_ffn for 21 rows against torch.nn.LSTM in f32 (1 and 2 layers)."""
    import rnnt_beam_fixture as fx
    from chunkformer_amd.transducer import RNNTGreedy
    cfg, sd = fx.model(name, "dense")
    host = fx.host_model(name, "dense")
    dev = tb.RNNTBeamSearch(RNNTGreedy(cfg, sd, "cuda"))
    gen = torch.Generator().manual_seed(3)
    R = 21
    tokens = torch.randint(0, cfg.vocab, (R,), generator=gen)
    h = torch.rand(cfg.num_layers, R, cfg.hidden, generator=gen) * 2 - 1
    c = torch.rand(cfg.num_layers, R, cfg.hidden, generator=gen) * 2 - 1
    pred, hn, cn = host.step(tokens.tolist(), h, c)
    pj = torch.nn.functional.linear(pred[:, 0], sd["joint.pred_ffn.weight"], sd["joint.pred_ffn.bias"])
    dh, dc, dpj = dev.lstm_step(tokens, h, c)
    worst = max(float((dh.cpu() - hn).abs().max()), float((dc.cpu() - cn).abs().max()))
    wpj = float((dpj.cpu() - pj).abs().max())
    print(f"lstm step {name}: state deviation {worst:.3e}, pred_ffn output deviation {wpj:.3e}")
    assert worst <= 1e-5 and wpj <= 1e-5
