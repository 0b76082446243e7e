"""GPU parity at the scale the bench runs (chunkformer-large, 12 layers, C=64, L=R=128),
against fixtures the reference itself produced (tests/golden/gen_golden.py):

  * the 3 golden utterances (30 s, 12.3 s, 6 s) embedded at the start, middle and end of the
    full 240-min configs[1] batch (B=70 + 3 utterances, ~2,850 chunks: ~10 front-end window
    groups, ~90-chunk ring-attention runs per block) -- bf16 rows vs the golden;
  * the same utterances inside a 60-min batch on the fp32 model -- max-abs 1e-4;
  * forced multi-window-group front-end on the small fixture;
  * configs[3] geometry: endless_decode over 4 segments of <= 12,807 frames, final caches;
  * configs[4] geometry: full attention over a padded 30 s + 21 s batch;
  * 4-head d=512 (head_dim 128): masked batch + padded chunked path;
  * ring-kernel ineligible window widths (W > 320) fall back and stay correct.

Tolerances: fp32 max-abs 1e-4 on encoder rows (5e-4 where 12 layers accumulate
over long windows, stated per test); bf16 rel-L2 <= 2e-2 and CTC argmax agreement >= 99%.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16_RELL2 = 2e-2
BF16_MARGIN = 5e-2   # log-prob top-2 margin beyond which a bf16 CTC id must equal the reference's


def _rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _workload_lengths(total_frames, seed=0):
    """bench.py / SURVEY §8d generator (log-uniform 1 s .. 30 min)."""
    g = torch.Generator().manual_seed(seed)
    lens, tot = [], 0
    lo, hi = math.log(100), math.log(180000)
    while tot < total_frames:
        T = int(math.exp(lo + float(torch.rand(1, generator=g)) * (hi - lo)))
        T = min(T, total_frames - tot)
        lens.append(T)
        tot += T
    return lens


@pytest.fixture(scope="module")
def large():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd.config import LARGE
    from chunkformer_amd.encoder import ChunkFormerEncoder
    from chunkformer_amd.weights import synthetic_state_dict
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "large.npz"))
    sd = synthetic_state_dict(LARGE, int(g["seed"]))
    return g, sd, {dt: ChunkFormerEncoder(LARGE, sd, dtype=dt) for dt in ("fp32", "bf16")}


def _embedded_batch(g, minutes, dev):
    """The golden utterances at the start, middle and end of a `minutes` batch of synthetic
    utterances (features of the fillers drawn on the device)."""
    from chunkformer_amd.weights import synthetic_features
    glens = g["lens"].tolist()
    gx = synthetic_features(glens, int(g["feat_seed"]))
    fill = _workload_lengths(int(minutes * 6000) - sum(glens), seed=0)
    gen = torch.Generator(device=dev).manual_seed(77)
    fx = [torch.randn(t, 80, generator=gen, device=dev) for t in fill]
    mid = len(fill) // 2
    xs = [gx[0].to(dev)] + fx[:mid] + [gx[1].to(dev)] + fx[mid:] + [gx[2].to(dev)]
    pos = [0, mid + 1, len(xs) - 1]
    return xs, pos


def _rows_of(out, nch, u):
    starts = np.cumsum([0] + list(nch))
    return out[starts[u]: starts[u + 1]]


@pytest.mark.parametrize("dtype,minutes", [("bf16", 240), ("fp32", 60)])
def test_golden_utterances_inside_bench_batch(large, dtype, minutes):
    g, _, models = large
    enc = models[dtype]
    dev = enc.device
    xs, pos = _embedded_batch(g, minutes, dev)
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int32)
    out, olens, nch, _, _, _ = enc.forward_parallel_chunk(xs, lens, 64, 128, 128)
    if minutes == 240:
        assert sum(nch) > 2800   # the configs[1] geometry: ~10 front-end window groups
    _, ids = enc.ctc_log_softmax(out, want_logp=False)
    gnch = g["nchunks"].tolist()
    gstart = np.cumsum([0] + gnch)
    margin = g["top2"][..., 0] - g["top2"][..., 1]
    agree = []
    for k, u in enumerate(pos):
        assert nch[u] == gnch[k]
        o = _rows_of(out, nch, u).cpu().numpy()
        exp = g["out"][gstart[k]: gstart[k + 1]]
        i = _rows_of(ids, nch, u).cpu().numpy()
        ei = g["ids"][gstart[k]: gstart[k + 1]]
        if dtype == "fp32":
            np.testing.assert_allclose(o, exp, atol=1e-4, rtol=0, err_msg=f"utt {k}")
            sure = margin[gstart[k]: gstart[k + 1]] > 1e-3
            np.testing.assert_array_equal(i[sure], ei[sure])
        else:
            # bf16 moves the log-probs by ~1e-2 (random weights: many near-tied frames), so an id may
            # flip where the reference's own top-2 margin is that small; beyond BF16_MARGIN every id
            # must agree, and agreement over the golden frames stays >= 99%; per
            # utterance one flip is already 1.4% of the 6 s utterance's 74 frames, so the 99% bar is the
            # aggregate one
            m = margin[gstart[k]: gstart[k + 1]]
            flips = m[i != ei]
            print(f"bf16 golden utt {k}: rel-L2 {_rel_l2(o, exp):.2e}, CTC argmax agreement {(i == ei).mean():.4f}, "
                  f"{flips.size} flips, largest flipped margin {flips.max() if flips.size else 0:.2e}")
            assert _rel_l2(o, exp) <= BF16_RELL2, f"utt {k}: {_rel_l2(o, exp)}"
            agree.append(i == ei)
            np.testing.assert_array_equal(i[m > BF16_MARGIN], ei[m > BF16_MARGIN])
    if dtype == "bf16":
        total = np.concatenate([a.ravel() for a in agree]).mean()
        print(f"bf16 golden frames: CTC argmax agreement {total:.4f}")
        assert total >= 0.99


@pytest.mark.parametrize("opts", [{"wsp_small_div": 4, "attn_min_chunks": 16},
                                  {"wsp_small_div": 2, "wsp_small_rows": 1 << 30, "attn_min_chunks": 64},
                                  {"wsp_small_div": 8, "wsp_small_rows": 1 << 30}])
def test_launch_parameters_bit_identical(large, opts):
    """The pipelined endless_decode's launch parameters (streaming.PIPELINE_OPTS: fewer workgroups for
    the weight-stationary GEMMs, longer attention runs) only regroup the same per-row / per-chunk
    work: a 30-min masked batch is bit-identical to the default launches (here forced at every size)."""
    g, _, models = large
    enc = models["bf16"]
    xs, _ = _embedded_batch(g, 30, enc.device)
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int32)
    ref = enc.forward_parallel_chunk(xs, lens, 64, 128, 128)[0].clone()
    with enc.scoped_options(**opts):
        out = enc.forward_parallel_chunk(xs, lens, 64, 128, 128)[0]
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert torch.equal(enc.forward_parallel_chunk(xs, lens, 64, 128, 128)[0], ref)   # restored


@pytest.mark.parametrize("dtype,minutes,parts", [("bf16", 240, 2), ("fp32", 60, 3)])
def test_stream_split_bit_identical(large, dtype, minutes, parts):
    """forward_parallel_chunk runs a large masked batch as utterance groups on separate streams,
    staggered by encoder layer (encoder.py _encode_masked_split); the rows must equal the single
    launch sequence's bit for bit (every kernel computes a row / chunk from its own inputs)."""
    g, _, models = large
    enc = models[dtype]
    xs, _ = _embedded_batch(g, minutes, enc.device)
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int32)
    saved = (enc.stream_split, enc.split_min_chunks)
    try:
        enc.set_option("stream_split", 1)
        ref = enc.forward_parallel_chunk(xs, lens, 64, 128, 128)[0]
        enc.set_option("stream_split", parts)
        enc.set_option("split_min_chunks", 0)
        out = enc.forward_parallel_chunk(xs, lens, 64, 128, 128)[0]
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
    finally:
        enc.stream_split, enc.split_min_chunks = saved


@pytest.mark.parametrize("minutes,group,dtype", [(240, 0, "bf16"), (1, 2, "bf16"), (240, 0, "fp16"), (1, 2, "fp16")])
def test_frontend_fused_dw2_bit_identical(large, minutes, group, dtype):
    """16-bit front-end option fe_fuse_dw2: pw1 + ReLU + dw2 in one weight-stationary GEMM (the dw2
    taps applied to the pw1 tile ring in LDS, gemm_wst.hip EPI_DW2) must give the rows of the
    pw1 GEMM + fe_dw2_kernel pair bit for bit -- same bf16 / f16 pw1 values, same f32 taps and FMA
    order.  (1 minute, 2 windows per group: group offsets > 0 and blocks with a halo tile at range
    start.)"""
    g, sd, models = large
    if dtype not in models:
        from chunkformer_amd.config import LARGE
        from chunkformer_amd.encoder import ChunkFormerEncoder
        models[dtype] = ChunkFormerEncoder(LARGE, sd, dtype=dtype)
    enc = models[dtype]
    xs, _ = _embedded_batch(g, minutes, enc.device)
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int32)
    try:
        enc.set_option("gemm_wst", 2)   # small groups: the unfused pw1 on the same kernel at any M
        enc.set_option("fe_group_windows", group)
        enc.set_option("fe_fuse_dw2", 0)
        ref = enc.forward_parallel_chunk(xs, lens, 64, 128, 128)[0]
        enc.set_option("fe_fuse_dw2", 1)
        out = enc.forward_parallel_chunk(xs, lens, 64, 128, 128)[0]
        torch.cuda.synchronize()
        o2, r2 = out.reshape(-1, out.shape[-1]), ref.reshape(-1, ref.shape[-1])
        bad = (o2 != r2).any(dim=1).nonzero().flatten()
        assert bad.numel() == 0, (f"{bad.numel()} of {o2.shape[0]} rows differ, first {bad[:8].tolist()}, "
                                  f"max abs {(o2.float() - r2.float()).abs().max().item():.3e}")
    finally:
        enc.set_option("fe_fuse_dw2", 1)   # the default
        enc.set_option("fe_group_windows", 0)
        enc.set_option("gemm_wst", 1)


def test_frontend_window_groups_forced(large):
    """Cap the front-end at 2 windows per group (per-model option): the 30 s utterance's 6
    windows then run in 3 groups whose offsets into the intermediate buffers are > 0."""
    from chunkformer_amd.weights import synthetic_features
    g, _, models = large
    lens = g["lens"].tolist()
    xs = synthetic_features(lens, int(g["feat_seed"]))
    for dt, tol in (("fp32", 1e-4), ("bf16", None)):
        enc = models[dt]
        ref_out = enc.forward_parallel_chunk(xs, torch.tensor(lens, dtype=torch.int32), 64, 128, 128)[0]
        enc.set_option("fe_group_windows", 2)
        try:
            out = enc.forward_parallel_chunk(xs, torch.tensor(lens, dtype=torch.int32), 64, 128, 128)[0]
        finally:
            enc.set_option("fe_group_windows", 0)
        o = out.cpu().numpy()
        if tol:
            np.testing.assert_allclose(o, g["out"], atol=tol, rtol=0)
        else:
            assert _rel_l2(o, g["out"]) <= BF16_RELL2
        assert _rel_l2(o, ref_out.cpu().numpy()) <= (1e-6 if tol else 5e-3)


@pytest.mark.parametrize("minutes,dtype", [(1, "bf16"), (240, "bf16"), (1, "fp16"), (240, "fp16")])
def test_frontend_conv_kernels_agree(large, minutes, dtype):
    """16-bit conv0 + ReLU + dw1: the channel-stationary kernel (fe_conv 6, the default: dw1 on MFMA,
    conv0's ReLU output rounded to the 16-bit format as autocast does; bf16: the ReLU as the
    conversion's clamp on 2^-24-scaled values, f16: unscaled and a packed max) and the
    position-stationary one (fe_conv 1: dw1 in f32 on the VALU) both stay at the golden's bar and
    agree with each other to the format's rounding (1 minute: partial last blocks; 240 minutes: the
    bench batch)."""
    g, sd, models = large
    if dtype not in models:
        from chunkformer_amd.config import LARGE
        from chunkformer_amd.encoder import ChunkFormerEncoder
        models[dtype] = ChunkFormerEncoder(LARGE, sd, dtype=dtype)
    enc = models[dtype]
    bar = BF16_RELL2 if dtype == "bf16" else 5e-3
    xs, pos = _embedded_batch(g, minutes, enc.device)
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int32)
    outs = {}
    try:
        for v in (1, 6):
            enc.set_option("fe_conv", v)
            out, _, nch, _, _, _ = enc.forward_parallel_chunk(xs, lens, 64, 128, 128)
            outs[v] = out.float()
    finally:
        enc.set_option("fe_conv", 6)   # the default
    torch.cuda.synchronize()
    gstart = np.cumsum([0] + g["nchunks"].tolist())
    for v in (1, 6):
        for k, u in enumerate(pos):
            o = _rows_of(outs[v], nch, u).cpu().numpy()
            exp = g["out"][gstart[k]: gstart[k + 1]]
            assert _rel_l2(o, exp) <= bar, (v, k, _rel_l2(o, exp))
    a, b = outs[1].cpu().numpy(), outs[6].cpu().numpy()
    print(f"{dtype} fe_conv 6 vs 1: rel-L2 {_rel_l2(b, a):.2e}")
    assert _rel_l2(b, a) <= 5e-3


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_large_endless_decode(large, dtype):
    """configs[3] geometry: endless_decode, C=64 L=R=128, 12 layers, tbd=20 -> 4 segments; encoder
    rows, CTC ids and the final att/cnn caches against the reference's segment loop."""
    from chunkformer_amd.config import LARGE
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.weights import synthetic_features
    from conftest import GOLDEN
    _, sd, _ = large
    g = np.load(os.path.join(GOLDEN, "large_endless.npz"))
    assert int(g["seed"]) == 0
    C, L, R, tbd = (int(v) for v in g["clrt"])
    x = synthetic_features([int(g["T"])], int(g["feat_seed"]))[0]
    m = ChunkFormerModel(LARGE, sd, dtype=dtype)
    ids, eo = m.endless_decode(x, C, L, R, total_batch_duration=tbd, return_encoder_out=True)
    ac, cc = m.last_endless_caches
    eo = eo[0].cpu().numpy()
    assert eo.shape == g["out"].shape
    ids = ids.reshape(-1).cpu().numpy()
    att = ac[torch.from_numpy(g["att_layers"]).long().to(ac.device)].cpu().numpy()
    if dtype == "fp32":
        np.testing.assert_allclose(eo, g["out"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(att, g["att"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(cc.cpu().numpy(), g["cnn"], atol=1e-4, rtol=0)
        assert (ids == g["ids"]).mean() >= 0.999
    else:
        assert _rel_l2(eo, g["out"]) <= BF16_RELL2
        assert _rel_l2(att, g["att"]) <= BF16_RELL2
        assert _rel_l2(cc.cpu().numpy(), g["cnn"]) <= BF16_RELL2
        assert (ids == g["ids"]).mean() >= 0.99
    # 4 segments: endless_decode ran them pipelined (two streams); the one-call-per-segment loop
    # gives bit-identical rows, ids and carried caches
    ids_s, eo_s = m.endless_decode(x, C, L, R, total_batch_duration=tbd, return_encoder_out=True, pipeline=False,
                                   cuda_graph=False)
    assert torch.equal(eo_s[0].cpu(), torch.from_numpy(eo))
    assert np.array_equal(ids_s.reshape(-1).cpu().numpy(), ids)
    assert torch.equal(m.last_endless_caches[0], ac) and torch.equal(m.last_endless_caches[1], cc)


def test_large_endless_multi_block_graphs_equal_eager(large):
    """configs[3] as the bench runs it (chunkformer-large, bf16, C=64 L=R=128, the graph-replayed pipeline
    with trim_right and fe_reuse), on an input long enough for TWO block graphs: 1.3 M frames at tbd 200 =
    134 segments = a 128-segment block + a 6-segment block.  Rows, CTC ids and the final caches equal the
    one-segment-at-a-time eager loop with trim_right off bit for bit, and so do the graph pipeline with
    trim / fe_reuse off and the eager pipeline (chunkformer_model.py:344-435 is the eager loop's model)."""
    from chunkformer_amd.config import LARGE
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.weights import synthetic_features
    _, sd, _ = large
    m = ChunkFormerModel(LARGE, sd, dtype="bf16")
    x = synthetic_features([1_300_000], 91)[0]
    kw = dict(total_batch_duration=200, return_encoder_out=True)

    def run(trim, reuse, **mode):
        m.endless_trim, m.endless_fe_reuse = trim, reuse
        ids, eo = m.endless_decode(x, 64, 128, 128, **kw, **mode)
        return ids, eo, [c.clone() for c in m.last_endless_caches]

    try:
        ids0, eo0, c0 = run(False, False, cuda_graph=False, pipeline=False)
        assert eo0.shape[1] > 150_000
        for trim, reuse, mode in ((True, True, dict(cuda_graph=True, pipeline=True)),
                                  (False, False, dict(cuda_graph=True, pipeline=True)),
                                  (True, True, dict(cuda_graph=False, pipeline=True))):
            ids, eo, c = run(trim, reuse, **mode)
            tag = (trim, reuse, mode)
            assert torch.equal(eo, eo0), tag
            assert torch.equal(ids, ids0), tag
            assert all(torch.equal(a, b) for a, b in zip(c, c0)), tag
            if mode["cuda_graph"]:
                runner = next(iter(m._endless_runners.values()))
                assert runner.replayed == len(runner._keep) == 134, tag   # every segment from a graph
                assert len(runner.graphs) == 2, tag                        # two blocks: 128 + 6
                if reuse:
                    assert sum(s_["reuse"] for s_ in runner._keep) > 0
            del ids, eo, c
    finally:
        m.endless_trim, m.endless_fe_reuse = True, True


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_large_full_attention(large, dtype):
    """configs[4] geometry: full attention (chunk_size 0), padded 30 s + 21 s batch, 12 layers."""
    from chunkformer_amd.weights import synthetic_features
    from conftest import GOLDEN
    _, _, models = large
    g = np.load(os.path.join(GOLDEN, "large_full.npz"))
    lens = g["lens"].tolist()
    xs = synthetic_features(lens, int(g["feat_seed"]))
    xp = torch.zeros(len(lens), max(lens), 80)
    for i, t in enumerate(xs):
        xp[i, : t.shape[0]] = t
    y, masks = models[dtype].forward_encoder(xp, torch.tensor(lens), 0, 0, 0)
    np.testing.assert_array_equal(masks.cpu().numpy(), g["mask"])
    valid = g["mask"][:, 0, :]
    o = y.cpu().numpy()[valid]
    exp = g["out"][valid]
    if dtype == "fp32":
        np.testing.assert_allclose(o, exp, atol=1e-4, rtol=0)
    else:
        assert _rel_l2(o, exp) <= BF16_RELL2


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_large_full_attention_mixed_batch(large, dtype):
    """configs[4] as the bench runs it (dense bf16 kernel, padded batch of utterances <= 30 s), pinned at 9
    utterances of 30 s down to 1 s (large_full_mixed.npz, reference-generated): masks bit-exact, valid rows
    (fp32 1e-4; bf16 rel-L2 per utterance), CTC ids (fp32: where the reference's margin > 1e-3; bf16: >= 99%
    overall and every id whose margin exceeds BF16_MARGIN)."""
    from chunkformer_amd.weights import synthetic_features
    from conftest import GOLDEN
    _, _, models = large
    g = np.load(os.path.join(GOLDEN, "large_full_mixed.npz"))
    lens = g["lens"].tolist()
    xs = synthetic_features(lens, int(g["feat_seed"]))
    xp = torch.zeros(len(lens), max(lens), 80)
    for i, t in enumerate(xs):
        xp[i, : t.shape[0]] = t
    enc = models[dtype]
    y, masks = enc.forward_encoder(xp, torch.tensor(lens), 0, 0, 0)
    np.testing.assert_array_equal(masks.cpu().numpy(), g["mask"])
    valid = torch.from_numpy(g["mask"][:, 0, :]).to(y.device)
    rows = y[valid].contiguous()
    _, ids = enc.ctc_log_softmax(rows, want_logp=False)
    o, ids = rows.cpu().numpy(), ids.cpu().numpy()
    if dtype == "fp32":
        np.testing.assert_allclose(o, g["out"], atol=1e-4, rtol=0)
        sure = g["margin"] > 1e-3
        np.testing.assert_array_equal(ids[sure], g["ids"][sure])
    else:
        starts = np.cumsum([0] + g["mask"][:, 0, :].sum(-1).tolist())
        for u in range(len(lens)):
            r = _rel_l2(o[starts[u]: starts[u + 1]], g["out"][starts[u]: starts[u + 1]])
            assert r <= BF16_RELL2, (u, lens[u], r)
        agree = (ids == g["ids"]).mean()
        print(f"bf16 full attention, 9 utterances: rel-L2 {_rel_l2(o, g['out']):.2e}, CTC argmax agreement {agree:.4f}")
        assert agree >= 0.99
        big = g["margin"] > BF16_MARGIN
        np.testing.assert_array_equal(ids[big], g["ids"][big])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_four_heads_head_dim_128(dtype):
    """d=512 with 4 heads (head_dim 128, the reference's large vie recipe family)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd.config import LARGE_4H
    from chunkformer_amd.encoder import ChunkFormerEncoder
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "large_4h.npz"))
    enc = ChunkFormerEncoder(LARGE_4H, synthetic_state_dict(LARGE_4H, int(g["seed"])), dtype=dtype)
    lens = g["lens"].tolist()
    xs = synthetic_features(lens, int(g["feat_seed"]))
    out, _, nch, _, _, _ = enc.forward_parallel_chunk(xs, torch.tensor(lens, dtype=torch.int32), 64, 128, 128)
    assert nch == g["nchunks"].tolist()
    _, ids = enc.ctc_log_softmax(out, want_logp=False)
    xp = torch.zeros(len(lens), max(lens), 80)
    for i, t in enumerate(xs):
        xp[i, : t.shape[0]] = t
    y, masks = enc.forward_encoder(xp, torch.tensor(lens), 64, 128, 128)
    np.testing.assert_array_equal(masks.cpu().numpy(), g["pc_mask"])
    if dtype == "fp32":
        np.testing.assert_allclose(out.cpu().numpy(), g["out"], atol=1e-4, rtol=0)
        np.testing.assert_allclose(y.cpu().numpy(), g["pc_out"], atol=1e-4, rtol=0)
        margin = g["top2"][..., 0] - g["top2"][..., 1]
        sure = margin > 1e-3
        np.testing.assert_array_equal(ids.cpu().numpy()[sure], g["ids"][sure])
    else:
        assert _rel_l2(out.cpu().numpy(), g["out"]) <= BF16_RELL2
        assert _rel_l2(y.cpu().numpy(), g["pc_out"]) <= BF16_RELL2
        assert (ids.cpu().numpy() == g["ids"]).mean() >= 0.99


@pytest.mark.parametrize("C,L,R", [(32, 160, 160), (16, 176, 176)])
def test_wide_windows_fall_back_correctly(C, L, R):
    """W = L + C + R > 320 is not eligible for the ring kernel (5 x 64 scores in registers): the
    generic kernel runs, and the result matches the oracle (advisor finding, round 1)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.encoder import ChunkFormerEncoder
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    from oracle import encoder_ref as ref
    sd = synthetic_state_dict(SMALL, 1)
    lens = [2100, 700, 333]
    xs = synthetic_features(lens, 41)
    r_out = ref.forward_parallel_chunk(sd, SMALL, xs, lens, C, L, R)[0].numpy()
    for dt in ("fp32", "bf16"):
        enc = ChunkFormerEncoder(SMALL, sd, dtype=dt)
        out = enc.forward_parallel_chunk(xs, torch.tensor(lens, dtype=torch.int32), C, L, R)[0].cpu().numpy()
        if dt == "fp32":
            np.testing.assert_allclose(out, r_out, atol=1e-4, rtol=0)
        else:
            assert _rel_l2(out, r_out) <= BF16_RELL2


@pytest.fixture(scope="module")
def model_4h():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd.config import LARGE_4H
    from chunkformer_amd.encoder import ChunkFormerEncoder
    from chunkformer_amd.weights import synthetic_state_dict
    return ChunkFormerEncoder(LARGE_4H, synthetic_state_dict(LARGE_4H, 0), dtype="bf16")


def _fast_vs_generic(enc, lens, seed, C, L, R):
    from chunkformer_amd.weights import synthetic_features
    xs = synthetic_features(lens, seed)
    tl = torch.tensor(lens, dtype=torch.int32)
    fast = enc.forward_parallel_chunk(xs, tl, C, L, R)[0].cpu().numpy()
    enc.set_option("ring_attention", 0)
    try:
        gen = enc.forward_parallel_chunk(xs, tl, C, L, R)[0].cpu().numpy()
    finally:
        enc.set_option("ring_attention", 1)
    assert np.isfinite(fast).all()
    return _rel_l2(fast, gen)


# every key-tile count the head_dim-128 kernel is built for (W = L + 64 + R = 64 .. 320, NT = 1 .. 5)
@pytest.mark.parametrize("C,L,R", [(64, 0, 0), (64, 64, 0), (64, 64, 64), (64, 96, 96), (64, 128, 128)])
def test_head_dim_128_kernel_vs_generic(model_4h, C, L, R):
    """The head_dim 128 masked-batch kernel (attention128.hip) against the generic per-block kernel
    (model option ring_attention = 0) on the 4-head d=512 model, 12 layers, a batch with utterance
    starts / ends (masked key ranges), a 1-chunk utterance and a T < 15 one."""
    rel = _fast_vs_generic(model_4h, [30_000, 519, 3000, 7, 12_345, 1100, 64_000], 17, C, L, R)
    print(f"head_dim 128 kernel vs generic (C={C} L={L} R={R}): rel-L2 {rel:.2e}")
    assert rel <= 5e-3


@pytest.mark.parametrize("C,L,R", [(64, 128, 128), (64, 64, 64), (64, 0, 0), (32, 64, 32), (48, 16, 32),
                                   (16, 32, 32), (64, 128, 0), (64, 62, 0), (32, 30, 0)])
def test_ring_kernel_shapes_vs_generic(large, C, L, R):
    """The dk = 64 ring kernel against the generic kernel on chunkformer-large (12 layers, 8 heads)
    over the chunk / context shapes it accepts (C % 16 == 0, W even and <= 320; the last two have
    W % 4 == 2: next-pair staging in row pairs), utterance edges included."""
    _, _, models = large
    rel = _fast_vs_generic(models["bf16"], [20_000, 519, 3000, 7, 1100, 9000], 19, C, L, R)
    print(f"ring kernel vs generic (C={C} L={L} R={R}): rel-L2 {rel:.2e}")
    assert rel <= 5e-3


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_small256_recipe_shape(dtype):
    """The reference's shipped small recipes (d=256, 4 heads, ff 2048, 12 blocks, bpe1024;
    examples/asr/ctc/conf/chunkformer-ctc-small-libri-100h.yaml:5-8) against small256.npz: masked
    batch at C=64 L=R=128 (+ CTC ids), the padded chunked path, and a C=128 masked batch."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd.config import SMALL256
    from chunkformer_amd.encoder import ChunkFormerEncoder
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    from conftest import GOLDEN, with_fixture_ctc_head
    g = np.load(os.path.join(GOLDEN, "small256.npz"))
    sd = with_fixture_ctc_head(synthetic_state_dict(SMALL256, int(g["seed"])), g)
    enc = ChunkFormerEncoder(SMALL256, sd, dtype=dtype)
    lens = g["lens"].tolist()
    xs = synthetic_features(lens, int(g["feat_seed"]))
    tl = torch.tensor(lens, dtype=torch.int32)
    out, olens, nch, _, _, _ = enc.forward_parallel_chunk(xs, tl, 64, 128, 128)
    assert nch == g["nchunks"].tolist() and olens.tolist() == g["outlens"].tolist()
    _, ids = enc.ctc_log_softmax(out, want_logp=False)
    ids = ids.cpu().numpy()
    xp = torch.zeros(len(lens), max(lens), 80)
    for i, t in enumerate(xs):
        xp[i, : t.shape[0]] = t
    y, masks = enc.forward_encoder(xp, torch.tensor(lens), 64, 128, 128)
    np.testing.assert_array_equal(masks.cpu().numpy(), g["pc_mask"])
    out2, olens2, nch2, _, _, _ = enc.forward_parallel_chunk(xs, tl, 128, 128, 128)
    assert nch2 == g["c128_nchunks"].tolist() and olens2.tolist() == g["c128_outlens"].tolist()
    margin = g["top2"][..., 0] - g["top2"][..., 1]
    pairs = ((out, g["out"]), (y, g["pc_out"]), (out2, g["c128_out"]))
    for a, b in pairs:
        if dtype == "fp32":
            np.testing.assert_allclose(a.float().cpu().numpy(), b, atol=1e-4, rtol=0)
        else:
            assert _rel_l2(a.float().cpu().numpy(), b) <= BF16_RELL2
    # the fixture's CTC head is peaked (reference median top-2 margin 0.70, min 8e-3;
    # gen_golden.py:peaked_ctc_head): ids are compared over ALL frames, no margin filter
    agree = float((ids == g["ids"]).mean())
    print(f"small256 {dtype}: CTC argmax agreement {agree:.4f} over all {ids.size} frames "
          f"(reference median top-2 margin {float(np.median(margin)):.3f})")
    if dtype == "fp32":
        np.testing.assert_array_equal(ids, g["ids"])
    else:
        assert agree >= 0.99
