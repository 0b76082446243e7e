"""GPU parity: libcfm.so (HIP, gfx950) against the reference-generated golden fixtures
and the oracle, through the C-ABI (chunkformer_amd.encoder mirror).

Tolerances:
  masks / n_chunks / lens : bit-exact
  fp32 mode               : max-abs <= FP32_ATOL on encoder output and CTC log-probs
  bf16 mode               : rel-L2 <= 2e-2 and CTC argmax agreement >= 99%
  fp16 mode               : rel-L2 <= 5e-3 (the reference's own autocast fp16 run is at 1.4e-3 of its f32
                            run on the 12-layer model, tests/test_gpu_autocast.py) and agreement >= 99%
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FP32_ATOL = 1e-4
BF16_RELL2 = 2e-2
RELL2 = {"bf16": BF16_RELL2, "fp16": 5e-3}


def _rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def cfm():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import chunkformer_amd.encoder as enc
    return enc


@pytest.fixture(scope="module")
def small_g(golden_dir):
    return np.load(os.path.join(golden_dir, "small.npz"))


@pytest.fixture(scope="module")
def small_models(cfm, small_g):
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(SMALL, int(small_g["seed"]))
    return {dt: cfm.ChunkFormerEncoder(SMALL, sd, dtype=dt) for dt in ("fp32", "bf16", "fp16")}


def test_masks_bit_exact(cfm, small_models, golden_dir):
    g = np.load(os.path.join(golden_dir, "masks.npz"))
    enc = small_models["fp32"]
    for i in range(int(g["n_cases"])):
        C, L, R = (int(v) for v in g[f"c{i}_clr"])
        lens = torch.from_numpy(g[f"c{i}_lens"])
        offs = torch.from_numpy(g[f"c{i}_offs"].astype(np.int64))
        att, pad = enc.masks(lens, C, L, R, offs)
        sa, sp = g[f"c{i}_att_shape"], g[f"c{i}_pad_shape"]
        exp_att = np.unpackbits(g[f"c{i}_att"], axis=-1, count=int(sa[1])).astype(bool)
        exp_pad = np.unpackbits(g[f"c{i}_pad"], axis=-1, count=int(sp[1])).astype(bool)
        np.testing.assert_array_equal(att[:, 0].cpu().numpy(), exp_att, err_msg=f"case {i}")
        np.testing.assert_array_equal(pad[:, 0].cpu().numpy(), exp_pad, err_msg=f"case {i}")


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_masked_batch(cfm, small_models, small_g, case, dtype):
    from chunkformer_amd.weights import synthetic_features
    g = small_g
    enc = small_models[dtype]
    lens = g[f"{case}_lens"].tolist()
    C, L, R = (int(v) for v in g[f"{case}_clr"])
    xs = synthetic_features(lens, int(g[f"{case}_seed"]))
    out, olens, nch, ra, rc, off = enc.forward_parallel_chunk(xs, torch.tensor(lens, dtype=torch.int32), C, L, R)
    assert nch == g[f"{case}_nchunks"].tolist()
    assert olens.tolist() == g[f"{case}_outlens"].tolist()
    assert off.tolist() == g[f"{case}_outlens"].tolist()
    assert tuple(ra.shape) == (2, 0, 0, 0) and tuple(rc.shape) == (2, 0, 0)
    o = out.cpu().numpy()
    exp = g[f"{case}_out"]
    assert np.isfinite(o).all()
    if dtype == "fp32":
        np.testing.assert_allclose(o, exp, atol=FP32_ATOL, rtol=0)
    else:
        assert _rel_l2(o, exp) <= RELL2[dtype]
    if case == "a":
        logp, ids = enc.ctc_log_softmax(out)
        lp = logp.cpu().numpy()
        if dtype == "fp32":
            np.testing.assert_allclose(lp, g["a_logp"], atol=FP32_ATOL * 5, rtol=0)
        agree = (ids.cpu().numpy() == g["a_logp"].argmax(-1)).mean()
        assert agree >= (0.999 if dtype == "fp32" else 0.99)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_cache_path(cfm, small_models, small_g, dtype):
    from chunkformer_amd.weights import synthetic_features
    g = small_g
    enc = small_models[dtype]
    xs = synthetic_features([900], int(g["cache_seed"]))
    off = torch.tensor([5], dtype=torch.int32)
    out, _, _, ac, cc, off2 = enc.forward_parallel_chunk(
        xs, torch.tensor([900], dtype=torch.int32), 16, 32, 32, torch.from_numpy(g["cache_att_in"]),
        torch.from_numpy(g["cache_cnn_in"]), 48, off)
    assert off2.tolist() == g["cache_offset_out"].tolist()
    for got, exp in ((out, g["cache_out"]), (ac, g["cache_att_out"]), (cc, g["cache_cnn_out"])):
        got = got.cpu().numpy()
        if dtype == "fp32":
            np.testing.assert_allclose(got, exp, atol=FP32_ATOL, rtol=0)
        else:
            assert _rel_l2(got, exp) <= RELL2[dtype]


@pytest.mark.parametrize("case", ["pc", "pf"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_padded_path(cfm, small_models, small_g, case, dtype):
    from chunkformer_amd.weights import synthetic_features
    g = small_g
    enc = small_models[dtype]
    lens = g[f"{case}_lens"].tolist()
    C, L, R = (int(v) for v in g[f"{case}_clr"])
    xs = synthetic_features(lens, int(g[f"{case}_seed"]))
    xp = torch.zeros(len(lens), max(lens), 80)
    for i, t in enumerate(xs):
        xp[i, : t.shape[0]] = t
    out, masks = enc.forward_encoder(xp, torch.tensor(lens), C, L, R)
    np.testing.assert_array_equal(masks.cpu().numpy(), g[f"{case}_mask"])
    o = out.cpu().numpy()
    if dtype == "fp32":
        np.testing.assert_allclose(o, g[f"{case}_out"], atol=FP32_ATOL, rtol=0)
    else:
        assert _rel_l2(o, g[f"{case}_out"]) <= RELL2[dtype]


@pytest.mark.parametrize("case", ["pc", "pf"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_padded_path_tiny_utterances(cfm, small_models, small_g, golden_dir, case, dtype):
    """The padded path with 5- and 3-frame utterances in the batch (tiny_padded.npz: calc_length -1,
    masks without a valid frame, their attention rows fully masked -> the reference's NaN -> 0)."""
    from chunkformer_amd.weights import synthetic_features
    g = np.load(os.path.join(golden_dir, "tiny_padded.npz"))
    assert int(g["seed"]) == int(small_g["seed"])
    enc = small_models[dtype]
    lens = g["lens"].tolist()
    C, L, R = (int(v) for v in g[f"{case}_clr"])
    xs = synthetic_features(lens, int(g["feat_seed"]))
    xp = torch.zeros(len(lens), max(lens), 80)
    for i, t in enumerate(xs):
        xp[i, : t.shape[0]] = t
    out, masks = enc.forward_encoder(xp, torch.tensor(lens), C, L, R)
    np.testing.assert_array_equal(masks.cpu().numpy(), g[f"{case}_mask"])
    o = out.cpu().numpy()
    assert np.isfinite(o).all()
    if dtype == "fp32":
        np.testing.assert_allclose(o, g[f"{case}_out"], atol=FP32_ATOL, rtol=0)
    else:
        assert _rel_l2(o, g[f"{case}_out"]) <= RELL2[dtype]


@pytest.fixture(scope="module")
def large(cfm, golden_dir):
    from chunkformer_amd.config import LARGE
    from chunkformer_amd.weights import synthetic_state_dict
    g = np.load(os.path.join(golden_dir, "large.npz"))
    sd = synthetic_state_dict(LARGE, int(g["seed"]))
    return g, {dt: cfm.ChunkFormerEncoder(LARGE, sd, dtype=dt) for dt in ("fp32", "bf16", "fp16")}


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_large_12L(cfm, large, dtype):
    from chunkformer_amd.weights import synthetic_features
    g, models = large
    enc = models[dtype]
    lens = g["lens"].tolist()
    xs = synthetic_features(lens, int(g["feat_seed"]))
    out, olens, nch, _, _, _ = enc.forward_parallel_chunk(xs, torch.tensor(lens, dtype=torch.int32), 64, 128, 128)
    assert nch == g["nchunks"].tolist()
    o = out.cpu().numpy()
    _, ids = enc.ctc_log_softmax(out, want_logp=False)
    ids = ids.cpu().numpy()
    margin = g["top2"][..., 0] - g["top2"][..., 1]
    if dtype == "fp32":
        # max-abs <= 1e-4 (measured 4.9e-6 on the box, tools/large12_err.py), ids equal
        # wherever the reference's top-2 margin is >= 1e-4
        np.testing.assert_allclose(o, g["out"], atol=FP32_ATOL, rtol=0)
        sure = margin > 1e-4
        np.testing.assert_array_equal(ids[sure], g["ids"][sure])
    else:
        assert _rel_l2(o, g["out"]) <= RELL2[dtype]
        assert (ids == g["ids"]).mean() >= 0.99


@pytest.mark.parametrize("case", ["a", "c"])
def test_ring_attention_matches_generic(cfm, small_models, small_g, case):
    """bf16: the sliding-ring attention kernel against the generic per-block kernel."""
    from chunkformer_amd.weights import synthetic_features
    g = small_g
    enc = small_models["bf16"]
    lens = g[f"{case}_lens"].tolist()
    C, L, R = (int(v) for v in g[f"{case}_clr"])
    xs = synthetic_features(lens, int(g[f"{case}_seed"]))
    outs = []
    for ring in (1, 0):
        enc.set_option("ring_attention", ring)
        outs.append(enc.forward_parallel_chunk(xs, torch.tensor(lens, dtype=torch.int32), C, L, R)[0].cpu().numpy())
    enc.set_option("ring_attention", 1)
    assert _rel_l2(outs[0], outs[1]) <= 1e-2
    assert _rel_l2(outs[0], g[f"{case}_out"]) <= BF16_RELL2


@pytest.mark.parametrize("clr", [(-1, -1, -1), (16, 0, 16), (64, 0, 0), (0, 0, 0)])
def test_dense_attention_matches_generic(cfm, small_models, clr):
    """bf16 padded plans without left context (full attention, or chunks with right context only):
    the dense kernel (every key staged once per block) against the generic per-block kernel, on
    utterances padded to different lengths (key padding masks, a masked partial last tile)."""
    from chunkformer_amd.weights import synthetic_features
    enc = small_models["bf16"]
    lens = [3000, 1790, 523, 40]
    xs = synthetic_features(lens, 77)
    T = max(lens)
    xp = torch.zeros(len(lens), T, 80)
    for i, t in enumerate(xs):
        xp[i, : t.shape[0]] = t
    outs = []
    for ring in (1, 0):
        enc.set_option("ring_attention", ring)
        y, _ = enc.forward_encoder(xp, torch.tensor(lens, dtype=torch.int32), *clr)
        outs.append(y.float().cpu().numpy())
    enc.set_option("ring_attention", 1)
    for b, t in enumerate(lens):
        n = (t - 15) // 8 + 1
        assert _rel_l2(outs[0][b, :n], outs[1][b, :n]) <= 1e-2, b


def test_masked_batch_rejects_length_mismatch(cfm, small_models):
    """x.size(0) rows and xs_origin_lens whose chunk counts differ: the reference's bound tensors
    then mismatch its windows (encoder.py:567-612, a RuntimeError on shapes); so does this build.
    Equal counts are accepted (test_rows_differ_from_origin_lens)."""
    enc = small_models["fp32"]
    xs = [torch.randn(300, 80), torch.randn(200, 80)]
    with pytest.raises(RuntimeError):
        enc.forward_parallel_chunk(xs, torch.tensor([300, 40], dtype=torch.int32), 16, 32, 32)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rows_differ_from_origin_lens(golden_dir, dtype):
    """forward_parallel_chunk with x.size(0) != xs_origin_lens in both directions (the reference unfolds
    x.size(0) rows and bounds masks / output lengths by xs_origin_lens) against the reference."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.encoder import ChunkFormerEncoder
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    g = np.load(os.path.join(golden_dir, "rows_neq.npz"))
    C, L, R = (int(v) for v in g["clr"])
    enc = ChunkFormerEncoder(SMALL, synthetic_state_dict(SMALL, int(g["seed"])), dtype=dtype)
    # "": rows > xs_origin_lens; "gt_": xs_origin_lens > rows (the masks reach past the real rows)
    for pre in ("", "gt_"):
        xs = synthetic_features(g[pre + "rows"].tolist(), int(g[pre + "feat_seed"]))
        off = torch.zeros(len(xs), dtype=torch.long)
        out, olens, nch, _, _, off2 = enc.forward_parallel_chunk(xs, torch.tensor(g[pre + "lens"]), C, L, R,
                                                                 offset=off)
        assert nch == g[pre + "nchunks"].tolist() and olens.tolist() == g[pre + "outlens"].tolist()
        assert off2.tolist() == g[pre + "outlens"].tolist()
        if dtype == "fp32":
            np.testing.assert_allclose(out.cpu().numpy(), g[pre + "out"], atol=1e-4, rtol=0, err_msg=pre)
        else:
            o = out.cpu().numpy().astype(np.float64)
            assert np.linalg.norm(o - g[pre + "out"]) / np.linalg.norm(g[pre + "out"]) <= 2e-2, pre


@pytest.mark.parametrize("seed", range(12))
def test_random_batches_match_oracle(cfm, small_models, seed):
    """Seeded random masked batches (1-40 utterances of 1-2500 frames, random chunk / context sizes,
    random offsets and carried caches) through the fp32 path against the oracle restatement
    (oracle/encoder_ref.py, itself pinned by the reference fixtures): outputs at 1e-4, lengths,
    chunk counts and the new caches."""
    from oracle import encoder_ref as ref
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    rng = np.random.default_rng(1000 + seed)
    B = int(rng.integers(1, 41))
    lens = [int(v) for v in np.minimum(rng.pareto(1.2, B) * 120 + 1, 2500).astype(int)]
    C = int(rng.choice([4, 8, 16, 24, 32, 64]))
    L, R = int(rng.choice([0, 8, 16, 40, 64])), int(rng.choice([0, 8, 16, 40, 64]))
    caches = B == 1 or seed % 4 == 3
    if caches:   # the cache path is single-utterance (endless_decode / forward_parallel_chunk with caches)
        lens, L = lens[:1], max(L, 16)
    xs = synthetic_features(lens, 500 + seed)
    enc = small_models["fp32"]
    sd = synthetic_state_dict(SMALL, 1)
    # per-utterance start offsets (forward_parallel_chunk's `offset`: masks and positions of a batch resumed
    # mid-stream), random on the cache-free batches too
    offs = [int(v) for v in rng.integers(0, 200, len(lens))]
    kw, rkw = dict(offset=torch.tensor(offs)), dict(offset=offs)
    if caches:
        g = torch.Generator().manual_seed(seed)
        ac = torch.randn(SMALL.num_blocks, L, SMALL.n_heads, 2 * SMALL.head_dim, generator=g) * 0.5
        cc = torch.randn(SMALL.num_blocks, SMALL.d_model, SMALL.conv_lorder, generator=g) * 0.5
        off = int(rng.integers(0, 300))
        trunc = C * int(rng.integers(1, 4))
        kw = dict(att_cache=ac, cnn_cache=cc, truncated_context_size=trunc, offset=torch.tensor([off]))
        rkw = dict(att_cache=ac, cnn_cache=cc, truncated_context_size=trunc, offset=[off])
    out, olens, nch, ra, rc, _ = enc.forward_parallel_chunk(xs, torch.tensor(lens, dtype=torch.int32), C, L, R, **kw)
    eo, el, enc_n, era, erc, _ = ref.forward_parallel_chunk(sd, SMALL, xs, lens, C, L, R, **rkw)
    assert nch == list(enc_n) and olens.tolist() == el.tolist(), (B, C, L, R)
    np.testing.assert_allclose(out.cpu().numpy(), eo.numpy(), atol=FP32_ATOL, rtol=0, err_msg=str((B, C, L, R)))
    if caches:
        np.testing.assert_allclose(ra.cpu().numpy(), era.numpy(), atol=FP32_ATOL, rtol=0)
        np.testing.assert_allclose(rc.cpu().numpy(), erc.numpy(), atol=FP32_ATOL, rtol=0)


@pytest.mark.parametrize("seed", range(4))
def test_random_large_batches_match_oracle(cfm, large, seed):
    """chunkformer-large (the fast kernels: ring attention, weight-stationary GEMMs, channel-stationary
    front-end) on seeded random masked batches with random C in {16..64}, L, R in {0..128}: fp32 at
    1e-4, bf16 and fp16 at their rel-L2 bars, against the oracle."""
    from oracle import encoder_ref as ref
    from chunkformer_amd.config import LARGE
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    g, models = large
    rng = np.random.default_rng(2000 + seed)
    B = int(rng.integers(1, 13))
    lens = [int(v) for v in rng.integers(1, 1500, B)]
    C = int(rng.choice([16, 32, 48, 64]))
    L, R = int(rng.choice([0, 32, 64, 128])), int(rng.choice([0, 32, 64, 128]))
    xs = synthetic_features(lens, 700 + seed)
    sd = synthetic_state_dict(LARGE, int(g["seed"]))
    eo, el, enc_n, _, _, _ = ref.forward_parallel_chunk(sd, LARGE, xs, lens, C, L, R)
    exp = eo.numpy()
    for dt in ("fp32", "bf16", "fp16"):
        out, olens, nch, _, _, _ = models[dt].forward_parallel_chunk(xs, torch.tensor(lens, dtype=torch.int32), C, L, R)
        assert nch == list(enc_n) and olens.tolist() == el.tolist()
        o = out.cpu().numpy()
        assert np.isfinite(o).all()
        if dt == "fp32":
            np.testing.assert_allclose(o, exp, atol=FP32_ATOL, rtol=0, err_msg=str((B, C, L, R)))
        else:
            assert _rel_l2(o, exp) <= RELL2[dt], (dt, B, C, L, R)


@pytest.mark.parametrize("seed", range(8))
def test_random_padded_batches_match_oracle(cfm, small_models, seed):
    """The padded path (forward_encoder) on seeded random batches: chunked (random C, L, R) and full
    attention, utterances of 1-1500 frames, fp32 at 1e-4 and the masks exact, against the oracle."""
    from oracle import encoder_ref as ref
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    rng = np.random.default_rng(3000 + seed)
    B = int(rng.integers(1, 9))
    lens = [int(v) for v in rng.integers(1, 1500, B)]
    C = 0 if seed % 4 == 0 else int(rng.choice([4, 8, 16, 32]))
    L, R = (0, 0) if C == 0 else (int(rng.choice([0, 8, 16, 40])), int(rng.choice([0, 8, 16, 40])))
    xs = synthetic_features(lens, 900 + seed)
    xp = torch.zeros(B, max(lens), 80)
    for i, t in enumerate(xs):
        xp[i, : t.shape[0]] = t
    sd = synthetic_state_dict(SMALL, 1)
    y, masks = ref.forward_encoder(sd, SMALL, xp, lens, C, L, R)
    out, m = small_models["fp32"].forward_encoder(xp, torch.tensor(lens), C, L, R)
    np.testing.assert_array_equal(m.cpu().numpy(), masks.numpy())
    np.testing.assert_allclose(out.cpu().numpy(), y.numpy(), atol=FP32_ATOL, rtol=0, err_msg=str((B, C, L, R)))


def test_model_options_kept_and_retired(cfm):
    """cfm_model_set_option: the keys of the retired kernel variants are unknown options (ValueError), every
    key that tests, the Python package or a kernel still read is accepted at its default value.  On a model of
    its own (SMALL: d = 128, 2 layers), so no other test sees the writes."""
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.weights import synthetic_state_dict
    enc = cfm.ChunkFormerEncoder(SMALL, synthetic_state_dict(SMALL, 1), dtype="bf16")
    for key in ("attn128_var", "conv_dot2", "conv_dma", "attn_reuse"):
        with pytest.raises(ValueError, match="unknown option"):
            enc.set_option(key, 1)
    defaults = {"ring_attention": 1, "fe_conv": 6, "fe_fuse_dw2": 1, "gemm_wst": 1, "fe_group_windows": 0,
                "wsp_small_div": 1, "wsp_small_rows": 32768, "attn_min_chunks": 2, "gemm_big_min": 0,
                "cache_fuse": 1, "ctc_fused": 1, "trim_right": 0, "fe_carry": 0, "fe_reuse": 0, "fe_save_from": -1,
                "profile": 0, "profile_reset": 0, "max_layers": -1,
                "nt_sites": 8, "store_mode": 0, "col_group": 0, "dw2_seg": 4, "attn_diag": 0, "gemm_diag": 0}
    for key, value in defaults.items():
        enc.set_option(key, value)
