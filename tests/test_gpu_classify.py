"""GPU: the classification consumer (csrc/classify.hip, cfm_cls_*, chunkformer_amd/classifier.py and
ChunkFormerModel.classify / classify_audio / batch_classify).

Op level: the masked mean pool against the fp64 mean of the same f32 input within a derived
worst-case summation bound, and the heads against fp64 numpy on the pooled vector the device returned.
Model level: parity with the reference's SpeechClassificationModel through the fixture
tests/golden/classification.npz (gen_golden_classification.py), fp32 within the project's fp32 bar,
bf16 / fp16 pooled vectors within the project's rel-L2 bars of the encoder output.

The pool's bound: the kernel sums a column over 64-row slabs (CLS_SLAB); in a 256-thread workgroup
G = 256 // (d // 4) row groups each add every G-th row of the slab in order (ceil(64 / G) terms), the
G group sums are added in order (G - 1 additions), and the finish kernel adds the
P = ceil(len / 64) slab partials the same way (ceil(P / G) + G - 1).  One element passes through at
most  h = ceil(64 / G) + (G - 1) + ceil(P / G) + (G - 1)  f32 additions, then one division; a sum
evaluated with chains of at most h roundings has |err| <= ((1 + u)^h - 1) sum|x|, u = 2^-24, so with
n_adds = h + 2 (the division, and one unit for the second-order terms, h u < 1e-4)
|pooled - mean| <= n_adds * 2^-24 * mean_rows|x| per column.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FP32_ATOL = 1e-4                       # tests/test_gpu_parity.py:19
RELL2 = {"bf16": 2e-2, "fp16": 5e-3}   # tests/test_gpu_parity.py:20-21
SLAB, THREADS = 64, 256                # CLS_SLAB, CLS_THREADS of csrc/classify.hip
U = 2.0 ** -24


def n_adds(length: int, d: int) -> int:
    G = max(1, THREADS // (d // 4))
    P = -(-length // SLAB)
    return -(-SLAB // G) + (G - 1) + -(-P // G) + (G - 1) + 2


@pytest.fixture(scope="module")
def cls():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import chunkformer_amd.classifier as c
    return c


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "classification.npz"))


def _layout(lens, gaps, d, seed, tail=37):
    """enc [rows, d] f32: utterance b's rows are N(0.8, 1) (a common mean like an encoder's), every gap
    row and everything after the last region NaN.  Returns (enc, row_start)."""
    starts, at = [], 0
    for n, gap in zip(lens, gaps):
        at += gap
        starts.append(at)
        at += n
    rows = at + tail
    g = torch.Generator().manual_seed(seed)
    enc = torch.full((rows, d), float("nan"))
    for s, n in zip(starts, lens):
        enc[s: s + n] = torch.randn(n, d, generator=g) + 0.8
    return enc, starts


def _check_pool(cls, enc, starts, lens):
    d = enc.shape[1]
    dev = enc.cuda()
    pooled = cls.masked_mean_pool(dev, starts, lens)
    again = cls.masked_mean_pool(dev, starts, lens)
    assert torch.equal(pooled, again), "two calls on the same input differ"
    got = pooled.cpu().numpy().astype(np.float64)
    x = enc.numpy().astype(np.float64)
    worst = 0.0
    for b, (s, n) in enumerate(zip(starts, lens)):
        if n == 0:
            assert (pooled[b] == 0).all() and not torch.signbit(pooled[b]).any(), "row_len 0 must give exact zeros"
            continue
        seg = x[s: s + n]
        bound = n_adds(n, d) * U * np.abs(seg).mean(0)
        err = np.abs(got[b] - seg.mean(0))
        worst = max(worst, float((err / bound).max()))
        assert np.isfinite(got[b]).all(), f"utterance {b} (len {n}): a gap row was summed"
        assert (err <= bound).all(), f"utterance {b} (len {n}): err/bound {float((err / bound).max()):.3f}"
    print(f"pool d={d} B={len(lens)}: worst err/bound {worst:.3f}")


EDGE_LENS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099, 127, 128, 129]
EDGE_GAPS = [0, 70, 0, 1, 13, 0, 64, 5, 33, 70, 2, 0, 47, 9]


@pytest.mark.parametrize("d", [128, 256, 512])
def test_pool_edge_lengths(cls, d):
    enc, starts = _layout(EDGE_LENS, EDGE_GAPS, d, seed=d)
    _check_pool(cls, enc, starts, EDGE_LENS)


@pytest.mark.parametrize("d", [128, 256, 512])
def test_pool_single_row(cls, d):
    enc, starts = _layout([1], [3], d, seed=1)
    _check_pool(cls, enc, starts, [1])
    enc, starts = _layout([1], [0], d, seed=2, tail=0)   # the whole input is the one row
    _check_pool(cls, enc, starts, [1])


def test_pool_skewed_batch(cls):
    """one 20,000-row utterance between thirty of 1 .. 50 rows: slabs, not utterances, are the unit of work"""
    rng = np.random.default_rng(5)
    short = rng.integers(1, 51, size=30).tolist()
    lens = short[:11] + [20000] + short[11:]
    gaps = rng.integers(0, 71, size=len(lens)).tolist()
    enc, starts = _layout(lens, gaps, 512, seed=9)
    _check_pool(cls, enc, starts, lens)


def test_pool_other_widths_and_bad_args(cls):
    for d in (4, 100, 1024):   # any multiple of 4 up to 1024
        enc, starts = _layout([1, 70, 300], [2, 0, 5], d, seed=d)
        _check_pool(cls, enc, starts, [1, 70, 300])
    enc = torch.zeros(10, 128).cuda()
    with pytest.raises(ValueError):
        cls.masked_mean_pool(enc, [8], [3])          # past the last row
    with pytest.raises(ValueError):
        cls.masked_mean_pool(enc, [-1], [3])
    with pytest.raises(ValueError):
        cls.masked_mean_pool(torch.zeros(10, 126).cuda(), [0], [3])   # width not a multiple of 4
    with pytest.raises(ValueError):
        cls.masked_mean_pool(torch.zeros(10, 1028).cuda(), [0], [3])


# ----------------------------------------------------------------------------- heads, op level
def _heads(cls, tasks, d, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    a = scale / math.sqrt(d)
    for name, n in tasks.items():
        sd[f"classification_heads.{name}.linear.weight"] = (torch.rand(n, d, generator=g) * 2 - 1) * a
        sd[f"classification_heads.{name}.linear.bias"] = (torch.rand(n, generator=g) * 2 - 1) * a
    return sd


def _check_heads(cls, tasks, sd, enc, starts, lens, expect_pred=None):
    """pooled, logits, pred, prob of one classify call against fp64 numpy on the returned pooled vectors."""
    d = enc.shape[-1]
    cfg = cls.ClassifierConfig(tasks=dict(tasks), enc_dim=d)
    heads = cls.ClassifierHeads(cfg, sd, "cuda:0")
    pooled, logits, pred, prob = heads.classify(enc, starts, lens)
    assert torch.equal(pooled, heads.pool(enc, starts, lens)), "classify and pool disagree on the pooled vectors"
    again = heads.classify(enc, starts, lens)
    assert all(torch.equal(a, b) for a, b in zip((pooled, logits, pred, prob), again))
    assert pred.dtype == torch.int32 and tuple(pred.shape) == (len(lens), len(tasks))
    p64 = pooled.cpu().numpy().astype(np.float64)
    parts = heads.split_logits(logits)
    worst_l = worst_p = 0.0
    for t, (name, n) in enumerate(tasks.items()):
        W = sd[f"classification_heads.{name}.linear.weight"].numpy().astype(np.float64)
        bias = sd[f"classification_heads.{name}.linear.bias"].numpy().astype(np.float64)
        ref = p64 @ W.T + bias
        got = parts[name].cpu().numpy().astype(np.float64)
        bound = 2.0 ** -23 * d * np.abs(W).max() * np.abs(p64).max()
        worst_l = max(worst_l, float(np.abs(got - ref).max() / bound))
        assert np.abs(got - ref).max() <= bound, f"{name}: logits off by {np.abs(got - ref).max():.3e} > {bound:.3e}"
        ids = pred[:, t].cpu().numpy()
        ref_ids = ref.argmax(-1)
        if n > 1:
            top = np.sort(ref, -1)
            clear = (top[:, -1] - top[:, -2]) > 2 * bound
        else:
            clear = np.ones(len(lens), bool)
        np.testing.assert_array_equal(ids[clear], ref_ids[clear], err_msg=name)
        assert ((0 <= ids) & (ids < n)).all()
        sm = np.exp(ref - ref.max(-1, keepdims=True))
        sm /= sm.sum(-1, keepdims=True)
        ref_p = sm[np.arange(len(lens)), ref_ids]
        got_p = prob[:, t].cpu().numpy().astype(np.float64)
        rel = np.abs(got_p[clear] - ref_p[clear]) / ref_p[clear]
        worst_p = max(worst_p, float(rel.max()) if rel.size else 0.0)
        assert (rel <= 1e-6).all(), f"{name}: probability off by {rel.max():.3e} relative"
        if n == 1:
            assert (ids == 0).all() and (got_p == 1.0).all()
        if expect_pred is not None and name in expect_pred:
            assert ids.tolist() == expect_pred[name]
    print(f"heads {list(tasks.values())} d={d}: logits err/bound {worst_l:.3f}, probability rel err {worst_p:.2e}")
    return pooled, logits, pred, prob


HEAD_LENS = [1, 40, 64, 65, 300, 7]
HEAD_GAPS = [0, 5, 0, 70, 3, 11]


@pytest.mark.parametrize("tasks,d", [({"gender": 2, "emotion": 7, "region": 5}, 128),
                                     ({"one": 1, "many": 1000, "few": 3}, 512),
                                     ({"gender": 2, "emotion": 7, "region": 5}, 256)])
def test_heads_op_level(cls, tasks, d):
    enc, starts = _layout(HEAD_LENS, HEAD_GAPS, d, seed=3 + d)
    _check_heads(cls, tasks, _heads(cls, tasks, d, seed=d), enc.cuda(), starts, HEAD_LENS)


def test_heads_tie_gives_lower_index(cls):
    tasks, d = {"a": 6, "b": 4}, 128
    sd = _heads(cls, tasks, d, seed=1)
    w, b = sd["classification_heads.a.linear.weight"], sd["classification_heads.a.linear.bias"]
    w[4] = w[2]
    b[2] = b[4] = 5.0       # rows 2 and 4 give the same logit, far above the others (|logit| < 1)
    enc, starts = _layout(HEAD_LENS, HEAD_GAPS, d, seed=8)
    _, logits, pred, prob = _check_heads(cls, tasks, sd, enc.cuda(), starts, HEAD_LENS)
    assert torch.equal(logits[:, 2], logits[:, 4])
    assert pred[:, 0].tolist() == [2] * len(HEAD_LENS)
    l64 = logits[:, :6].cpu().numpy().astype(np.float64)
    ref_p = 1.0 / np.exp(l64 - l64[:, 2:3]).sum(-1)
    np.testing.assert_allclose(prob[:, 0].cpu().numpy(), ref_p, rtol=1e-6)
    assert (ref_p < 0.5).all() and (ref_p > 0.45).all()   # two equal winners share nearly all the mass


def test_heads_limits(cls):
    d = 128
    many = {f"t{i}": 2 for i in range(17)}
    with pytest.raises(ValueError):
        cls.ClassifierHeads(cls.ClassifierConfig(tasks=many, enc_dim=d), _heads(cls, many, d, 0), "cuda:0")
    big = {"big": 1025}
    with pytest.raises(ValueError):
        cls.ClassifierHeads(cls.ClassifierConfig(tasks=big, enc_dim=d), _heads(cls, big, d, 0), "cuda:0")
    total = {f"t{i}": 1024 for i in range(5)}   # 5120 classes in total
    with pytest.raises(ValueError):
        cls.ClassifierHeads(cls.ClassifierConfig(tasks=total, enc_dim=d), _heads(cls, total, d, 0), "cuda:0")
    ok = {"a": 2, "b": 3}
    sd = _heads(cls, ok, d, 0)
    del sd["classification_heads.b.linear.bias"]
    with pytest.raises(ValueError):
        cls.ClassifierHeads(cls.ClassifierConfig(tasks=ok, enc_dim=d), sd, "cuda:0")
    sd = _heads(cls, ok, d, 0)
    sd["classification_heads.a.linear.weight"] = sd["classification_heads.a.linear.weight"][:, :-4]
    with pytest.raises(ValueError):
        cls.ClassifierHeads(cls.ClassifierConfig(tasks=ok, enc_dim=d), sd, "cuda:0")
    sixteen = {f"t{i}": 1 + i for i in range(16)}   # the limit itself is accepted
    cls.ClassifierHeads(cls.ClassifierConfig(tasks=sixteen, enc_dim=d), _heads(cls, sixteen, d, 0), "cuda:0")


# ----------------------------------------------------------------------------- reference parity
def _fixture_state_dict(fx):
    import dataclasses

    from chunkformer_amd.config import SMALL
    from chunkformer_amd.weights import synthetic_state_dict
    cfg = dataclasses.replace(SMALL, vocab=0)
    sd = synthetic_state_dict(cfg, int(fx["seed"]))
    tasks = {str(n): int(c) for n, c in zip(fx["task_names"], fx["task_classes"])}
    for n in tasks:
        sd[f"classification_heads.{n}.linear.weight"] = torch.from_numpy(fx[f"w_{n}"])
        sd[f"classification_heads.{n}.linear.bias"] = torch.from_numpy(fx[f"b_{n}"])
    return cfg, sd, tasks


@pytest.fixture(scope="module")
def models(cls, fx):
    from chunkformer_amd.model import ChunkFormerModel
    cfg, sd, tasks = _fixture_state_dict(fx)
    return {dt: ChunkFormerModel(cfg, sd, dtype=dt, model_type="classification", tasks=tasks)
            for dt in ("fp32", "bf16", "fp16")}


@pytest.fixture(scope="module")
def utts(fx):
    from chunkformer_amd.weights import synthetic_features
    return synthetic_features(fx["lens"].tolist(), int(fx["feat_seed"]))


def _logit_bar(fx, name):
    return FP32_ATOL * float(np.abs(fx[f"w_{name}"]).sum(1).max()) + 1e-6


def _check_against_fixture(fx, geo, tasks, pooled, logits_by_task, pred_by_task, prob_by_task):
    err = np.abs(pooled - fx[f"{geo}_pooled"]).max()
    print(f"{geo}: max|pooled - reference| = {err:.2e}")
    assert err <= FP32_ATOL
    for n in tasks:
        bar = _logit_bar(fx, n)
        if logits_by_task is not None:
            lerr = np.abs(logits_by_task[n] - fx[f"{geo}_logits_{n}"]).max()
            print(f"{geo}/{n}: max|logits - reference| = {lerr:.2e} (bar {bar:.2e})")
            assert lerr <= bar
        np.testing.assert_array_equal(pred_by_task[n], fx[f"{geo}_prediction_{n}"], err_msg=f"{geo}/{n}")
        perr = np.abs(prob_by_task[n] - fx[f"{geo}_probability_{n}"]).max()
        assert perr <= bar, f"{geo}/{n}: probability off by {perr:.3e}"


@pytest.mark.parametrize("geo", ["full", "chunk"])
def test_classify_padded_matches_reference(models, fx, utts, geo):
    m = models["fp32"]
    C, L, R = (-1, -1, -1) if geo == "full" else (int(v) for v in fx["chunk_clr"])
    xs = torch.nn.utils.rnn.pad_sequence(utts, batch_first=True)
    res = m.classify(xs, torch.from_numpy(fx["lens"]), C, L, R)
    tasks = m.get_tasks()
    assert list(tasks.items()) == [("gender", 2), ("emotion", 7), ("region", 5)]
    pooled, logits = m.last_classification
    parts = m.get_classification_heads().split_logits(logits)
    for n in tasks:
        assert res[f"{n}_prediction"].dtype == torch.int64 and res[f"{n}_prediction"].is_cuda
        assert res[f"{n}_probability"].dtype == torch.float32 and tuple(res[f"{n}_probability"].shape) == (len(utts),)
    _check_against_fixture(fx, geo, tasks, pooled.cpu().numpy(), {n: parts[n].cpu().numpy() for n in tasks},
                           {n: res[f"{n}_prediction"].cpu().numpy() for n in tasks},
                           {n: res[f"{n}_probability"].cpu().numpy() for n in tasks})


def test_batch_classify_matches_reference(models, fx, utts):
    m = models["fp32"]
    C, L, R = (int(v) for v in fx["chunk_clr"])
    tasks = m.get_tasks()
    one = m.batch_classify(utts, C, L, R, total_batch_duration=1800)          # one packed group
    pooled, logits = m.last_classification
    parts = m.get_classification_heads().split_logits(logits)
    _check_against_fixture(fx, "packed", tasks, pooled.cpu().numpy(), {n: parts[n].cpu().numpy() for n in tasks},
                           {n: np.array([r[n]["label_id"] for r in one]) for n in tasks},
                           {n: np.array([r[n]["prob"] for r in one], np.float32) for n in tasks})
    from chunkformer_amd.model import budget_groups
    assert len(budget_groups(fx["lens"].tolist(), 16)) == 2
    two = m.batch_classify(utts, C, L, R, total_batch_duration=16)            # two groups, input order kept
    assert len(two) == len(utts)
    _check_against_fixture(fx, "packed", tasks, pooled.cpu().numpy(), None,
                           {n: np.array([r[n]["label_id"] for r in two]) for n in tasks},
                           {n: np.array([r[n]["prob"] for r in two], np.float32) for n in tasks})
    assert all(r[n]["label"] == str(r[n]["label_id"]) for r in one for n in tasks)


def test_batch_classify_rejects_too_short(models, utts):
    with pytest.raises(ValueError, match="input 1"):
        models["fp32"].batch_classify([utts[0], torch.zeros(6, 80)], 8, 16, 8)


def test_classify_audio(models, fx, utts, tmp_path):
    m = models["fp32"]
    i = 0   # the longest utterance: unpadded in the fixture's batch too, so the fixture's row is this very run
    assert m.label_mapping is None
    plain = m.classify_audio(utts[i])
    C, L, R = (int(v) for v in fx["chunk_clr"])
    chunked = m.classify_audio(utts[i], C, L, R)
    p = str(tmp_path / "utt.npy")
    np.save(p, utts[i].numpy())
    from_file = m.classify_audio(p)
    assert all(from_file[n]["label_id"] == plain[n]["label_id"] and
               abs(from_file[n]["prob"] - plain[n]["prob"]) <= 1e-6 for n in plain)
    m.label_mapping = {"gender": {"0": "female", "1": "male"}, "emotion": {"0": "neutral"}}
    try:
        named = m.classify_audio(utts[i])
    finally:
        m.label_mapping = None
    for n in m.get_tasks():
        for geo, got in (("full", plain), ("chunk", chunked)):
            assert set(got[n]) == {"label", "label_id", "prob"}
            assert got[n]["label_id"] == int(fx[f"{geo}_prediction_{n}"][i])
            assert got[n]["label"] == str(got[n]["label_id"]) and isinstance(got[n]["prob"], float)
            assert abs(got[n]["prob"] - float(fx[f"{geo}_probability_{n}"][i])) <= _logit_bar(fx, n)
        assert named[n]["label_id"] == plain[n]["label_id"] and abs(named[n]["prob"] - plain[n]["prob"]) <= 1e-6
    gid, eid = plain["gender"]["label_id"], plain["emotion"]["label_id"]
    assert named["gender"]["label"] == {0: "female", 1: "male"}[gid]
    assert named["emotion"]["label"] == ("neutral" if eid == 0 else str(eid))   # id missing from the mapping
    assert named["region"]["label"] == str(plain["region"]["label_id"])         # task missing from the mapping


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_pooled_and_heads(cls, models, fx, utts, dtype):
    m = models[dtype]
    xs = torch.nn.utils.rnn.pad_sequence(utts, batch_first=True)
    lens = torch.from_numpy(fx["lens"])
    for geo, (C, L, R) in (("full", (-1, -1, -1)), ("chunk", tuple(int(v) for v in fx["chunk_clr"]))):
        m.classify(xs, lens, C, L, R)
        pooled = m.last_classification[0].cpu().numpy().astype(np.float64)
        ref = fx[f"{geo}_pooled"].astype(np.float64)
        rel = float(np.linalg.norm(pooled - ref) / np.linalg.norm(ref))
        print(f"{dtype} {geo}: pooled rel-L2 {rel:.2e}")
        assert rel <= RELL2[dtype]
    # predictions are not compared end to end in 16 bit (the allowed encoder error exceeds the fixture's
    # margins): the op-level head check runs on this encoder's output instead
    out, out_lens = m.encode(xs, lens)
    B, Tp, d = out.shape
    tasks = {"gender": 2, "emotion": 7, "region": 5}
    _check_heads(cls, tasks, _heads(cls, tasks, d, seed=17), out.reshape(B * Tp, d), [b * Tp for b in range(B)],
                 out_lens.tolist())


# ----------------------------------------------------------------------------- loading
ENCODER_CONF = {"output_size": 128, "attention_heads": 2, "linear_units": 256, "num_blocks": 2,
                "cnn_module_kernel": 15, "cnn_module_norm": "layer_norm", "dynamic_conv": True,
                "input_layer": "dw_striding", "pos_enc_layer_type": "chunk_rel_pos",
                "selfattention_layer_type": "chunk_rel_seflattn", "activation_type": "swish"}


def test_from_pretrained_classification_dir(cls, fx, utts, tmp_path):
    import yaml

    from chunkformer_amd.model import ChunkFormerModel
    cfg, sd, tasks = _fixture_state_dict(fx)
    path = str(tmp_path)
    conf = {"encoder": "chunkformer", "encoder_conf": ENCODER_CONF, "input_dim": 80, "model": "classification",
            "model_conf": {"tasks": dict(tasks), "dropout_rate": 0.1}}
    with open(os.path.join(path, "config.yaml"), "w") as f:
        yaml.safe_dump(conf, f, sort_keys=False)
    with open(os.path.join(path, "global_cmvn"), "w") as f:   # the checkpoint's own CMVN buffers win over it
        json.dump({"mean_stat": [0.0] * 80, "var_stat": [1.0] * 80, "frame_num": 1.0}, f)
    torch.save(dict(sd), os.path.join(path, "pytorch_model.bin"))
    mapping = {"gender": {"0": "female", "1": "male"}, "region": {str(i): f"r{i}" for i in range(5)}}
    with open(os.path.join(path, "label_mapping.json"), "w") as f:
        json.dump(mapping, f)
    m = ChunkFormerModel.from_pretrained(path, dtype="fp32")
    assert m.is_classification and m.model_type == "classification" and m.config.vocab == 0
    assert list(m.get_tasks().items()) == list(tasks.items()) and m.label_mapping == mapping
    assert m.get_classification_heads() is m.classifier
    xs = torch.nn.utils.rnn.pad_sequence(utts, batch_first=True)
    res = m.classify(xs, torch.from_numpy(fx["lens"]))
    for n in tasks:
        np.testing.assert_array_equal(res[f"{n}_prediction"].cpu().numpy(), fx[f"full_prediction_{n}"])
    got = m.classify_audio(utts[0])
    assert got["gender"]["label"] == mapping["gender"][str(int(fx["full_prediction_gender"][0]))]
    assert got["emotion"]["label"] == str(int(fx["full_prediction_emotion"][0]))
    out, out_lens = m.encode(xs, torch.from_numpy(fx["lens"]))     # encode works unchanged
    assert tuple(out.shape[::2]) == (len(utts), 128) and out_lens.tolist() == fx["packed_out_lens"].tolist()
    with pytest.raises(ValueError):
        m.endless_decode(utts[0])
    with pytest.raises(ValueError):
        m.batch_decode([utts[0]])
    # a classification config without tasks is refused like init_model.py:109-111
    conf["model_conf"] = {"tasks": {}}
    with open(os.path.join(path, "config.yaml"), "w") as f:
        yaml.safe_dump(conf, f)
    with pytest.raises(ValueError):
        ChunkFormerModel.from_pretrained(path, dtype="fp32")


def test_classify_on_other_model_types_raises(cls, utts):
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.transducer import RNNTConfig, synthetic_transducer_state_dict
    from chunkformer_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(SMALL, 1)
    asr = ChunkFormerModel(SMALL, sd, dtype="fp32")
    rc = RNNTConfig(vocab=SMALL.vocab, enc_dim=SMALL.d_model, hidden=256, num_layers=1, embed_size=128, pred_out=256,
                    join_dim=384)
    rnnt = ChunkFormerModel(SMALL, {**sd, **synthetic_transducer_state_dict(rc, 1)}, dtype="fp32",
                            model_type="transducer", rnnt_config=rc)
    msg = "This model is not a classification model. Use ASR decoding methods instead."
    for m in (asr, rnnt):
        assert not m.is_classification and m.get_tasks() is None and m.get_classification_heads() is None
        with pytest.raises(ValueError, match=msg):
            m.classify_audio(utts[0])
        with pytest.raises(ValueError, match=msg):
            m.classify(utts[0].unsqueeze(0), torch.tensor([utts[0].shape[0]]))
        with pytest.raises(ValueError, match=msg):
            m.batch_classify([utts[0]])
    with pytest.raises(ValueError):
        ChunkFormerModel(SMALL, sd, dtype="fp32", model_type="classification")   # no tasks
