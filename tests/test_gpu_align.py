"""CTC forced alignment on the device (csrc/ctc_align.hip) against the host restatement
(align.force_align_host, itself checked against enumeration in test_align_cpu.py).

Host and kernel consume the same f32 log-probs and do the same f64 operations in the same order, so
frames, spans, frame log-probs, status and score are compared bit for bit: there is no tolerance.
Covered: both sides of the 16-state backpointer word, one and several strips per workgroup with the
labels in registers (1, 2 and 3 runs per thread) and in the generic strip loop, the alpha rows in LDS
and in the workspace (either side of the 8192-state threshold, and forced at a small size), packed
batches with gaps, non-finite log-probs, the argument checks, and the model-level entry points."""
import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V32 = 32
_HOST = {}


@pytest.fixture(scope="module")
def align():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import align
    return align


def _case(T, L, seed, V=V32, blank=0):
    """Seeded log-softmax rows [T, V] and a random target without the blank."""
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(T, V, generator=g) * 2, dim=-1)
    toks = torch.tensor([v for v in range(V) if v != blank])
    y = toks[torch.randint(0, V - 1, (L,), generator=g)].tolist()
    return lp, y


def _host(align, key, lp, y, blank=0):
    """(status, AlignResult) of the host restatement, computed once per case."""
    if key not in _HOST:
        _HOST[key] = align.align_host_status(lp, y, blank)
    return _HOST[key]


def _pack(cases, gap=0, lead=0, V=V32):
    starts, rows = [], lead
    for lp, _ in cases:
        starts.append(rows)
        rows += lp.shape[0] + gap
    x = torch.full((max(rows, 1), V), float("nan"))
    for s0, (lp, _) in zip(starts, cases):
        x[s0:s0 + lp.shape[0]] = lp
    return x, starts, [lp.shape[0] for lp, _ in cases]


def _check(align, raw, starts, lens, expected):
    """Every utterance of a raw device result equals its host (status, result), bit for bit."""
    res = align.results_from_raw(raw, starts, lens)
    assert raw["status"].tolist() == [st for st, _ in expected]
    for b, ((st, exp), got) in enumerate(zip(expected, res)):
        if st != 0:
            assert got is None
            continue
        assert got.frames == exp.frames, b
        assert got.spans == exp.spans, b
        assert got.frame_logp == exp.frame_logp, b
        assert got.score == exp.score, (b, got.score, exp.score)


SMALL = [(1, 0), (1, 1), (5, 0), (2, 1), (16, 7), (17, 8), (40, 15), (40, 16)]


def test_small_shapes_and_the_word_boundary(align):
    """(T, L) down to one frame; S = 15 / 17 / 31 / 33 lie either side of the 16-state word."""
    cases = [_case(T, L, 100 + i) for i, (T, L) in enumerate(SMALL)]
    assert {2 * L + 1 for _, L in SMALL} >= {15, 17, 31, 33}
    exp = [_host(align, ("small", i), lp, y) for i, (lp, y) in enumerate(cases)]
    assert all(st == 0 for st, _ in exp)
    for i, c in enumerate(cases):                      # one utterance per call
        x, starts, lens = _pack([c])
        _check(align, align.align_packed_device_raw(x.cuda(), starts, lens, [c[1]]), starts, lens, [exp[i]])
    x, starts, lens = _pack(cases, gap=3, lead=2)      # and all of them in one
    _check(align, align.align_packed_device_raw(x.cuda(), starts, lens, [y for _, y in cases]), starts, lens, exp)


def test_single_possible_path_with_repeats(align):
    y = [3, 3, 5, 5, 5, 2, 2, 9, 4, 4, 4, 4, 7, 1, 1, 6, 6, 8]
    R = sum(1 for a, b in zip(y[1:], y[:-1]) if a == b)
    lp, _ = _case(len(y) + R, 0, 7)
    st, exp = _host(align, "tight", lp, y)
    assert st == 0 and align.remove_duplicates_and_blank(exp.frames) == y and exp.frames.count(0) == R
    x, starts, lens = _pack([(lp, y)])
    _check(align, align.align_packed_device_raw(x.cuda(), starts, lens, [y]), starts, lens, [(st, exp)])
    # one frame fewer: infeasible on both
    raw = align.align_packed_device_raw(x[:-1].cuda(), [0], [lp.shape[0] - 1], [y])
    assert raw["status"].tolist() == [1] == [align.align_host_status(lp[:-1], y)[0]]


# (T, L, lds_max_states, generic_strips): runs = ceil((2L + 1) / 16) over 512 threads
LONG = {
    "lds_257_runs": (2300, 2049, -1, False),
    "workspace_rows_forced": (2300, 2049, 0, False),
    "generic_loop": (2300, 2049, -1, True),
    "lds_at_threshold_8191": (4300, 4095, -1, False),
    "workspace_above_threshold_8195_two_strips": (4300, 4097, -1, False),
    "generic_loop_two_strips_workspace": (4300, 4097, 0, True),
    "three_strips": (8500, 8200, -1, False),
}


@pytest.mark.parametrize("name", list(LONG))
def test_long_targets_every_path(align, name):
    T, L, lds, generic = LONG[name]
    lp, y = _case(T, L, 1000 + L)
    st, exp = _host(align, ("long", T, L), lp, y)
    assert st == 0 and align.remove_duplicates_and_blank(exp.frames) == y
    x, starts, lens = _pack([(lp, y)])
    raw = align.align_packed_device_raw(x.cuda(), starts, lens, [y], lds_max_states=lds, generic_strips=generic)
    _check(align, raw, starts, lens, [(st, exp)])


def test_non_zero_blank(align):
    cases = [_case(T, L, 300 + i, blank=3) for i, (T, L) in enumerate([(40, 15), (33, 16), (9, 0), (50, 21)])]
    assert all(3 not in y for _, y in cases)
    exp = [_host(align, ("blank3", i), lp, y, 3) for i, (lp, y) in enumerate(cases)]
    assert all(st == 0 for st, _ in exp) and exp[2][1].frames == [3] * 9
    x, starts, lens = _pack(cases, gap=1)
    raw = align.align_packed_device_raw(x.cuda(), starts, lens, [y for _, y in cases], blank_id=3)
    _check(align, raw, starts, lens, exp)
    # the same rows with blank 0: a target that holds token 0 is refused, one that holds 3 is not
    raw0 = align.align_packed_device_raw(x.cuda(), starts[:2], lens[:2], [[1, 0, 2], [1, 3, 2]], blank_id=0)
    assert raw0["status"].tolist() == [3, 0]


def test_real_head_v5000(align):
    """Log-probs of the one-block d512 / V = 5000 synthetic head at T = 300: the collapsed argmax as
    target (its alignment is the argmax path wherever that is a valid path) and a random target."""
    from chunkformer_amd.config import LARGE
    from chunkformer_amd.encoder import ChunkFormerEncoder
    from chunkformer_amd.weights import synthetic_state_dict
    cfg = dataclasses.replace(LARGE, num_blocks=1)
    assert cfg.vocab == 5000
    enc = ChunkFormerEncoder(cfg, synthetic_state_dict(cfg, 5), dtype="fp32")
    g = torch.Generator().manual_seed(21)
    hs = (torch.randn(300, cfg.d_model, generator=g) * 2).to(enc.device)
    logp, ids = enc.ctc_log_softmax(hs)
    greedy = align.remove_duplicates_and_blank(ids.cpu().tolist())
    rand = torch.randint(1, 5000, (90,), generator=g).tolist()
    lp_h = logp.cpu()
    for name, y in (("greedy", greedy), ("random", rand)):
        st, exp = _host(align, ("v5000", name), lp_h, y)
        assert st == 0
        raw = align.align_packed_device_raw(logp, [0], [300], [y])
        _check(align, raw, [0], [300], [(st, exp)])
    # the reference's signature on the device tensor
    assert align.force_align(logp, torch.tensor(rand), blank_id=0) == _HOST[("v5000", "random")][1].frames


def _packed_batch():
    shapes = [(37, 9), (0, 0), (120, 33), (6, 5), (64, 31)]      # (6, 5): infeasible once it repeats
    cases = [_case(T, L, 500 + i) for i, (T, L) in enumerate(shapes)]
    cases[3] = (cases[3][0], [4, 4, 4, 9, 2])                     # 5 tokens + 2 repeats > 6 frames
    return cases


def _bits(raw):
    return [raw["frames"], raw["frame_logp"].view(torch.int32), raw["spans"], raw["score"].view(torch.int64),
            raw["status"]]


def test_packed_batch_gaps_sentinels_and_determinism(align):
    cases = _packed_batch()
    exp = [_host(align, ("packed", i), lp, y) for i, (lp, y) in enumerate(cases)]
    assert [st for st, _ in exp] == [0, 0, 0, 1, 0]
    x, starts, lens = _pack(cases, gap=5, lead=3)
    tg = [y for _, y in cases]
    raw = align.align_packed_device_raw(x.cuda(), starts, lens, tg)
    _check(align, raw, starts, lens, exp)
    # rows outside every range, and the infeasible utterance's rows and spans, keep their fill
    written = torch.zeros(x.shape[0], dtype=torch.bool)
    for b, (s0, n) in enumerate(zip(starts, lens)):
        if exp[b][0] == 0:
            written[s0:s0 + n] = True
    assert written.sum() == 37 + 120 + 64
    assert (raw["frames"][~written] == align.FRAME_SENTINEL).all() and (raw["frames"][written] >= 0).all()
    assert torch.isnan(raw["frame_logp"][~written]).all() and not torch.isnan(raw["frame_logp"][written]).any()
    t3 = raw["target_start"][3]
    assert (raw["spans"][t3:t3 + 5] == align.FRAME_SENTINEL).all() and torch.isnan(raw["score"][3])
    assert raw["score"][1] == 0.0
    # two runs are bit-identical, and regions in another order give the same per-utterance results
    again = align.align_packed_device_raw(x.cuda(), starts, lens, tg)
    assert all(torch.equal(a, b) for a, b in zip(_bits(raw), _bits(again)))
    perm = [4, 0, 3, 2, 1]
    raw_p = align.align_packed_device_raw(x.cuda(), [starts[i] for i in perm], [lens[i] for i in perm],
                                          [tg[i] for i in perm])
    _check(align, raw_p, [starts[i] for i in perm], [lens[i] for i in perm], [exp[i] for i in perm])
    # the public call names the infeasible utterance after computing the others
    with pytest.raises(ValueError, match=r"utterance\(s\) \[3\]"):
        align.align_packed(x.cuda(), starts, lens, tg)
    res, status = align.align_packed(x.cuda(), starts, lens, tg, return_status=True)
    assert status == [0, 0, 0, 1, 0] and res[3] is None and res[2] == exp[2][1]


def test_non_finite_log_probs_end_with_status_4(align):
    cases = [_case(50, 12, 700), _case(50, 12, 701), _case(50, 12, 702), _case(31, 15, 703)]
    y1 = cases[1][1]
    cases[1][0][:, y1[5]] = float("-inf")          # a target token impossible on every frame
    cases[2][0][20] = float("nan")                 # a NaN row: every path crosses it
    exp = [align.align_host_status(lp, y) for lp, y in cases]
    assert [st for st, _ in exp] == [0, 4, 4, 0]
    x, starts, lens = _pack(cases, gap=2)
    raw = align.align_packed_device_raw(x.cuda(), starts, lens, [y for _, y in cases])
    _check(align, raw, starts, lens, exp)
    assert (raw["frames"][starts[1]:starts[1] + 50] == align.FRAME_SENTINEL).all()
    assert (raw["frames"][starts[2]:starts[2] + 50] == align.FRAME_SENTINEL).all()
    # -inf on some frames only leaves finite paths: still exact
    lp, y = _case(60, 14, 704)
    lp[10:30, y[3]] = float("-inf")
    lp[5, 0] = float("-inf")
    st, e = align.align_host_status(lp, y)
    assert st == 0
    _check(align, align.align_packed_device_raw(lp.cuda(), [0], [60], [y]), [0], [60], [(st, e)])


def test_argument_checks(align):
    """A short workspace is CFM_ERR_VALUE (the ValueError of _lib.check) before anything is launched."""
    lp, y = _case(40, 15, 900)
    x = lp.cuda()
    need = align.plan_workspace([40], [15])
    assert need == align.align_packed_device_raw(x, [0], [40], [y])["workspace_bytes"] > 40 * 2 * 4
    with pytest.raises(ValueError, match="workspace too small"):
        align.align_packed_device_raw(x, [0], [40], [y], workspace_bytes=need - 1)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        align.align_packed_device_raw(x, [0], [40], [y], max_workspace_bytes=need - 1)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        align.align_packed(x, [0], [40], [y], max_workspace_bytes=64)
    with pytest.raises(ValueError):
        align.align_packed_device_raw(x, [0], [40], [y], blank_id=V32)
    with pytest.raises(ValueError):
        align.align_packed(x, [10], [40], [y])                      # rows beyond the tensor
    # a row range outside the tensor reaches the kernel only through the raw call: status 2, ids: 3
    raw = align.align_packed_device_raw(x, [10, 0, 0, -1], [40, 40, 40, 5], [y, [1, V32], [1, -1, 2], [1]])
    assert raw["status"].tolist() == [2, 3, 3, 2]
    assert (raw["frames"] == align.FRAME_SENTINEL).all()


# ------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def small_model(align, golden_dir):
    from chunkformer_amd.config import SMALL256
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.weights import synthetic_state_dict
    from conftest import with_fixture_ctc_head
    g = np.load(os.path.join(golden_dir, "small256.npz"))
    sd = with_fixture_ctc_head(synthetic_state_dict(SMALL256, int(g["seed"])), g)
    return ChunkFormerModel(SMALL256, sd, dtype="fp32")


def test_batch_align_equals_host_on_device_log_probs(align, small_model):
    from chunkformer_amd.weights import synthetic_features
    m, C, L, R = small_model, 16, 32, 16
    xs = synthetic_features([611, 97, 350, 1203], 31)
    greedy = m.batch_decode(xs, C, L, R)
    targets = [align.remove_duplicates_and_blank(h.tolist()) for h in greedy]
    assert sum(1 for t in targets if t) >= 2
    res = m.batch_align(xs, targets, C, L, R)
    lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int)
    eo, el, n_chunks, _, _, _ = m.encoder.forward_parallel_chunk(xs, lens, C, L, R, offset=torch.zeros(4, dtype=torch.int))
    starts = (np.cumsum([0] + list(n_chunks[:-1])) * C).tolist()
    logp, _ = m.encoder.ctc_log_softmax(eo.reshape(-1, eo.shape[-1]), want_logp=True, want_ids=False)
    logp = logp.cpu()
    for r, y, s0, n in zip(res, targets, starts, [int(v) for v in el.tolist()]):
        assert len(r.frames) == n and align.remove_duplicates_and_blank(r.frames) == y
        assert r == align.force_align_host(logp[s0:s0 + n], y)
    # two budget groups give the same; a target that cannot be aligned is named by its input index
    again = m.batch_align(xs, targets, C, L, R, total_batch_duration=10)
    assert all(align.remove_duplicates_and_blank(a.frames) == y and len(a.frames) == len(b.frames)
               for a, b, y in zip(again, res, targets))
    bad = list(targets)
    bad[2] = [1] * 400
    with pytest.raises(ValueError, match=r"utterance\(s\) \[2\]"):
        m.batch_align(xs, bad, C, L, R, total_batch_duration=10)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        m.batch_align(xs, targets, C, L, R, max_workspace_bytes=1000)
    # the reference's signature on one utterance's device rows
    assert align.force_align(logp[starts[0]:starts[0] + len(res[0].frames)].cuda(), torch.tensor(targets[0])) == \
        res[0].frames


def test_endless_align_equals_host_on_returned_rows(align, small_model):
    from chunkformer_amd.model import endless_segments
    from chunkformer_amd.weights import synthetic_features
    m, C, L, R, tbd = small_model, 16, 32, 16, 20
    T = 3000
    assert len(endless_segments(T, C, L, R, tbd, m.config.num_blocks, m.config.kernel_size)[1]) == 3
    x = synthetic_features([T], 47)[0]
    ids, eo = m.endless_decode(x, C, L, R, total_batch_duration=tbd, return_encoder_out=True)
    y = align.remove_duplicates_and_blank(ids.reshape(-1).tolist())
    assert len(y) >= 1
    r = m.endless_align(x, y, C, L, R, total_batch_duration=tbd)
    logp, _ = m.encoder.ctc_log_softmax(eo[0], want_logp=True, want_ids=False)
    assert len(r.frames) == eo.shape[1] and align.remove_duplicates_and_blank(r.frames) == y
    assert r == align.force_align_host(logp.cpu(), y)
    assert len(r.token_times()) == len(y) and r.token_times()[0][0] == r.spans[0][0] * 0.08


def test_align_rejected_on_transducer_and_classification_checkpoints(align, golden_dir):
    from chunkformer_amd.config import LARGE, SMALL
    from chunkformer_amd.model import ChunkFormerModel
    from chunkformer_amd.transducer import RNNTConfig, synthetic_transducer_state_dict
    from chunkformer_amd.weights import synthetic_features, synthetic_state_dict
    g = np.load(os.path.join(golden_dir, "rnnt.npz"))
    c = RNNTConfig(vocab=int(g["vocab"]))
    cfg = dataclasses.replace(LARGE, num_blocks=1)
    sd = synthetic_state_dict(cfg, 1)
    sd.update(synthetic_transducer_state_dict(c, int(g["seed"])))
    m = ChunkFormerModel(cfg, sd, dtype="fp32", model_type="transducer", rnnt_config=c)
    x = synthetic_features([200], 3)
    with pytest.raises(ValueError, match="transducer"):
        m.batch_align(x, [[1, 2]], 16, 32, 16)
    with pytest.raises(ValueError, match="transducer"):
        m.endless_align(x[0], [1, 2], 16, 32, 16)
    cfg = dataclasses.replace(SMALL, vocab=0)
    sd = synthetic_state_dict(cfg, 1)
    sd["classification_heads.gender.linear.weight"] = torch.randn(2, cfg.d_model, generator=torch.Generator().manual_seed(0))
    sd["classification_heads.gender.linear.bias"] = torch.zeros(2)
    m = ChunkFormerModel(cfg, sd, dtype="fp32", model_type="classification", tasks={"gender": 2})
    with pytest.raises(ValueError, match="classification model"):
        m.batch_align(x, [[1, 2]], 16, 32, 16)
    with pytest.raises(ValueError, match="classification model"):
        m.endless_align(x[0], [1, 2], 16, 32, 16)
