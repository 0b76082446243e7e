"""The two kernels of the full-sum transducer score, one at a time (include/cfm_ops.h): cfm_op_rnnt_lattice against
the f64 host lattice and cfm_op_rnnt_alpha against the host recursion.

Lattice shapes: per fixture model one call over five utterances of T = 1, 2, 9, 33, 65 rows, each with six hypotheses
of U = 0, 1, 7, 31, 32, 33 tokens (several hypotheses of different U share an utterance, several utterances share a
call, node tiles of 64 straddle hypotheses and the last one ends inside a lattice; U + 1 = 32 / 33 / 34 sit on both
sides of the 32-node MFMA column tile); every hypothesis with tokens holds the id V - 1.  One shipped-width case
J = 512, V = 1024, T = 33, U = 17.  All of these run 64 nodes per workgroup: 64 nodes of z fit the LDS beside the
ffn_out tile up to J = 544 in f32 and J = 928 in bf16.  The 32-node instantiations are what serves the widths above
that, so one case runs them at the widest join the kernel takes, J = 1,024 (V = 130: one full and one partly padded
vocabulary tile; T = 9 with U = 0, 7, 33, 40: 328 nodes, eleven tiles of 32 of which the last is partly filled), in
f32 (the 152 KB dynamic-LDS launch) and in bf16.
fp32 bars: 1e-5 per node on the fixture models (the bar test_gpu_rnnt_beam.py holds this joint to), 1e-4 at J = 512 and
J = 1,024 (the project's fp32 bar).  bf16 at J = 1,024: twice the largest per-node deviation measured for the bf16
kernel (tests/test_gpu_td_rescore.py states it)."""
import functools

import numpy as np
import pytest
import torch

import rnnt_beam_fixture as F

pytestmark = pytest.mark.gpu

TS = (1, 2, 9, 33, 65)
US = (0, 1, 7, 31, 32, 33)


@functools.lru_cache(maxsize=None)
def device_model(name, recipe="dense"):
    from chunkformer_amd.transducer import RNNTGreedy
    from chunkformer_amd.transducer_rescore import TransducerRescorer
    cfg, sd = F.model(name, recipe)
    return TransducerRescorer(RNNTGreedy(cfg, sd, "cuda:0"), None, "fp32")


def _utterances(cfg, seed):
    g = np.random.default_rng(seed)
    enc, hyps = [], []
    for u, T in enumerate(TS):
        enc.append(torch.from_numpy(g.integers(-128, 128, size=(T, cfg.enc_dim)).astype(np.float32) / 64.0))
        for U in US:
            y = g.integers(1, cfg.vocab, size=U).tolist()
            if U:
                y[int(g.integers(0, U))] = cfg.vocab - 1
            hyps.append((u, y))
    return enc, hyps


def _lattice_case(tr, host, enc, hyps, dtype):
    """Device (b, k) of every hypothesis from the host's f64 projections rounded to f32, beside the host's f64 lattice."""
    from chunkformer_amd import transducer_rescore as TR
    starts = np.cumsum([0] + [e.shape[0] for e in enc[:-1]]).tolist()
    lens = [e.shape[0] for e in enc]
    e_all, q_all, want = [None] * len(enc), [], []
    for u, y in hyps:
        e, q = TR.joint_projections_host(host, enc[u], y)
        e_all[u] = e
        q_all.append(q)
        want.append(TR.lattice_logp_host(host, enc[u], y))
    got = tr.lattice(torch.cat(e_all).float(), torch.cat(q_all).float(), starts, lens, hyps, dtype)
    return got, want


def _worst(got, want):
    w = 0.0
    for (gb, gk), (wb, wk) in zip(got, want):
        assert gb.shape == wb.shape and gk.shape == wk.shape
        assert np.isfinite(gb).all() and np.isfinite(gk).all()
        w = max(w, float(np.abs(gb - wb).max()), float(np.abs(gk - wk).max()) if gk.size else 0.0)
    return w


@pytest.mark.parametrize("name", ["v17", "v37", "v130", "v1024"])
def test_lattice_fp32_vs_host(name):
    tr = device_model(name)
    enc, hyps = _utterances(tr.cfg, 7)
    got, want = _lattice_case(tr, F.host_model(name, "dense"), enc, hyps, "fp32")
    worst = _worst(got, want)
    print(f"{name}: max |device - f64| per node = {worst:.3e}")
    assert worst <= 1e-5


@functools.lru_cache(maxsize=None)
def wide_model():
    from chunkformer_amd.transducer import RNNTConfig, RNNTGreedy, synthetic_transducer_state_dict
    from chunkformer_amd.transducer_beam import HostTransducer
    from chunkformer_amd.transducer_rescore import TransducerRescorer
    cfg = RNNTConfig(vocab=1024, enc_dim=64, embed_size=32, hidden=64, num_layers=1, pred_out=64, join_dim=512)
    sd = synthetic_transducer_state_dict(cfg, seed=31)
    return TransducerRescorer(RNNTGreedy(cfg, sd, "cuda:0"), None, "fp32"), HostTransducer(cfg, sd)


def wide_case():
    tr, host = wide_model()
    g = np.random.default_rng(5)
    enc = [torch.from_numpy(g.integers(-128, 128, size=(33, 64)).astype(np.float32) / 64.0)]
    y = g.integers(1, 1024, size=17).tolist()
    y[3] = 1023
    return tr, host, enc, [(0, y)]


def test_lattice_fp32_shipped_width():
    tr, host, enc, hyps = wide_case()
    got, want = _lattice_case(tr, host, enc, hyps, "fp32")
    worst = _worst(got, want)
    print(f"J = 512: max |device - f64| per node = {worst:.3e}")
    assert worst <= 1e-4


@functools.lru_cache(maxsize=None)
def widest_model():
    from chunkformer_amd.transducer import RNNTConfig, RNNTGreedy, synthetic_transducer_state_dict
    from chunkformer_amd.transducer_beam import HostTransducer
    from chunkformer_amd.transducer_rescore import TransducerRescorer
    cfg = RNNTConfig(vocab=130, enc_dim=32, embed_size=32, hidden=32, num_layers=1, pred_out=32, join_dim=1024)
    sd = synthetic_transducer_state_dict(cfg, seed=33)
    return TransducerRescorer(RNNTGreedy(cfg, sd, "cuda:0"), None, "fp32"), HostTransducer(cfg, sd)


def widest_case():
    tr, host = widest_model()
    g = np.random.default_rng(6)
    enc = [torch.from_numpy(g.integers(-128, 128, size=(9, 32)).astype(np.float32) / 64.0)]
    hyps = []
    for U in (0, 7, 33, 40):
        y = g.integers(1, 130, size=U).tolist()
        if U:
            y[U // 2] = 129
        hyps.append((0, y))
    return tr, host, enc, hyps


def test_lattice_fp32_widest_join_32_node_kernel():
    tr, host, enc, hyps = widest_case()
    got, want = _lattice_case(tr, host, enc, hyps, "fp32")
    worst = _worst(got, want)
    print(f"J = 1024 fp32: max |device - f64| per node = {worst:.3e}")
    assert worst <= 1e-4


def test_lattice_bf16_widest_join_32_node_kernel():
    from test_gpu_td_rescore import BF16_NODE_MEASURED
    tr, host, enc, hyps = widest_case()
    got, want = _lattice_case(tr, host, enc, hyps, "bf16")
    worst = _worst(got, want)
    print(f"J = 1024 bf16: max |device - f64| per node = {worst:.3e}")
    assert worst <= 2 * BF16_NODE_MEASURED


def _random_lattice(g, T, U):
    return -3.0 * g.random((T, U + 1)), -5.0 * g.random((T, U))


def test_alpha_vs_host():
    from chunkformer_amd import transducer_rescore as TR
    g = np.random.default_rng(11)
    # 1 x 0 .. 130 x 70, a thin 1000 x 300, and one whose diagonals (U + 1 > 2048) live in the workspace
    shapes = [(1, 0), (1, 1), (2, 0), (1, 5), (5, 1), (2, 2), (9, 7), (33, 31), (17, 40), (65, 33), (130, 70),
              (1000, 300), (3, 2100)]
    lats = [_random_lattice(g, T, U) for T, U in shapes]
    lats = [(b.astype(np.float32), k.astype(np.float32)) for b, k in lats]
    got, err = TR.alpha_device(lats, "cuda:0")
    assert err == 0
    for (T, U), (b, k), v in zip(shapes, lats, got):
        want = TR.td_score_host(b, k)
        print(f"{T} x {U}: |device - host| = {abs(v - want):.3e}")
        assert abs(v - want) <= 1e-9, (T, U, v, want)


def test_alpha_nan_sets_the_error_word():
    from chunkformer_amd import transducer_rescore as TR
    g = np.random.default_rng(12)
    good = tuple(a.astype(np.float32) for a in _random_lattice(g, 9, 7))
    b, k = (a.astype(np.float32) for a in _random_lattice(g, 9, 7))
    b[4, 3] = np.nan
    got, err = TR.alpha_device([good, (b, k)], "cuda:0")
    assert err == 4
    assert abs(got[0] - TR.td_score_host(*good)) <= 1e-9 and got[1] != got[1]
