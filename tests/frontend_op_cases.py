"""Seeded inputs and fp64 reference outputs of every case of the front-end operator tests
(cfm_op_frontend_conv0_dw, cfm_op_frontend_dw2): shared by tests/test_gpu_ops_frontend.py (the kernels) and
tests/test_frontend_op_ref_cpu.py (the references and the tolerances).  The ops run on a model's own weights:
one synthetic-weight model per d -- SMALL (d = 128), SMALL256 and LARGE cut to one block -- built on the GPU by the
test, its state dict here.  Everything in this module is CPU-only and cached; cases must not be modified.
"""
import dataclasses
import functools
import zlib
from types import SimpleNamespace

import torch

from chunkformer_amd.config import LARGE, SMALL, SMALL256
from chunkformer_amd.weights import synthetic_state_dict
from oracle import frontend_op_ref as R

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTS = ["fp32", "bf16", "fp16"]
DS = [128, 256, 512]
CFG = {128: SMALL, 256: dataclasses.replace(SMALL256, num_blocks=1), 512: dataclasses.replace(LARGE, num_blocks=1)}
GUARD = 64           # NaN elements after every output
NWIN = 3
E = "encoder.embed."


def rel_err(got, exp):
    return ((got.double() - exp).abs().max() / exp.abs().max()).item()


@functools.lru_cache(maxsize=None)
def state_dict(d):
    """the synthetic recipe, with the CMVN mean x 4 (U(-2, 2): a padding row, -mean * istd, then differs from a zero
    row by as much as a real frame does) and the conv0 bias x 4 (U(-4/3, 4/3)), so that CMVN applied before the
    padding and a dropped conv0 bias move the output by 10 x the loosest bar (tests/test_frontend_op_ref_cpu.py)"""
    sd = synthetic_state_dict(CFG[d], 1)
    sd["encoder.global_cmvn.mean"] = 4.0 * sd["encoder.global_cmvn.mean"]
    sd[E + "conv.0.bias"] = 4.0 * sd[E + "conv.0.bias"]
    return sd


@functools.lru_cache(maxsize=None)
def weights(d):
    sd = state_dict(d)
    return SimpleNamespace(w0=sd[E + "conv.0.weight"][:, 0], b0=sd[E + "conv.0.bias"], w1=sd[E + "conv.2.weight"][:, 0],
                           b1=sd[E + "conv.2.bias"], pw1=sd[E + "conv.3.weight"][:, :, 0, 0], b_pw1=sd[E + "conv.3.bias"],
                           w2=sd[E + "conv.5.weight"][:, 0], b2=sd[E + "conv.5.bias"],
                           mean=sd["encoder.global_cmvn.mean"], istd=sd["encoder.global_cmvn.istd"])


# =================================================================================== conv0 + ReLU + dw1
# kernels: (name, selector, k) -- the channel-stationary kernel at k = 0, 1, 4 chunks-per-workgroup settings: the
# 3 chunks of W = 119 / 135 split 1 + 1 + 1, 1 + 2 and 3
KERNELS = {"valu": ("valu", 0), "pos": ("pos", 0), "ch_k0": ("ch", 0), "ch_k1": ("ch", 1), "ch_k4": ("ch", 4)}
# W: 15 -> T2 = 3, P = 57 positions (less than one tile); 63 -> P = 285: two 256-position chunks, the second
# partial, the boundary mid-row; 119, 135 -> 3 chunks; 100 .. 103: the four parities of the padded path
WS = [15, 63, 119, 135, 100, 101, 102, 103]


def _conv_keys():
    """(W, cmvn, table addressing, feature scale): every W x CMVN on / off x packed / table addressing, and one case
    with features x 50 (realistic outliers stay exact under the bf16 channel-stationary kernel's 2^-24 clamp trick)"""
    keys = [(W, cm, tab, 1.0) for W in WS for cm in (True, False) for tab in (False, True)]
    return keys + [(119, True, False, 50.0)]


CONV_KEYS = _conv_keys()


def geometry(W):
    T1 = R.sub_len(W)
    return T1, R.sub_len(T1)


@functools.lru_cache(maxsize=None)
def conv_inputs(key):
    """the feature buffers and window records of a case (the same for every d): per window NVALID in {W, W - 5, 1}
    (rotated per case); source rows at or past NVALID, and every row between the windows, are NaN"""
    W, cmvn, tab, scale = key
    gen = torch.Generator().manual_seed(zlib.crc32(repr(("fe", key)).encode()))
    rot = zlib.crc32(repr(key).encode()) % 3
    nvalid = [[W, W - 5, 1][(n + rot) % 3] for n in range(NWIN)]
    step = W + 3
    c = SimpleNamespace(W=W, cmvn=cmvn, tab=tab, scale=scale, nvalid=nvalid, step=step)
    if tab:   # utterance 0 holds windows 0 and 1 (chunks 0 and 1, `step` rows apart), utterance 1 window 2
        c.utts = [torch.full((step + W, 80), float("nan")), torch.full((W, 80), float("nan"))]
        c.where = [(0, 0), (0, 1), (1, 0)]                                # (utterance, chunk) per window
        for n, (u, ch) in enumerate(c.where):
            c.utts[u][ch * step: ch * step + nvalid[n]] = scale * torch.randn(nvalid[n], 80, generator=gen)
        c.src = [(c.utts[u], ch * step) for u, ch in c.where]
    else:
        c.feats = torch.full((NWIN * step, 80), float("nan"))
        c.row0 = [n * step for n in range(NWIN)]
        for n in range(NWIN):
            c.feats[c.row0[n]: c.row0[n] + nvalid[n]] = scale * torch.randn(nvalid[n], 80, generator=gen)
        c.src = [(c.feats, r) for r in c.row0]
    c.meta = torch.zeros(NWIN, 8, dtype=torch.int32)
    for n in range(NWIN):
        c.meta[n, 1] = nvalid[n]
        if tab:
            c.meta[n, 6], c.meta[n, 7] = c.where[n]
        else:
            c.meta[n, 0] = c.row0[n]
    return c


def conv_windows(c, w, cmvn_before_padding=False, nvalid=None):
    nv = c.nvalid if nvalid is None else nvalid
    xs = [R.windows(buf, [r], [v], c.W, w.mean if c.cmvn else None, w.istd if c.cmvn else None, cmvn_before_padding)
          for (buf, r), v in zip(c.src, nv)]
    return torch.cat(xs)


@functools.lru_cache(maxsize=None)
def conv_case(key, d):
    c = SimpleNamespace(**vars(conv_inputs(key)))
    w = weights(d)
    c.d, c.key = d, key
    c.T1, c.T2 = geometry(c.W)
    c.x = conv_windows(c, w)
    assert torch.isfinite(c.x).all()
    c.ref = R.conv0_dw_op_ref(c.x, w.w0, w.b0, w.w1, w.b1)
    c.scale = c.ref.abs().max().item()
    return c


def conv_e_round(key, d, kernel, dt):
    c, w = conv_case(key, d), weights(d)
    return rel_err(R.conv0_dw_op_ref(c.x, w.w0, w.b0, w.w1, w.b1, emulate=TDT[dt], kernel=kernel), c.ref)


# =================================================================================== dw2 (and pw1 + ReLU + dw2)
# T2: 3 -> one output row; even T2 leaves the last pw1 row unused; T2 * 19 is never a multiple of 64 (the GEMM's
# row tile), so every window boundary falls inside a tile of the fused kernel
DW2_T2 = [3, 4, 7, 8, 15, 29, 33]
DW2_NWIN = [1, 2, 5]
DW2_KEYS = [(t2, n) for t2 in DW2_T2 for n in DW2_NWIN]


def dw2_segs(T2):
    return [1, 4, R.sub_len(T2) + 3]


@functools.lru_cache(maxsize=None)
def dw2_case(key, d, dt):
    """a: the dw1 output [nwin, T2, 19, d] in the type (N(0, 1)); z: its pw1 + ReLU rows, computed here in float64
    and rounded to the type -- the input of the UNFUSED mode; ref: dw2 of z; ref_fused: dw2 of the unrounded pw1 rows"""
    T2, nwin = key
    w, tdt = weights(d), TDT[dt]
    gen = torch.Generator().manual_seed(zlib.crc32(repr(("dw2", key, d)).encode()))
    c = SimpleNamespace(T2=T2, T3=R.sub_len(T2), nwin=nwin, d=d, dt=dt)
    c.a = torch.randn(nwin, T2, 19, d, generator=gen).to(tdt)
    c.pw1 = w.pw1.to(tdt)
    c.z_exact = R.pw1_relu_ref(c.a, c.pw1, w.b_pw1)
    c.z = c.z_exact.to(tdt)
    c.ref = R.dw2_op_ref(c.z, w.w2, w.b2)
    c.ref_fused = R.dw2_op_ref(c.z_exact, w.w2, w.b2)
    return c


def dw2_e_round(key, d, dt, fused):
    c, w = dw2_case(key, d, dt), weights(d)
    if fused:
        z = R.pw1_relu_ref(c.a, c.pw1, w.b_pw1, emulate=TDT[dt])
        return rel_err(R.dw2_op_ref(z, w.w2, w.b2, emulate=TDT[dt]), c.ref_fused)
    return rel_err(R.dw2_op_ref(c.z, w.w2, w.b2, emulate=TDT[dt]), c.ref)
