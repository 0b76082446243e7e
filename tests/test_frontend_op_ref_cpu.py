"""CPU-side guard of the front-end operator parity tests (tests/test_gpu_ops_frontend.py): the fp64 references are
pinned to oracle/encoder_ref.py's front-end, the E_round tables the 16-bit bars come from are recomputed, and the
bars are shown to see the errors a kernel can make silently -- on the tests' own inputs each mutation of the
reference must move the output by at least 10 x the bar."""
import math

import pytest
import torch

import frontend_op_cases as A
from oracle import encoder_ref
from oracle import frontend_op_ref as R
from test_gpu_ops_frontend import BAR, E_ROUND

MARGIN = 10.0
PIN = 1e-5
E = A.E


# ------------------------------------------------------------------------------------------ the references, pinned
def _tail(x, sd, d, after):
    """the rest of the front-end, in the reference's own calls, from the dw1 output (after = 2) or the dw2 output
    (after = 5), channels-last [n, t, f, d] -> [n, T', d]"""
    import torch.nn.functional as F
    x = x.permute(0, 3, 1, 2)
    if after == 2:
        x = F.relu(F.conv2d(x, sd[E + "conv.3.weight"], sd[E + "conv.3.bias"]))
        x = F.conv2d(x, sd[E + "conv.5.weight"], sd[E + "conv.5.bias"], stride=2, groups=d)
    x = F.relu(F.conv2d(x, sd[E + "conv.6.weight"], sd[E + "conv.6.bias"]))
    n, c, t, f = x.shape
    x = x.permute(0, 2, 1, 3).reshape(n, t, c * f)
    return F.linear(x, sd[E + "out.weight"], sd[E + "out.bias"]) * math.sqrt(d)


@pytest.mark.parametrize("W", [15, 63, 100, 101, 102, 103])
def test_references_match_encoder_oracle_frontend(W):
    """encoder_ref.frontend() cut after conv.2 and after conv.5: the operator references replace its head up to
    the cut, the remaining layers run as frontend() runs them, and the two ends must agree"""
    d = 128
    sd = {k: v.double() for k, v in A.state_dict(d).items()}
    w = A.weights(d)
    x = torch.randn(2, W, 80, generator=torch.Generator().manual_seed(W), dtype=torch.float64)
    exp = encoder_ref.frontend(x, sd, d)
    dw1 = R.conv0_dw_op_ref(x, w.w0, w.b0, w.w1, w.b1)
    assert dw1.shape == (2, A.geometry(W)[1], 19, d)
    assert A.rel_err(_tail(dw1, sd, d, 2), exp) <= PIN, "cut after conv.2"
    z = R.pw1_relu_ref(dw1, w.pw1, w.b_pw1)
    dw2 = R.dw2_op_ref(z, w.w2, w.b2)
    assert A.rel_err(_tail(dw2, sd, d, 5), exp) <= PIN, "cut after conv.5"


def test_windows_match_encoder_oracle_packing():
    """padding, then CMVN (padding rows become -mean * istd): encoder_ref.pack_windows + cmvn"""
    C, T = 2, 61
    sd = A.state_dict(128)
    x = torch.randn(T, 80, generator=torch.Generator().manual_seed(3))
    win, (n,) = encoder_ref.pack_windows([x], C)
    exp = encoder_ref.cmvn(win, sd).double()
    W, step = 8 * (C - 1) + 15, 8 * C
    w = A.weights(128)
    got = R.windows(x, [c * step for c in range(n)], [T - c * step for c in range(n)], W, w.mean, w.istd)
    assert (torch.tensor([T - c * step for c in range(n)]) < W).any(), "no padded window"
    assert A.rel_err(got, exp) <= PIN


# ------------------------------------------------------------------------------------------ the E_round tables
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("kernel", ["valu", "pos", "ch"])
def test_e_round_table_conv0_dw(kernel, dt):
    worst = max((A.conv_e_round(k, d, kernel, dt), k, d) for k in A.CONV_KEYS for d in A.DS)
    print(f"E_round(conv0_dw {kernel}, {dt}) = {worst[0]:.3e} at {worst[1:]}")
    assert 0.9 * E_ROUND[kernel][dt] <= worst[0] <= E_ROUND[kernel][dt]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_e_round_table_dw2(fused, dt):
    worst = max((A.dw2_e_round(k, d, dt, fused), k, d) for k in A.DW2_KEYS for d in ([512] if fused else A.DS))
    fam = "dw2_fused" if fused else "dw2"
    print(f"E_round({fam}, {dt}) = {worst[0]:.3e} at {worst[1:]}")
    assert 0.9 * E_ROUND[fam][dt] <= worst[0] <= E_ROUND[fam][dt]


# ------------------------------------------------------------------------------------------ sensitivity
def _report(seen, bar, what):
    for name, e in seen.items():
        print(f"{what}: {name}: {e:.3e} = {e / bar:.0f} x the bar")
    for name, e in seen.items():
        assert e >= MARGIN * bar, f"{what}: {name} moves the output by {e:.3e} < {MARGIN} x the bar ({bar:.3e})"


def _unpoisoned(c):
    """the case with the NaN source rows (at or past NVALID) replaced by data, 8 x larger as in the attention and conv
    module cases: what a kernel that reads one row too many would see if the buffer held a neighbour's frames"""
    gen = torch.Generator().manual_seed(99)
    u = A.SimpleNamespace(**vars(c))
    u.src = [(torch.where(torch.isnan(buf), 8.0 * torch.randn(buf.shape, generator=gen), buf), r) for buf, r in c.src]
    return u


@pytest.mark.parametrize("dt", A.DTS)
@pytest.mark.parametrize("d", A.DS)
@pytest.mark.parametrize("key", [(63, True, False, 1.0), (119, True, True, 1.0), (100, True, False, 1.0)],
                         ids=["W63", "W119-tab", "W100"])
def test_bar_sees_conv0_dw_errors(key, d, dt):
    """against the loosest bar of the three kernels (the channel-stationary kernel's)"""
    c, w = A.conv_case(key, d), A.weights(d)
    bar, seen = max(BAR[k][dt] for k in ("valu", "pos", "ch")), {}
    ref = lambda x=c.x, **kw: R.conv0_dw_op_ref(x, kw.pop("w0", w.w0), kw.pop("b0", w.b0), kw.pop("w1", w.w1), w.b1, **kw)
    seen["CMVN before the padding"] = A.rel_err(ref(A.conv_windows(c, w, cmvn_before_padding=True)), c.ref)
    seen["NVALID + 1"] = A.rel_err(ref(A.conv_windows(_unpoisoned(c), w, nvalid=[v + 1 for v in c.nvalid])), c.ref)
    seen["ReLU dropped"] = A.rel_err(ref(relu=False), c.ref)
    seen["conv0 bias dropped"] = A.rel_err(ref(b0=torch.zeros_like(w.b0)), c.ref)
    seen["dw1 taps transposed"] = A.rel_err(ref(w1=w.w1.transpose(1, 2)), c.ref)
    # a 256-position chunk boundary off by one: the first position of each later chunk computed as the one before
    flat = c.ref.reshape(A.NWIN, -1, d).clone()
    assert flat.shape[1] > 256
    for p in range(256, flat.shape[1], 256):
        flat[:, p] = c.ref.reshape(A.NWIN, -1, d)[:, p - 1]
    seen["chunk boundary shifted by one position"] = A.rel_err(flat.reshape(c.ref.shape), c.ref)
    _report(seen, bar, f"conv0_dw {key} d={d} {dt}")


@pytest.mark.parametrize("dt", A.DTS)
@pytest.mark.parametrize("d", A.DS)
@pytest.mark.parametrize("T2", [4, 8])
def test_bar_sees_dw2_errors(T2, d, dt):
    """even T2 (the last pw1 row of a window unused), 5 windows; against the looser of the two dw2 bars"""
    c, w = A.dw2_case((T2, 5), d, dt), A.weights(d)
    bar = max(BAR["dw2"][dt], BAR["dw2_fused"][dt])
    seen = {"window boundary ignored (pitch 2 T3 + 1)": A.rel_err(R.dw2_op_ref(c.z, w.w2, w.b2, pitch=2 * c.T3 + 1), c.ref),
            "stride-2 phase off by one": A.rel_err(R.dw2_op_ref(c.z, w.w2, w.b2, phase=1), c.ref)}
    _report(seen, bar, f"dw2 T2={T2} d={d} {dt}")
