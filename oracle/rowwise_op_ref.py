"""ORACLE — test infrastructure only.  Float64 CPU references of the row-wise operators of include/cfm_ops.h
(cfm_op_layernorm, cfm_op_conv_module, cfm_op_pos_table), written from the operator contracts alone: no code is
shared with the kernels or with oracle/encoder_ref.py.

emulate=<16-bit dtype> rounds exactly where a correct kernel of that type must round and nowhere else; it sizes
the tests' tolerance (E_round) and is never compared with a kernel.  The rounding points:

  layernorm    y, y2 arrive in the type (the caller's tensors).  x stays f32: the residual chain is the kernel's
               f32 fmaf chain (csrc/norm.hip:104-111), reproduced bit-exactly by fmaf32 below, and the second
               LayerNorm of LN2 continues from the unrounded first one (norm.hip:161-167: registers).  Rounded:
               `out` alone (store_row<H>, norm.hip:72 / 76); LN2_F32's out is f32 and rounds nothing.
  conv_module  the 15 taps are rounded to the type (pke<E>, csrc/conv_module.hip:148: the dot2 kernels run on
               16-bit taps); the products accumulate in f32 (conv_module.hip:186), bias / LayerNorm / SiLU are
               f32; `out` is rounded (conv_module.hip:213).
  pos_table    the angle is the f32 product |p| * div_i of two f32 factors (csrc/misc.hip:30-31), as in the
               reference's torch code (pos * div, both f32); sin / cos of that f32 angle in float64; `out` is
               rounded (misc.hip:33-34).
"""
import math

import torch

LN, LN2, LN2_F32 = 0, 1, 2


def _rnd(emulate):
    return (lambda t: t.to(emulate).double()) if emulate is not None else (lambda t: t)


def fmaf32(a, y, x):
    """fmaf(a, y, x) on f32 tensors, correctly rounded (one rounding): the product is exact in float64, the sum
    is rounded to odd (TwoSum gives the rounding error's sign) and then to f32."""
    assert a.dtype == y.dtype == x.dtype == torch.float32
    p, xd = a.double() * y.double(), x.double()
    s = p + xd
    bb = s - p
    e = (p - (s - bb)) + (xd - bb)
    even = (s.view(torch.int64) & 1) == 0
    toward = torch.where(e > 0, torch.full_like(s, math.inf), torch.full_like(s, -math.inf))
    s = torch.where((e != 0) & even, torch.nextafter(s, toward), s)
    return s.float()


def resid_chain(x, y=None, alpha=1.0, ymask=None, y2=None, alpha2=1.0, ymask2=None):
    """the f32 row values the LayerNorm sees: x, then + alpha * ymask * y, then + alpha2 * ymask2 * y2"""
    v = x.float().clone()
    M = v.shape[0]
    for yy, al, mk in ((y, alpha, ymask), (y2, alpha2, ymask2)):
        if yy is None:
            continue
        a = torch.full((M, 1), al, dtype=torch.float32)
        if mk is not None:
            a = a * mk.float().view(M, 1)
        v = fmaf32(a.expand_as(v).contiguous(), yy.float(), v)
    return v


def _ln64(v, w, b, eps):
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    return (v - mean) / torch.sqrt(var + eps) * w.double() + b.double()


def layernorm_op_ref(kind, x, w1, b1, eps, y=None, alpha=1.0, ymask=None, y2=None, alpha2=1.0, ymask2=None,
                     defer=False, w2=None, b2=None, rowmask=None, emulate=None):
    """-> (x after the call: f32 for LN (bit-exact contract), float64 for LN2 / LN2_F32;  out float64)"""
    rnd = _rnd(emulate)
    v = resid_chain(x, y, alpha, ymask, y2, alpha2, ymask2)
    t = _ln64(v.double(), w1, b1, eps)
    if kind == LN:
        x_new = x.float().clone() if (defer or y is None) else v
        out = rnd(t)
        if rowmask is not None:
            out = out * (rowmask != 0).double().view(-1, 1)
        return x_new, out
    out = _ln64(t, w2, b2, eps) if w2 is not None else t
    return t, (out if kind == LN2_F32 else rnd(out))


def conv_module_op_ref(glu, desc, wdw_t, bdw, lnw, lnb, eps, out_rows, emulate=None):
    """-> [out_rows, d] float64, rows no descriptor covers NaN.  glu [rows, d]: row SRC_ROW0 + j is window column j;
    only the columns in [J_LO, J_HI) are touched (the others may hold anything, NaN included)."""
    rnd = _rnd(emulate)
    g = glu.double()
    d = g.shape[1]
    w = rnd(wdw_t.float()).double()
    out = torch.full((out_rows, d), float("nan"), dtype=torch.float64)
    for o0, nout, s0, jlo, jhi, *_ in desc.tolist():
        if nout <= 0:
            continue
        j = torch.arange(nout)[:, None] + torch.arange(15)[None, :]            # window column of (row i, tap t)
        real = (j >= jlo) & (j < jhi)
        rows = s0 + j
        assert not real.any() or (rows[real].min() >= 0 and rows[real].max() < g.shape[0])
        xs = torch.where(real[..., None], g[rows.clamp(0, g.shape[0] - 1)], torch.zeros((), dtype=torch.float64))
        z = _ln64(bdw.double() + torch.einsum("itc,tc->ic", xs, w), lnw, lnb, eps)
        out[o0: o0 + nout] = rnd(z * torch.sigmoid(z))
    return out


def pos_angle_f32(d, p_rows, anchor):
    """[p_rows, d / 2] f32 angles |p| * div_i (both factors f32) and the [p_rows] distances p = anchor - k"""
    p = anchor - torch.arange(p_rows)
    div = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
    return p.abs().float().unsqueeze(1) * div, p


def pos_table_op_ref(d, p_rows, anchor, emulate=None):
    rnd = _rnd(emulate)
    a, p = pos_angle_f32(d, p_rows, anchor)
    a = a.double()
    out = torch.empty(p_rows, d, dtype=torch.float64)
    out[:, 0::2] = torch.sin(a) * torch.where(p < 0, -1.0, 1.0).double().unsqueeze(1)
    out[:, 1::2] = torch.cos(a)
    return rnd(out)
