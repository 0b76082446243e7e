"""ORACLE — test infrastructure only.  Float64 CPU reference of the attention *operator*
(cfm_op_attention, include/cfm_ops.h), written from the descriptor contract alone.

For each descriptor (Q_ROW0, NQ, KV_ROW0, KEY_LO, KEY_HI, P_BASE, Q_VALID, -) and head h, with i < NQ and
j in [KEY_LO, KEY_HI):
    s[i, j] = ((q_i + u) . K[KV_ROW0 + j] + (q_i + v) . P[P_BASE - i + j]) / sqrt(dk)
    out_i   = softmax_j(s[i, :]) . V
rows i >= Q_VALID and rows with an empty key range give 0.  KV rows are [H][K dk | V dk]; P is a
[p_rows, >= H*dk] tensor (a strided view stands for p_ld), head h at column h*dk.

emulate=<16-bit dtype> rounds q+u, q+v, the un-normalised probabilities (the numerator's; the
denominator sums them unrounded) and the output to that type and nothing else: the roundings a kernel
on that type cannot avoid.  It sizes the tests' tolerance and is never compared with a kernel.
"""
import math

import torch


def attention_op_ref(q, kv, P, pos_u, pos_v, desc, H, dk, emulate=None, terms=None):
    """-> [q rows, H*dk] float64; rows no descriptor covers are NaN.  terms (a list) receives the
    scaled content and rel-pos terms (two flat tensors per descriptor) for input-sharpness checks."""
    rnd = (lambda t: t.to(emulate).double()) if emulate is not None else (lambda t: t)
    q, kv = q.double(), kv.double()
    Ph = P[:, : H * dk].double().reshape(-1, H, dk)
    u, v = pos_u.double().view(H, dk), pos_v.double().view(H, dk)
    out = torch.full((q.shape[0], H * dk), float("nan"), dtype=torch.float64)
    for q0, nq, kv0, lo, hi, pb, qvalid, _ in desc.tolist():
        out[q0: q0 + nq] = 0.0
        n = min(nq, qvalid)
        if n <= 0 or hi <= lo:
            continue
        idx = pb - torch.arange(n)[:, None] + torch.arange(lo, hi)[None, :]          # P row of (i, j)
        assert kv0 + lo >= 0 and kv0 + hi <= kv.shape[0] and idx.min() >= 0 and idx.max() < Ph.shape[0]
        qq = q[q0: q0 + n].view(n, H, dk)
        kw = kv[kv0 + lo: kv0 + hi].view(hi - lo, H, 2 * dk)
        ac = torch.einsum("ihd,jhd->hij", rnd(qq + u), kw[..., :dk]) / math.sqrt(dk)
        bd = torch.einsum("ihd,khd->hik", rnd(qq + v), Ph).gather(2, idx.expand(H, n, hi - lo)) / math.sqrt(dk)
        if terms is not None:
            terms += [ac.flatten(), bd.flatten()]
        s = ac + bd
        p = torch.exp(s - s.amax(-1, keepdim=True))
        o = torch.einsum("hij,jhd->ihd", rnd(p), kw[..., dk:]) / p.sum(-1).t()[..., None]
        out[q0: q0 + n] = rnd(o.reshape(n, H * dk))
    return out
