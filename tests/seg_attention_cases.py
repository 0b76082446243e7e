"""Cases of the segment attention operator (cfm_op_seg_attention, include/cfm_ops.h) and its float64 reference,
shared by the CPU and GPU tests of tests/test_gpu_rescore_ops.py.

One call holds every segment of the grid: NQ in {1, 16, 17, 65} x NK in {0, 1, 63, 64, 65, 129} x {all keys, causal}.
Query segments are laid out one after another with 1 to 3 rows between them that no descriptor covers (so they start
at unaligned rows); the key ranges, one per NK, are laid out the same way and each is shared by the eight query
segments with that NK.  Uncovered rows hold NaN: one that is read reaches an output.
"""
import functools
from types import SimpleNamespace

import torch

H = 2
NQS = (1, 16, 17, 65)
NKS = (0, 1, 63, 64, 65, 129)
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SQ = 1.5      # scale of q: the scores q . k / sqrt(dk) then have a standard deviation of about 1.5
FIELDS = ("Q0", "NQ", "K0", "NK", "CAUSAL")


@functools.lru_cache(maxsize=None)
def geometry():
    k0, kpos = {}, 2
    for nk in NKS:
        k0[nk] = kpos
        kpos += nk + 1 + nk % 3
    desc, qpos = [], 3
    for causal in (0, 1):
        for nk in NKS:
            for nq in NQS:
                desc.append([qpos, nq, k0[nk], nk, causal, 0, 0, 0])
                qpos += nq + 1 + (nq + nk) % 3
    return SimpleNamespace(desc=torch.tensor(desc, dtype=torch.int32), q_rows=qpos + 2, k_rows=kpos + 2)


def seg_attention_ref(q, kv, desc, H, dk, emulate=None):
    """float64 reference: out [q_rows, H * dk], NaN in rows no descriptor covers.  emulate (a 16-bit torch dtype):
    q, k, v, the un-normalised probabilities exp(s - max) and the output are rounded to it, the rest stays float64."""
    rnd = (lambda t: t.to(emulate).double()) if emulate is not None else (lambda t: t)
    d = H * dk
    out = torch.full((q.shape[0], d), float("nan"), dtype=torch.float64)
    qd, kd, vd = rnd(q.double()), rnd(kv[:, :d].double()), rnd(kv[:, d:].double())
    for q0, nq, k0, nk, causal, *_ in desc.tolist():
        for h in range(H):
            c = slice(h * dk, (h + 1) * dk)
            s = qd[q0: q0 + nq, c] @ kd[k0: k0 + nk, c].T / dk ** 0.5
            vis = torch.ones(nq, nk, dtype=torch.bool)
            if causal:
                vis = torch.arange(nk)[None, :] <= torch.arange(nq)[:, None]
            s = s.masked_fill(~vis, float("-inf"))
            mx = s.max(dim=1, keepdim=True).values if nk else torch.zeros(nq, 1, dtype=torch.float64)
            p = torch.where(vis, torch.exp(s - mx), torch.zeros_like(s))
            den = p.sum(dim=1, keepdim=True)
            o = rnd(p) @ vd[k0: k0 + nk, c] / torch.where(den > 0, den, torch.ones_like(den))
            out[q0: q0 + nq, c] = rnd(o)
    return out


@functools.lru_cache(maxsize=None)
def case(dt: str, dk: int):
    """Inputs in dtype `dt` (the same seeded values for every dtype, rounded to it) and their float64 reference."""
    g = geometry()
    d = H * dk
    gen = torch.Generator().manual_seed(1000 + dk)
    c = SimpleNamespace(g=g, dt=dt, dk=dk, d=d)
    q = SQ * torch.randn(g.q_rows, d, generator=gen)
    kv = torch.randn(g.k_rows, 2 * d, generator=gen)
    qc, kc = torch.zeros(g.q_rows, dtype=torch.bool), torch.zeros(g.k_rows, dtype=torch.bool)
    for q0, nq, k0, nk, *_ in g.desc.tolist():
        qc[q0: q0 + nq] = True
        kc[k0: k0 + nk] = True
    q[~qc] = float("nan")
    kv[~kc] = float("nan")
    c.q, c.kv, c.q_covered = q.to(TDT[dt]), kv.to(TDT[dt]), qc
    c.ref = seg_attention_ref(c.q, c.kv, g.desc, H, dk)
    return c


def rel_err(got, exp):
    """max-abs difference relative to the exact output's max-abs, over the rows the descriptors cover"""
    m = ~torch.isnan(exp)
    return ((got.double() - exp)[m].abs().max() / exp[m].abs().max()).item()


def e_round(dt: str, dk: int) -> float:
    """the rounding a correct `dt` kernel must incur (no kernel involved), relative to the output's max-abs"""
    c = case(dt, dk)
    return rel_err(seg_attention_ref(c.q, c.kv, c.g.desc, H, dk, emulate=TDT[dt]), c.ref)


def _matters(field: int, delta: int, row) -> bool:
    """the change alters what the segment computes (e.g. a causal segment never reads keys past its last query)"""
    q0, nq, k0, nk, causal = row[:5]
    if field == 2:
        return nk > 0
    if field == 3:
        seen = min(nk, nq) if causal else nk
        return (min(nk + delta, nq) if causal else nk + delta) != seen
    if field == 4:
        return nk > 1
    return nk > 0      # Q0 / NQ: without keys every row is zero; the NaN guard of the GPU test sees those


def one_off_error(dt: str, dk: int, field: int, delta: int) -> float:
    """the smallest error, over the segments where the change is legal and matters, of the exact operator run with
    descriptor field `field` off by `delta` (CAUSAL: flipped) in that one segment, relative to the output's max-abs;
    a row the true segment covers and the changed one does not write counts with its full value, and so does a row
    written where nothing should be"""
    c = case(dt, dk)
    g = c.g
    gen = torch.Generator().manual_seed(7)      # a shifted range touches uncovered rows: random values there
    q = torch.where(torch.isnan(c.q.float()), SQ * torch.randn(c.q.shape, generator=gen), c.q.float()).to(TDT[dt])
    kv = torch.where(torch.isnan(c.kv.float()), torch.randn(c.kv.shape, generator=gen), c.kv.float()).to(TDT[dt])
    scale = c.ref[~torch.isnan(c.ref)].abs().max()
    worst = float("inf")
    for s, row in enumerate(g.desc.tolist()):
        q0, nq, k0, nk, causal = row[:5]
        new = list(row)
        new[field] = (1 - causal) if field == 4 else row[field] + delta
        if not _matters(field, delta, row) or new[1] < 1 or min(new[0], new[2], new[3]) < 0:
            continue
        if new[0] + new[1] > g.q_rows or new[2] + new[3] > g.k_rows:
            continue
        got = seg_attention_ref(q, kv, torch.tensor([new], dtype=torch.int32), H, dk)
        lo, hi = min(q0, new[0]), max(q0 + nq, new[0] + new[1])
        exp, got = c.ref[lo:hi], got[lo:hi]
        both = ~torch.isnan(exp) & ~torch.isnan(got)
        diff = torch.where(both, (got - exp).abs(), torch.nan_to_num(got, nan=0.0).abs() + torch.nan_to_num(exp, nan=0.0).abs())
        own = torch.zeros(hi - lo, dtype=torch.bool)     # rows of the true or the changed segment only
        own[q0 - lo: q0 + nq - lo] = True
        own[new[0] - lo: new[0] + new[1] - lo] = True
        worst = min(worst, (diff[own].max() / scale).item())
    return worst
