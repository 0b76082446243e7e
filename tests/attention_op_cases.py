"""Seeded inputs, descriptors and the fp64 reference output of every attention-operator case: shared by
tests/test_gpu_ops_attention.py (the kernels) and tests/test_attention_op_ref_cpu.py (the reference and the
tolerance).  Descriptors come from the project's host planners (chunkformer_amd/csrc/planner.cpp, no GPU);
everything here is CPU-only and cached: a case is built once and must not be modified by its users.

A geometry key is one of
    ("masked", C, L, R, batch)           plan_masked; batch: "std" (23 chunks, 5 utterances) or "n1" / "n2" / "n3"
    ("padded", C, L, R)                  plan_padded, chunked, two utterances of 150 and 100 frames
    ("dense", T')                        plan_padded with chunk_size <= 0 (full attention), three utterances
    ("stream", offset, shift)            plan_stream (C 64, L 128, R 16, 70 frames); shift > 0 is the hand-written
                                         variant whose window starts `shift` rows before the KV buffer
"""
import functools
import zlib
from types import SimpleNamespace

import torch

from chunkformer_amd import _lib
from oracle.attention_op_ref import attention_op_ref

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
H = 2
GUARD = 4              # NaN rows after kv_rows and after the last query row
OUTSIDE = 8.0          # KV rows no window may read (a neighbour utterance's data) are this much larger
# N(0, 1) keys and values; queries at 1.6 and rel-pos rows at 1.2 give the content term of a score a standard
# deviation of 1.6 and the rel-pos term one of 1.9 after the 1/sqrt(dk) scaling, at either head dim: a peaked
# softmax, in which a wrong mask edge, skew or key row moves the output (see `sharp`)
SQ, SP, SUV = 1.6, 1.2, 0.3


def feat_rows(m: int) -> int:
    """feature rows that subsample to m frames (1 + (T - 15) // 8 = m); m = 0: a T < 15 utterance"""
    return 8 * m + 7


def masked_lens(C: int, batch: str = "std"):
    """std: 9 + 1 + 8 + 1 + 4 = 23 chunks: windows clipped at both edges of every utterance, a one-chunk
    utterance of 5 frames, a last chunk of a single frame (7C + 1), a T < 15 utterance (no valid key)"""
    m = {"std": [8 * C + C // 2, 5, 7 * C + 1, 0, 3 * C + 5], "n1": [5], "n2": [C + 3], "n3": [2 * C + 1]}[batch]
    return [feat_rows(x) for x in m]


def _desc(plan):
    h = plan[:_lib.PLAN_HEADER].tolist()
    off = _lib.PLAN_HEADER + _lib.PLAN_REC * h[1]
    return plan[off: off + _lib.PLAN_REC * h[2]].view(-1, _lib.PLAN_REC).clone(), h


@functools.lru_cache(maxsize=None)
def geometry(key):
    kind = key[0]
    g = SimpleNamespace(nutt=0, nd=0, t_keys=0)
    if kind == "masked":
        _, C, L, R, batch = key
        plan, nch, _ = _lib.plan_masked(masked_lens(C, batch), None, C, L, R)
        g.desc, h = _desc(plan)
        g.C, g.W, g.n_chunks = C, L + C + R, sum(nch)
    elif kind == "padded":
        _, C, L, R = key
        plan, tp = _lib.plan_padded([feat_rows(150), feat_rows(100)], feat_rows(150), C, L, R)
        g.desc, h = _desc(plan)
        g.C, g.W = C, L + C + R
    elif kind == "dense":
        tp = key[1]
        lens = [feat_rows(tp), feat_rows(max(1, 2 * tp // 3)), feat_rows(tp // 3)]
        plan, tp2 = _lib.plan_padded(lens, feat_rows(tp), -1, 0, 0)
        assert tp2 == tp
        g.desc, h = _desc(plan)
        g.C, g.W, g.nutt, g.nd, g.t_keys = tp, tp, 3, (tp + 63) // 64, tp
    else:
        _, offset, shift = key
        plan, tp = _lib.plan_stream(feat_rows(70), 64, 128, 16, offset)
        g.desc, h = _desc(plan)
        g.C, g.W = 64, 128 + 64 + 16
        assert 0 <= shift <= int(g.desc[:, 3].min())   # rows below KEY_LO are never read (the contract)
        g.desc[:, 2] -= shift
        h[12] -= shift
    g.q_rows, g.p_rows, g.kv_rows = h[4], h[10], h[12]
    return g


def rel_err(got, exp):
    """max-abs difference relative to the exact output's max-abs, over the rows the descriptors cover"""
    m = ~torch.isnan(exp)
    return ((got.double() - exp)[m].abs().max() / exp[m].abs().max()).item()


@functools.lru_cache(maxsize=None)
def case(key, dt: str, dk: int, pcol: bool = False):
    """Inputs in dtype `dt` (the same seeded values for every dtype, rounded to it) and their fp64 reference.
    pcol: P is the middle third of a [p_rows, 3 d] table (p_ld = 3 d, the layer-1 column of a 3-layer table)."""
    g = geometry(key)
    tdt, d = TDT[dt], H * dk
    gen = torch.Generator().manual_seed(zlib.crc32(repr((key, dk)).encode()))
    c = SimpleNamespace(g=g, dt=dt, dk=dk, d=d)
    c.q = (SQ * torch.randn(g.q_rows, d, generator=gen)).to(tdt)
    kv = torch.randn(g.kv_rows + GUARD, 2 * d, generator=gen)
    inside = torch.zeros(g.kv_rows + GUARD, dtype=torch.bool)
    for _, _, kv0, lo, hi, _, _, _ in g.desc.tolist():
        inside[max(kv0 + lo, 0): max(kv0 + hi, 0)] = True
    kv[~inside] *= OUTSIDE
    kv[g.kv_rows:] = float("nan")
    c.kv = kv.to(tdt)
    ptab = SP * torch.randn(g.p_rows, 3 * d if pcol else d, generator=gen)
    if pcol:
        ptab[:, :d] *= OUTSIDE
        ptab[:, 2 * d:] *= OUTSIDE
    c.ptab = ptab.to(tdt)
    c.P = c.ptab[:, d: 2 * d] if pcol else c.ptab          # a view: row stride p_ld
    c.p_ld = c.ptab.shape[1]
    c.u = SUV * torch.randn(d, generator=gen)
    c.v = SUV * torch.randn(d, generator=gen)
    terms = []
    c.ref = attention_op_ref(c.q, c.kv[: g.kv_rows], c.P, c.u, c.v, g.desc, H, dk, terms=terms)
    c.scale = c.ref[~torch.isnan(c.ref)].abs().max().item()
    # input sharpness: std of the content and of the rel-pos term over every (head, query, key) of the case
    c.n_scores = sum(t.numel() for t in terms[0::2])
    c.sharp = (torch.cat(terms[0::2]).std().item(), torch.cat(terms[1::2]).std().item()) if c.n_scores > 1 else None
    return c


def e_round(key, dt: str, dk: int, pcol: bool = False) -> float:
    """the rounding a correct `dt` kernel must incur on this case, relative to the output's max-abs (no kernel
    involved: the reference with emulate=dt against the exact reference)"""
    c = case(key, dt, dk, pcol)
    emu = attention_op_ref(c.q, c.kv[: c.g.kv_rows], c.P, c.u, c.v, c.g.desc, H, dk, emulate=TDT[dt])
    return rel_err(emu, c.ref)


# ---------------------------------------------------------------------------------- the case lists
GENERIC_KEYS = [("masked", 64, 128, 128, "std"), ("masked", 16, 8, 4, "std"),
                ("masked", 80, 16, 16, "std"),      # C > 64: two query sub-blocks per chunk
                ("masked", 24, 63, 0, "std"),       # W odd
                ("padded", 64, 32, 16),             # short last chunk, Q_VALID < NQ, KV_ROW0 < 0 at the first chunk
                ("stream", 40, 0),                  # KEY_LO = 88 > 0
                ("stream", 40, 50)]                 # hand-written: KV_ROW0 = -50
RING_SHAPES = [(64, 0, 0), (64, 64, 0), (64, 64, 64), (64, 128, 64), (64, 128, 128),      # NT = 1..5
               (48, 16, 32), (16, 32, 32),                                                # W % 64 != 0: NT = 0
               (32, 160, 128),                                                            # W = 320 at C = 32
               (64, 62, 0), (32, 30, 0), (16, 18, 16), (64, 126, 128)]                    # W = 2 (mod 4)
RING_SMALL = [(64, 128, 128), (64, 62, 0), (16, 18, 16)]                                  # at 1, 2 and 3 chunks
RING_REFUSED = [(16, 9, 4), (80, 16, 16), (64, 130, 128), (64, 256, 64)]   # W odd; C = 80; W = 322; W + C > 384
A128_SHAPES = [(64, 0, 0), (64, 64, 0), (64, 64, 64), (64, 128, 64), (64, 128, 128)]      # W = 64 .. 320
A128_REFUSED = [(64, 16, 16)]                                                             # W = 96
DENSE_T = [1, 63, 64, 65, 128, 129, 383, 384]
DENSE_REFUSED_T = 385
PCOL_KEY = ("masked", 16, 8, 4, "std")


def all_cases(dt: str):
    """every (key, dk, pcol) the GPU tests run on 16-bit type `dt`: the list E_round is the maximum over"""
    out = [(k, dk, False) for k in GENERIC_KEYS for dk in (64, 128)]
    out += [(PCOL_KEY, dk, True) for dk in (64, 128)]
    out += [(("masked", C, L, R, "std"), 64, False) for C, L, R in RING_SHAPES]
    out += [(("masked", C, L, R, b), 64, False) for C, L, R in RING_SMALL for b in ("n1", "n2", "n3")]
    out += [(("masked", 64, 128, 128, "std"), 64, True)]
    if dt == "bf16":
        out += [(("masked", C, L, R, "std"), 128, False) for C, L, R in A128_SHAPES]
        out += [(("masked", 64, 128, 128, b), 128, False) for b in ("n1", "n2", "n3")]
        out += [(("dense", t), 64, False) for t in DENSE_T]
    return list(dict.fromkeys(out))
