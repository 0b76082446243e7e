"""Seeded inputs, descriptors and fp64 reference outputs of every case of the row-wise operator tests
(cfm_op_layernorm, cfm_op_conv_module, cfm_op_pos_table): shared by tests/test_gpu_ops_rowwise.py (the kernels)
and tests/test_rowwise_op_ref_cpu.py (the references and the tolerances).  Conv descriptors and the (p_rows,
anchor) pairs come from the project's host planners (chunkformer_amd/csrc/planner.cpp, no GPU); no descriptor here
is hand-written.  Everything is CPU-only and cached: a case is built once and must not be modified by its users.
"""
import functools
import zlib
from types import SimpleNamespace

import torch

from chunkformer_amd import _lib
from oracle import rowwise_op_ref as R

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTS = ["fp32", "bf16", "fp16"]
DS = [128, 256, 512]
GUARD = 4            # NaN rows after the last row of every output (and of the GLU stream)
OUTSIDE = 8.0        # GLU rows outside every descriptor's real range: this much larger in the un-poisoned copy
EPS = 1e-5           # the model's norm_eps


def feat_rows(m: int) -> int:
    """feature rows that subsample to m frames (1 + (T - 15) // 8 = m); m = 0: a T < 15 utterance"""
    return 8 * m + 7


def rel_err(got, exp):
    """max-abs difference relative to the exact output's max-abs, over the non-NaN rows of `exp`"""
    m = ~torch.isnan(exp)
    return ((got.double() - exp)[m].abs().max() / exp[m].abs().max()).item()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# =================================================================================== LayerNorm
# kernel variants: LN (ln_kernel), LN2 with / without the second LayerNorm and LN2_F32 (ln2_kernel)
LN_KINDS = {"ln": (R.LN, False), "ln2_w2": (R.LN2, True), "ln2": (R.LN2, False), "ln2_f32": (R.LN2_F32, True)}
LN_M = [1, 2, 3, 4, 5, 7, 8, 9, 1001]
# residual forms: branches (0, 1, 2), mask on branch 1 / 2, defer, rowmask
_F = lambda nb, m1=False, m2=False, defer=False, rowmask=False: SimpleNamespace(nb=nb, m1=m1, m2=m2, defer=defer,
                                                                               rowmask=rowmask)
LN_FORMS = {"none": _F(0), "y": _F(1), "y_m": _F(1, True), "yy": _F(2), "yy_m1": _F(2, True), "yy_m2": _F(2, m2=True),
            "yy_m12": _F(2, True, True), "y_defer": _F(1, defer=True), "y_m_defer": _F(1, True, defer=True),
            "yy_m12_defer": _F(2, True, True, defer=True), "none_rowmask": _F(0, rowmask=True),
            "yy_m12_rowmask": _F(2, True, True, rowmask=True)}
ALPHA, ALPHA2 = 0.5, 1.0     # the model's FFN / attention branch scales: distinct, so a swap shows
# row kinds, cycling with the row index (shifted per case so that M = 1 sees every kind):
#   0 N(0, 1)   1 mean 30, std 1   2 std 1e-2 (eps is 10 % of the variance)   3 exactly constant
#   4 std 2e-3 (eps is 2.5 x the variance: where a dropped eps clears the 16-bit bars too)
N_ROWKINDS = 5
ROW_STD = [1.0, 1.0, 1e-2, 0.0, 2e-3]
# constant rows hold multiples of 1/4 (y: 1/2), so every partial sum of the row is exact in f32 in any order and
# the kernel's mean is the constant itself: out = b up to the output rounding (a mean that is off by one ulp
# would be amplified by 1 / sqrt(eps) = 316, which is f32 LayerNorm, not a kernel error)
CONSTS = [0.5, 1.5, -2.25, 3.0]


def ln_forms(kindv):
    return [f for f, v in LN_FORMS.items() if kindv == "ln" or not (v.defer or v.rowmask)]


def ln_case_list(kindv):
    """(M, form): every M with the forms cycling, and every form at M = 7 (odd, not a multiple of 4: the duplicated
    last row and early-exit waves) and M = 1001"""
    forms = ln_forms(kindv)
    out = [(M, forms[i % len(forms)]) for i, M in enumerate(LN_M)]
    out += [(M, f) for M in (7, 1001) for f in forms]
    return list(dict.fromkeys(out))


def row_kinds(M, shift):
    return (torch.arange(M) + shift) % N_ROWKINDS


@functools.lru_cache(maxsize=None)
def ln_case(kindv, d, M, form, dt):
    """inputs (the same seeded values for every dtype, y / y2 rounded to it) and the fp64 reference"""
    kind, has_w2 = LN_KINDS[kindv]
    f, tdt = LN_FORMS[form], TDT[dt]
    g = _gen("ln", kindv, d, M, form)
    shift = zlib.crc32(repr((kindv, M, form)).encode()) % N_ROWKINDS
    rk = row_kinds(M, shift)
    std = torch.tensor(ROW_STD)[rk].view(M, 1)
    const = torch.tensor(CONSTS)[torch.arange(M) % len(CONSTS)].view(M, 1)
    is_c = (rk == 3).view(M, 1)

    def rows(mean30, cscale):
        t = torch.randn(M, d, generator=g) * std
        if mean30:
            t = t + 30.0 * (rk == 1).float().view(M, 1)
        return torch.where(is_c, (const * cscale).expand(M, d), t)

    c = SimpleNamespace(kindv=kindv, kind=kind, d=d, M=M, form=form, f=f, dt=dt, rk=rk)
    c.x = rows(True, 1.0)
    c.y = rows(False, 2.0).to(tdt) if f.nb >= 1 else None
    c.y2 = rows(False, -1.0).to(tdt) if f.nb >= 2 else None
    r = torch.arange(M)
    c.ymask = ((r * 7 + 3) % 3 != 0).to(torch.uint8) if f.m1 else None       # zeros at rows 0, 3, 6, ..
    c.ymask2 = ((r * 5 + 1) % 4 != 0).to(torch.uint8) if f.m2 else None      # zeros at rows 3, 7, 11, ..
    c.rowmask = ((r + 1) % 3 != 0).to(torch.uint8) if f.rowmask else None    # zeros at rows 2, 5, 8, ..
    c.w1 = 1.0 + 0.3 * torch.randn(d, generator=g)
    c.b1 = 0.3 * torch.randn(d, generator=g)
    c.w2 = 1.0 + 0.3 * torch.randn(d, generator=g) if has_w2 else None
    c.b2 = 0.3 * torch.randn(d, generator=g) if has_w2 else None
    c.kw = dict(y=c.y, alpha=ALPHA, ymask=c.ymask, y2=c.y2, alpha2=ALPHA2, ymask2=c.ymask2, defer=f.defer,
                w2=c.w2, b2=c.b2, rowmask=c.rowmask)
    c.x_ref, c.ref = R.layernorm_op_ref(kind, c.x, c.w1, c.b1, EPS, **c.kw)
    c.scale = c.ref.abs().max().item()
    return c


def ln_e_round(kindv, d, M, form, dt):
    c = ln_case(kindv, d, M, form, dt)
    _, emu = R.layernorm_op_ref(c.kind, c.x, c.w1, c.b1, EPS, emulate=TDT[dt], **c.kw)
    return rel_err(emu, c.ref)


def ln_all_cases():
    return [(kv, d, M, f) for kv in LN_KINDS for d in DS for M, f in ln_case_list(kv)]


# =================================================================================== conv module
# ("masked", C, R, offsets): plan_masked over 5 utterances (see masked_lens); NOUT = C for C <= 64, C = 128 gives two
#     descriptors per chunk, the second with q0 = 64 and a negative J_LO.  offsets: per-utterance carried offset
#     (first chunks with J_LO = 7 at offset 0, J_LO = max(0, 7 - o) at a positive one)
# ("padded", T', C): plan_padded, two utterances of T' and max(1, 2 T' / 3) frames; C <= 0: full attention
#     (the first utterance has SRC_ROW0 = -7)
# ("stream", T', C, R): plan_stream with L = 32, offset 5: GLUOFF = 7, T' < C + R
CONV_KEYS = [("masked", 64, 8, (0, 3, 10, 0, 0)),      # full chunks
             ("masked", 48, 3, (0, 0, 2, 0, 7)),       # the second half-block partly filled, whole waves exit
             ("masked", 32, 0, (0, 3, 10, 0, 0)),      # the dot2h second block exits
             ("masked", 16, 8, (0, 0, 0, 0, 0)),
             ("masked", 128, 3, (0, 3, 10, 0, 0)),     # two descriptors per chunk
             ("masked", 8, 0, (0, 0, 0, 0, 0)),        # window shorter than the taps; R = 0: the C + R + 7 limit
             ("masked", 8, 8, (5, 0, 9, 0, 1)),
             ("padded", 1, -1), ("padded", 33, -1), ("padded", 70, -1), ("padded", 130, -1),
             ("padded", 70, 16),
             ("stream", 70, 64, 16), ("stream", 20, 16, 8)]


def masked_lens(C):
    """9 + 1 + 8 + 1 + 4 = 23 chunks: windows clipped at both edges of every utterance, a one-chunk utterance of
    5 frames, a last chunk of a single frame (7C + 1), a T < 15 utterance (an empty window: J_HI <= J_LO)"""
    return [feat_rows(x) for x in (8 * C + C // 2, 5, 7 * C + 1, 0, 3 * C + 5)]


@functools.lru_cache(maxsize=None)
def conv_geometry(key):
    kind = key[0]
    if kind == "masked":
        _, C, Rc, offs = key
        plan, _, _ = _lib.plan_masked(masked_lens(C), list(offs), C, 16, Rc)
    elif kind == "padded":
        _, tp, C = key
        lens = [feat_rows(tp), feat_rows(max(1, 2 * tp // 3))]
        plan, tp2 = _lib.plan_padded(lens, feat_rows(tp), C, 8 if C > 0 else 0, 4 if C > 0 else 0)
        assert tp2 == tp
    else:
        _, tp, C, Rc = key
        plan, tp2 = _lib.plan_stream(feat_rows(tp), C, 32, Rc, 5)
        assert tp2 == tp
    h = plan[:_lib.PLAN_HEADER].tolist()
    off = _lib.PLAN_HEADER + _lib.PLAN_REC * (h[1] + h[2])
    g = SimpleNamespace(desc=plan[off: off + _lib.PLAN_REC * h[3]].view(-1, _lib.PLAN_REC).clone(), rows=h[4],
                        glu_rows=h[13], gluoff=h[15], kind=h[0])
    # the real range of every descriptor: the columns a kernel may read, as stream rows
    g.real = torch.zeros(g.glu_rows + GUARD, dtype=torch.bool)
    for o0, nout, s0, jlo, jhi, *_ in g.desc.tolist():
        assert 0 < nout <= 64 and 0 <= o0 and o0 + nout <= g.rows
        lo, hi = max(jlo, 0), min(jhi, nout + 14)
        if hi > lo:
            assert 0 <= s0 + lo and s0 + hi <= g.glu_rows, "a descriptor's real range leaves the GLU stream"
            g.real[s0 + lo: s0 + hi] = True
    return g


@functools.lru_cache(maxsize=None)
def conv_case(key, d, dt):
    g, tdt = conv_geometry(key), TDT[dt]
    gen = _gen("conv", key, d)
    c = SimpleNamespace(g=g, d=d, dt=dt, key=key)
    full = torch.randn(g.glu_rows + GUARD, d, generator=gen)
    full[~g.real] *= OUTSIDE
    c.glu_full = full.to(tdt)                     # for the CPU guard's mutated references
    glu = full.clone()
    glu[~g.real] = float("nan")                   # what the kernels get: one read outside a real range reaches out
    c.glu = glu.to(tdt)
    c.wdw = 0.3 * torch.randn(15, d, generator=gen)
    c.bdw = 0.3 * torch.randn(d, generator=gen)
    c.lnw = 1.0 + 0.3 * torch.randn(d, generator=gen)
    c.lnb = 0.3 * torch.randn(d, generator=gen)
    c.ref = R.conv_module_op_ref(c.glu, g.desc, c.wdw, c.bdw, c.lnw, c.lnb, EPS, g.rows)
    c.scale = c.ref[~torch.isnan(c.ref)].abs().max().item()
    return c


def conv_e_round(key, d, dt):
    c = conv_case(key, d, dt)
    emu = R.conv_module_op_ref(c.glu, c.g.desc, c.wdw, c.bdw, c.lnw, c.lnb, EPS, c.g.rows, emulate=TDT[dt])
    return rel_err(emu, c.ref)


def conv_all_cases():
    return [(k, d) for k in CONV_KEYS for d in DS]


# =================================================================================== pos_table
def _plan_pos(plan):
    h = plan[:_lib.PLAN_HEADER].tolist()
    return h[10], h[11]


@functools.lru_cache(maxsize=None)
def pos_shapes():
    """name -> (p_rows, anchor), from a masked, a padded-full and a stream plan, and the table's far end"""
    return {"masked": _plan_pos(_lib.plan_masked(masked_lens(64), None, 64, 128, 128)[0]),
            "padded_full": _plan_pos(_lib.plan_padded([feat_rows(130), feat_rows(86)], feat_rows(130), -1, 0, 0)[0]),
            "stream": _plan_pos(_lib.plan_stream(feat_rows(70), 64, 128, 16, 40)[0]),
            "far": (130, 4998),            # distances 4998 .. 4869: the largest angles of the table
            "whole": (9997, 4998)}         # every distance of the reference's table, -4998 .. 4998


POS_KEYS = ["masked", "padded_full", "stream", "far", "whole"]
POS_D = [128, 512]


@functools.lru_cache(maxsize=None)
def pos_case(name, d):
    p_rows, anchor = pos_shapes()[name]
    c = SimpleNamespace(p_rows=p_rows, anchor=anchor, d=d)
    c.ref = R.pos_table_op_ref(d, p_rows, anchor)
    a, _ = R.pos_angle_f32(d, p_rows, anchor)
    ulp = torch.nextafter(a, torch.full_like(a, float("inf"))) - a          # ulp_f32 of the angle
    c.angle_ulp = ulp.double().repeat_interleave(2, dim=1)                  # the sin and the cos column
    return c
