"""CPU-side guard of the attention-operator parity tests (tests/test_gpu_ops_attention.py): the fp64 reference
is pinned to oracle/encoder_ref.py's attention, the E_round table the 16-bit bars come from is recomputed, and
the bars are shown to see the errors a kernel can make silently -- on the tests' own inputs each mutation of
the reference must move the output by at least 10 x the bar."""
import pytest
import torch

import attention_op_cases as A
from oracle import encoder_ref
from oracle.attention_op_ref import attention_op_ref
from test_gpu_ops_attention import BAR, E_ROUND

MARGIN = 10.0
# the W = 2 (mod 4) ring shapes whose 23-chunk batch is longer than the 384-row ring: where a staging that
# assumed W % 4 == 0 left stale rows, and what such rows hold there (other utterances' keys, padding)
GUARD_KEYS = [("masked", 64, 62, 0, "std"), ("masked", 32, 30, 0, "std"), ("masked", 64, 126, 128, "std")]


def test_reference_matches_encoder_oracle():
    """the masked-batch attention of oracle/encoder_ref.py (gathered windows, boolean key masks) on the
    descriptors' batch: the two references share no code"""
    C, Lc, R = 16, 8, 4
    c = A.case(("masked", C, Lc, R, "std"), "fp32", 64)
    g, W, dk = c.g, Lc + C + R, 64
    N = g.n_chunks
    flat = c.kv[: g.kv_rows].view(g.kv_rows, A.H, 2 * dk)
    win = flat[torch.arange(N)[:, None] * C + torch.arange(W)[None, :]]
    j = torch.arange(W)[None, :]
    mask = ((j >= g.desc[:, 3:4]) & (j < g.desc[:, 4:5])).unsqueeze(1)
    o = encoder_ref._attention_core(c.q.view(N, C, A.H, dk), win[..., :dk], win[..., dk:], c.P.view(-1, A.H, dk),
                                    c.u.view(A.H, dk), c.v.view(A.H, dk), mask, dk)
    assert torch.isfinite(o).all()
    assert A.rel_err(o.reshape(N * C, -1), c.ref) <= 1e-5


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_e_round_table(dt):
    """the constants of the GPU test are the measured maximum over its whole case list (rounded up)"""
    worst = max(A.e_round(key, dt, dk, pcol) for key, dk, pcol in A.all_cases(dt))
    print(f"E_round({dt}) = {worst:.3e}")
    assert 0.9 * E_ROUND[dt] <= worst <= E_ROUND[dt]


def _mutated(c, desc=None, P=None):
    return attention_op_ref(c.q, c.kv[: c.g.kv_rows], c.P if P is None else P, c.u, c.v,
                            c.g.desc if desc is None else desc, A.H, c.dk)


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("key", GUARD_KEYS, ids=lambda k: "-".join(map(str, k)))
def test_bar_sees_descriptor_and_stale_row_errors(key, dt):
    c = A.case(key, dt, 64)
    g, need = c.g, MARGIN * BAR[dt]
    lo, hi, kv0 = g.desc[:, 3], g.desc[:, 4], g.desc[:, 2]
    seen = {}
    # P_BASE + 1 (the table gets one more row so that the shifted reads stay inside it)
    d = g.desc.clone()
    d[:, 5] += 1
    seen["P_BASE + 1"] = A.rel_err(_mutated(c, d, torch.cat([c.P, c.P[:1]])), c.ref)
    # KEY_HI + 1 / KEY_LO - 1 on the clipped chunks: one more key, a row of the neighbour utterance
    d = g.desc.clone()
    clipped = (hi > lo) & (hi < g.W) & (kv0 + hi < g.kv_rows)
    assert clipped.any()
    d[clipped, 4] += 1
    seen["KEY_HI + 1"] = A.rel_err(_mutated(c, d), c.ref)
    d = g.desc.clone()
    clipped = (hi > lo) & (lo > 0)
    assert clipped.any()
    d[clipped, 3] -= 1
    seen["KEY_LO - 1"] = A.rel_err(_mutated(c, d), c.ref)
    # keys 0 and 1 of a whole window hold the keys 384 rows earlier (ring rows a wrapped staging did not refresh)
    stale = torch.full_like(c.ref, float("nan"))
    for i in torch.nonzero((lo == 0) & (hi == g.W) & (kv0 >= 384)).flatten().tolist():
        k0 = int(kv0[i])
        kv = c.kv.clone()
        kv[k0: k0 + 2] = c.kv[k0 - 384: k0 - 382]
        q0, nq = int(g.desc[i, 0]), int(g.desc[i, 1])
        stale[q0: q0 + nq] = attention_op_ref(c.q, kv[: g.kv_rows], c.P, c.u, c.v, g.desc[i: i + 1], A.H, c.dk)[q0: q0 + nq]
    touched = ~torch.isnan(stale[:, 0])
    assert touched.any()
    seen["stale ring rows"] = ((stale - c.ref)[touched].abs().max() / c.scale).item()
    for name, e in seen.items():
        print(f"{key} {dt}: {name}: {e:.3f} = {e / BAR[dt]:.0f} x the bar")
    for name, e in seen.items():
        assert e >= need, f"{name} moves the output by {e:.3e} < {MARGIN} x the bar ({need:.3e})"
