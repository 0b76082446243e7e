"""Kernel-level parity of the attention decoder's two segment attention kernels (cfm_op_seg_attention,
include/cfm_ops.h; csrc/aed.hip): the generic kernel (any type, head dim 16 .. 128) and the MFMA kernel (bf16 / f16,
head dim 64 / 128), each selected explicitly -- a shape the selected kernel does not take is an error, never the
other kernel -- against a float64 reference of the operator computed here (tests/seg_attention_cases.py).

One call runs the whole grid: NQ in {1, 16, 17, 65} x NK in {0, 1, 63, 64, 65, 129} x {all keys, causal}, 48 segments
at unaligned rows, eight query segments sharing each key range, NaN in every row no descriptor covers.

Tolerance, as in test_gpu_ops_attention.py.  fp32: 1e-4 of the output's max-abs.  16-bit types: the rounding a correct
kernel must incur, E_round(dtype), is computed on the CPU with no kernel involved -- max|ref(emulate=dtype) - ref| /
max|ref|, where emulate rounds q, k, v, the un-normalised probabilities and the output to the type
(seg_attention_cases.seg_attention_ref) -- and the bar is 4 x E_round (MFMA accumulation order, the hardware exp,
the online softmax's rescaling).  test_e_round_table recomputes the table on the CPU.

    E_round, measured (CPU, float64)      dk 16       dk 64       dk 128      worst case
    bf16                                  2.283e-3    2.411e-3    1.600e-3    dk 64
    fp16                                  2.886e-4    3.348e-4    2.391e-4    dk 64

test_bars_see_one_off_descriptor_errors (CPU): the exact operator with one descriptor field of one segment off by one
(CAUSAL: flipped), the smallest error over the segments where the change matters.  Every field exceeds the fp32 and
fp16 bars in every segment (smallest: NK + 1 at dk 128, 1.39e-3 against the fp16 bar 1.34e-3 / the fp32 bar 1e-4);
Q0, NQ and CAUSAL exceed the bf16 bar too (>= 8.1e-2).  One key more or less among 63 or more (K0, NK: 1.4e-3 ..
1.8e-2) is of the size of bf16 rounding itself (bar 9.6e-3): the bf16 runs cannot see it; the same kernel templates
run in fp16, where they can, and test_mfma_matches_generic compares the two kernels on the same bf16 inputs.
"""
import pytest
import torch

import seg_attention_cases as S

E_ROUND = {"bf16": 2.42e-3, "fp16": 3.35e-4}
BAR = {"fp32": 1e-4, "bf16": 4 * E_ROUND["bf16"], "fp16": 4 * E_ROUND["fp16"]}
GUARD = 8


# ------------------------------------------------------------------------------------------ CPU
def test_e_round_table():
    for dt in ("bf16", "fp16"):
        worst = max(S.e_round(dt, dk) for dk in (16, 64, 128))
        assert 0.9 * E_ROUND[dt] <= worst <= E_ROUND[dt], f"E_round({dt}) = {worst:.4e}"


def test_bars_see_one_off_descriptor_errors():
    for dk in (16, 64, 128):
        for f, name in enumerate(S.FIELDS):
            for delta in ((1,) if f == 4 else (-1, 1)):
                for dt in ("fp32", "fp16"):
                    e = S.one_off_error(dt, dk, f, delta)
                    assert e > BAR[dt], f"{dt} dk {dk}: {name} {delta:+d} gives {e:.2e} <= bar {BAR[dt]:.2e}"
                if name in ("Q0", "NQ", "CAUSAL"):
                    e = S.one_off_error("bf16", dk, f, delta)
                    assert e > 5 * BAR["bf16"], f"bf16 dk {dk}: {name} {delta:+d} gives {e:.2e}"


def test_reference_properties():
    c = S.case("fp32", 16)
    g = c.g
    assert torch.isnan(c.ref[~c.q_covered]).all() and torch.isfinite(c.ref[c.q_covered]).all()
    for q0, nq, k0, nk, causal, *_ in g.desc.tolist():
        if nk == 0:
            assert (c.ref[q0: q0 + nq] == 0).all()
        if causal and nk > 0:   # row 0 sees key 0 only: the output is that key's value row
            assert torch.allclose(c.ref[q0], c.kv[k0, c.d:].double(), atol=1e-12)
    assert {(int(r[1]), int(r[3]), int(r[4])) for r in g.desc} == {(a, b, z) for a in S.NQS for b in S.NKS for z in (0, 1)}
    assert any(int(r[0]) % 16 for r in g.desc) and any(int(r[2]) % 16 for r in g.desc)


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import _lib
    return _lib


def _launch(L, c, kernel, desc=None):
    """-> (cfm_status, out [q_rows + GUARD, d] on the CPU, status word); out starts as NaN"""
    g, dev = c.g, "cuda"
    desc = (g.desc if desc is None else desc).contiguous().to(dev)
    q, kv = c.q.to(dev), c.kv.to(dev)
    out = torch.full((g.q_rows + GUARD, c.d), float("nan"), dtype=S.TDT[c.dt], device=dev)
    scratch = torch.full((desc.shape[0] + 2,), -1, dtype=torch.int32, device=dev)
    code = {"fp32": L.DTYPE_F32, "bf16": L.DTYPE_BF16, "fp16": L.DTYPE_F16}[c.dt]
    rc = L.cfm_op_seg_attention(code, kernel, q.data_ptr(), g.q_rows, kv.data_ptr(), g.k_rows, desc.data_ptr(),
                                desc.shape[0], S.H, c.dk, out.data_ptr(), scratch.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu(), int(scratch[0].item())


def _check(L, c, kernel, what):
    g = c.g
    rc, out, status = _launch(L, c, kernel)
    L.check(rc)
    assert status == 0
    o = out[: g.q_rows].float()
    assert torch.isnan(out[g.q_rows:].float()).all(), "guard rows after the last query row were written"
    assert torch.isfinite(o[c.q_covered]).all(), "non-finite output (a NaN row was read)"
    assert torch.isnan(o[~c.q_covered]).all(), "a row no descriptor covers was written"
    for q0, nq, k0, nk, causal, *_ in g.desc.tolist():
        if nk == 0:
            assert (o[q0: q0 + nq] == 0).all(), "rows without keys must be exactly 0"
    err, bar = S.rel_err(o, c.ref), BAR[c.dt]
    print(f"seg-attention {what} {c.dt} dk={c.dk}: err {err:.3e} = {err / bar:.3f} of the bar {bar:.2e}")
    assert err <= bar, f"max|out - ref| / max|ref| = {err:.3e} > {bar:.2e}"
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("dk", [16, 64, 128])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_generic_kernel(L, dt, dk):
    _check(L, S.case(dt, dk), L.SEG_ATTN_GENERIC, "generic")


@pytest.mark.gpu
@pytest.mark.parametrize("dk", [64, 128])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_mfma_kernel(L, dt, dk):
    _check(L, S.case(dt, dk), L.SEG_ATTN_MFMA, "mfma")


@pytest.mark.gpu
@pytest.mark.parametrize("dk", [64, 128])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_mfma_matches_generic(L, dt, dk):
    """The two kernels on the same 16-bit inputs: both round the output to the type, the MFMA kernel also the
    probabilities, so they differ by at most the rounding bar itself."""
    c = S.case(dt, dk)
    a = _check(L, c, L.SEG_ATTN_GENERIC, "generic")
    b = _check(L, c, L.SEG_ATTN_MFMA, "mfma")
    m = c.q_covered
    scale = c.ref[m].abs().max().item()
    diff = (a[m].double() - b[m].double()).abs().max().item() / scale
    print(f"seg-attention mfma vs generic {dt} dk={dk}: {diff:.3e}")
    assert diff <= BAR[dt]


@pytest.mark.gpu
def test_kernels_refuse_what_they_do_not_take(L):
    for c, kernel, name in ((S.case("fp32", 64), L.SEG_ATTN_MFMA, "mfma"), (S.case("bf16", 16), L.SEG_ATTN_MFMA, "mfma")):
        rc, out, _ = _launch(L, c, kernel)
        assert rc == L.CFM_ERR_ASSERT, f"status {rc}: the {name} kernel must refuse this shape, not run or fall back"
        with pytest.raises(AssertionError, match=name):
            L.check(rc)
        assert torch.isnan(out.float()).all(), "a refused call wrote to out"


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_bad_descriptor_is_skipped(L, kernel):
    """A range outside its array sets the status word; that segment is skipped, the others are as without it."""
    c = S.case("bf16", 64)
    g = c.g
    kid = L.SEG_ATTN_GENERIC if kernel == "generic" else L.SEG_ATTN_MFMA
    for field, value in ((3, g.k_rows), (0, g.q_rows - 3), (2, -1), (1, -5)):
        desc = g.desc.clone()
        s = 34                       # NQ 17, NK 63, causal
        desc[s, field] = value
        rc, out, status = _launch(L, c, kid, desc)
        L.check(rc)
        assert status == 1
        q0, nq = int(g.desc[s, 0]), int(g.desc[s, 1])
        o = out[: g.q_rows].float()
        assert torch.isnan(o[q0: q0 + nq]).all(), "the bad segment's rows were written"
        keep = c.q_covered.clone()
        keep[q0: q0 + nq] = False
        ref = c.ref.clone()
        ref[~keep] = float("nan")
        assert torch.isnan(o[~keep]).all() and S.rel_err(o, ref) <= BAR["bf16"]
