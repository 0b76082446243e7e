"""Kernel-level GPU parity of the five attention kernels (cfm_op_attention, include/cfm_ops.h): the generic
chunk_attention_kernel<T, DK>, the dk = 64 ring kernel (bf16 / f16), the head_dim 128 kernel (with
vt_transpose), and the dense full-attention kernel, each selected explicitly -- a shape the selected kernel
does not take is an error, never another kernel -- against a float64 reference of the operator
(oracle/attention_op_ref.py) on descriptors from the host planners (tests/attention_op_cases.py).

Tolerance.  fp32: 1e-4 of the output's max-abs (the project's fp32 golden bar).  16-bit types: the rounding a
correct kernel must incur, E_round(dtype), is computed on the CPU with no kernel involved -- the maximum over
every case below of max|ref(emulate=dtype) - ref| / max|ref|, where emulate rounds q+u, q+v, the un-normalised
probabilities and the output to the type -- and the bar is 4 x E_round: the factor covers MFMA accumulation
order, the hardware exp and the ring / dense kernels' further rounding point (the skewed band through a 16-bit
scratch).  tests/test_attention_op_ref_cpu.py recomputes the table and checks that the bars still see one-off
errors of the descriptor fields and stale ring rows with a 10 x margin.

    E_round, measured (CPU, float64)      worst case
    bf16   6.136e-3                        masked C=64 L=128 R=128, p_ld = 3 d, dk 64
    fp16   7.733e-4                        masked C=64 L=126 R=128, dk 64
"""
import pytest
import torch

import attention_op_cases as A

pytestmark = pytest.mark.gpu

E_ROUND = {"bf16": 6.14e-3, "fp16": 7.74e-4}
BAR = {"fp32": 1e-4, "bf16": 4 * E_ROUND["bf16"], "fp16": 4 * E_ROUND["fp16"]}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import _lib
    return _lib


def _launch(L, c, kernel, min_chunks=2):
    """-> (cfm_status, out [q_rows + GUARD, d] on the CPU); out starts as NaN"""
    g, dev = c.g, "cuda"
    q, kv, ptab, u, v = (t.to(dev) for t in (c.q, c.kv, c.ptab, c.u, c.v))
    desc = g.desc.contiguous().to(dev)
    out = torch.full((g.q_rows + A.GUARD, c.d), float("nan"), dtype=A.TDT[c.dt], device=dev)
    p_ptr = ptab.data_ptr() + (c.d * ptab.element_size() if c.p_ld != c.d else 0)
    vt, vt_ld = None, 0
    if kernel == L.ATTN_A128:   # NaN: a read of a column the transpose did not write would reach the output
        vt_ld = (g.kv_rows + 7) // 8 * 8
        vt = torch.full((A.H * c.dk, vt_ld), float("nan"), dtype=torch.bfloat16, device=dev)
    code = {"fp32": L.DTYPE_F32, "bf16": L.DTYPE_BF16, "fp16": L.DTYPE_F16}[c.dt]
    rc = L.cfm_op_attention(code, kernel, q.data_ptr(), kv.data_ptr(), g.kv_rows, p_ptr, g.p_rows, c.p_ld, u.data_ptr(),
                            v.data_ptr(), desc.data_ptr(), desc.shape[0], A.H, c.dk, g.C, g.W, out.data_ptr(), min_chunks,
                            L.ptr(vt), vt_ld, g.nutt, g.nd, g.t_keys, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu()


def _check(L, c, kernel, min_chunks=2, what=""):
    g = c.g
    if c.n_scores >= 100:   # (a handful of scores, as at T' = 1, has no meaningful spread)
        assert min(c.sharp) >= 1.0, f"flat inputs: std of the content / rel-pos term {c.sharp}"
    rc, out = _launch(L, c, kernel, min_chunks)
    L.check(rc)
    o = out[: g.q_rows].float()
    assert torch.isnan(out[g.q_rows:].float()).all(), "guard rows after the last query row were written"
    covered = ~torch.isnan(c.ref[:, 0])
    assert torch.isfinite(o[covered]).all(), "non-finite output"
    assert torch.isnan(o[~covered]).all(), "a row no descriptor covers was written"
    for q0, nq, _, lo, hi, _, qvalid, _ in g.desc.tolist():
        z = o[q0: q0 + nq] if hi <= lo else o[q0 + max(qvalid, 0): q0 + nq]
        assert (z == 0).all(), "rows >= Q_VALID / rows without keys must be exactly 0"
    err, bar = A.rel_err(o, c.ref), BAR[c.dt]
    print(f"attention-op {what or kernel} {c.dt} dk={c.dk}: err {err:.3e} = {err / bar:.3f} of the bar {bar:.2e}")
    assert err <= bar, f"max|out - ref| / max|ref| = {err:.3e} > {bar:.2e}"


def _refused(L, c, kernel, name):
    rc, out = _launch(L, c, kernel)
    assert rc == L.CFM_ERR_ASSERT, f"status {rc}: the {name} kernel must refuse this shape, not run or fall back"
    with pytest.raises(AssertionError, match=name):
        L.check(rc)
    assert torch.isnan(out.float()).all(), "a refused call wrote to out"


# ------------------------------------------------------------------------------------------ generic
@pytest.mark.parametrize("dk", [64, 128])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("key", A.GENERIC_KEYS, ids=lambda k: "-".join(map(str, k)))
def test_generic_kernel(L, key, dt, dk):
    _check(L, A.case(key, dt, dk), L.ATTN_GENERIC, what="generic")


@pytest.mark.parametrize("dk", [64, 128])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_generic_kernel_p_stride(L, dt, dk):
    """p_ld = 3 d with the rows of the middle layer column (the other columns hold 8 x larger values)"""
    _check(L, A.case(A.PCOL_KEY, dt, dk, True), L.ATTN_GENERIC, what="generic p_ld")


# ------------------------------------------------------------------------------------------ ring
@pytest.mark.parametrize("runs", ["min2", "one_block"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("C,L_,R", A.RING_SHAPES)
def test_ring_kernel(L, C, L_, R, dt, runs):
    """min2: many short runs (2 and 3 chunks, an idle second half-block at odd lengths); one_block: one block
    per head sweeps all 23 chunks, so the 384-row ring wraps (at C = 64 three times)"""
    c = A.case(("masked", C, L_, R, "std"), dt, 64)
    assert c.g.n_chunks == 23
    _check(L, c, L.ATTN_RING, 2 if runs == "min2" else c.g.n_chunks, what=f"ring C={C} L={L_} R={R} {runs}")


@pytest.mark.parametrize("batch", ["n1", "n2", "n3"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("C,L_,R", A.RING_SMALL)
def test_ring_kernel_small_batches(L, C, L_, R, dt, batch):
    c = A.case(("masked", C, L_, R, batch), dt, 64)
    assert c.g.n_chunks == int(batch[1])
    _check(L, c, L.ATTN_RING, what=f"ring C={C} L={L_} R={R} {batch}")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_ring_kernel_p_stride(L, dt):
    _check(L, A.case(("masked", 64, 128, 128, "std"), dt, 64, True), L.ATTN_RING, what="ring p_ld")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("C,L_,R", A.RING_REFUSED)
def test_ring_kernel_refuses(L, C, L_, R, dt):
    _refused(L, A.case(("masked", C, L_, R, "std"), dt, 64), L.ATTN_RING, "ring")


# ------------------------------------------------------------------------------------------ head_dim 128
@pytest.mark.parametrize("C,L_,R", A.A128_SHAPES)
def test_a128_kernel(L, C, L_, R):
    _check(L, A.case(("masked", C, L_, R, "std"), "bf16", 128), L.ATTN_A128, what=f"a128 W={L_ + C + R}")


@pytest.mark.parametrize("batch", ["n1", "n2", "n3"])
def test_a128_kernel_small_batches(L, batch):
    _check(L, A.case(("masked", 64, 128, 128, batch), "bf16", 128), L.ATTN_A128, what=f"a128 {batch}")


def test_a128_kernel_refuses(L):
    for C, L_, R in A.A128_REFUSED:
        _refused(L, A.case(("masked", C, L_, R, "std"), "bf16", 128), L.ATTN_A128, "a128")


# ------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize("tp", A.DENSE_T)
def test_dense_kernel(L, tp):
    """full attention over T' frames: three utterances of T', 2T'/3 and T'/3 frames (KEY_HI per utterance)"""
    _check(L, A.case(("dense", tp), "bf16", 64), L.ATTN_DENSE, what=f"dense T'={tp}")


def test_dense_kernel_refuses(L):
    _refused(L, A.case(("dense", A.DENSE_REFUSED_T), "bf16", 64), L.ATTN_DENSE, "dense")
