"""Kernel-level GPU parity of the row-wise kernels of the encoder step, one at a time on caller-owned buffers
(include/cfm_ops.h): cfm_op_layernorm (csrc/norm.hip: ln_kernel, ln2_kernel), cfm_op_conv_module
(csrc/conv_module.hip: the per-tap f32 kernel, the dot2 whole-chunk kernel at d = 128 / 256, the dot2 half-chunk
kernel at d = 512) and cfm_op_pos_table (csrc/misc.hip), against float64 references of the operators
(oracle/rowwise_op_ref.py) on the cases of tests/rowwise_op_cases.py (conv descriptors from the host planners).

Tolerance (the method of tests/test_gpu_ops_attention.py).  fp32, and every f32 output of a 16-bit kernel (the x
rows ln2_kernel writes, LN2_F32's out): 1e-4 of the output's max-abs, the project's fp32 golden bar.  16-bit
outputs: the rounding a correct kernel must incur, E_round(family, dtype), is computed on the CPU with no kernel
involved -- the maximum over the family's whole case list of max|ref(emulate=dtype) - ref| / max|ref|, where
emulate rounds exactly the points listed in oracle/rowwise_op_ref.py -- and the bar is 4 x E_round (accumulation
order, hardware rsqrt / exp / rcp).  tests/test_rowwise_op_ref_cpu.py recomputes the table and checks that the
bars still see the listed mutations with a 10 x margin.

    E_round, measured (CPU, float64)         worst case
    layernorm    bf16   3.785e-3             LN, d 256, M 7, two branches with both masks
    layernorm    fp16   4.714e-4             LN2 with w2, d 256, M 2, one branch
    conv_module  bf16   4.855e-3             padded full attention T' = 1, d 512
    conv_module  fp16   5.434e-4             padded chunked C = 16 T' = 70, d 128

pos_table.  Per element |out - ref| <= 4 ulp_f32(angle) + half an ulp of the output type at 1.0.  Both terms follow
from the f32 angle the reference itself uses (|p| * div_i, both factors f32): a kernel whose f32 div_i or product
is a few ulp off evaluates sin / cos at an angle that many ulp_f32(angle) away, and |d sin|, |d cos| <= |d angle|;
the result (|.| <= 1) is then rounded once to the output type.
"""
from types import SimpleNamespace

import pytest
import torch

import rowwise_op_cases as A

pytestmark = pytest.mark.gpu

E_ROUND = {"layernorm": {"bf16": 3.79e-3, "fp16": 4.72e-4}, "conv_module": {"bf16": 4.86e-3, "fp16": 5.44e-4}}
F32_BAR = 1e-4
BAR = {fam: {"fp32": F32_BAR, "bf16": 4 * e["bf16"], "fp16": 4 * e["fp16"]} for fam, e in E_ROUND.items()}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import _lib
    return _lib


def _code(L, dt):
    return {"fp32": L.DTYPE_F32, "bf16": L.DTYPE_BF16, "fp16": L.DTYPE_F16}[dt]


def _dev(t):
    return None if t is None else t.contiguous().to("cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------ LayerNorm
def _ln_launch(L, c, d_arg=None, alpha=A.ALPHA):
    """-> (status, x [M + GUARD, d] f32, out [M + GUARD, d]) on the CPU; the guard rows of x and all of out start NaN"""
    M, d = c.M, c.d
    x = torch.full((M + A.GUARD, d), float("nan"), dtype=torch.float32)
    x[:M] = c.x
    x = x.to("cuda")
    odt = torch.float32 if c.kind == L.LN2_F32 else A.TDT[c.dt]
    out = torch.full((M + A.GUARD, d), float("nan"), dtype=odt, device="cuda")
    y, y2, ym, ym2, rm = _dev(c.y), _dev(c.y2), _dev(c.ymask), _dev(c.ymask2), _dev(c.rowmask)
    w1, b1, w2, b2 = _dev(c.w1), _dev(c.b1), _dev(c.w2), _dev(c.b2)
    rc = L.cfm_op_layernorm(_code(L, c.dt), c.kind, x.data_ptr(), M, d_arg or d, L.ptr(y), alpha, L.ptr(ym), L.ptr(y2),
                            A.ALPHA2, L.ptr(ym2), int(c.f.defer), w1.data_ptr(), b1.data_ptr(), L.ptr(w2), L.ptr(b2),
                            A.EPS, out.data_ptr(), L.ptr(rm), _stream())
    torch.cuda.synchronize()
    return rc, x.cpu(), out.cpu()


def _ln_check(L, c):
    M = c.M
    rc, x, out = _ln_launch(L, c)
    L.check(rc)
    assert torch.isnan(x[M:]).all() and torch.isnan(out[M:].float()).all(), "rows past M were written"
    o = out[:M].double()
    assert torch.isfinite(o).all() and torch.isfinite(x[:M]).all(), "non-finite output"
    worst = 0.0
    if c.kind == L.LN:
        # defer / no branch: x bit-unchanged; otherwise exactly the f32 fmaf chain
        assert torch.equal(x[:M], c.x_ref), "x is not the f32 fmaf chain of the residual terms (bit-exact contract)"
        if c.rowmask is not None:
            assert (o[c.rowmask == 0] == 0).all(), "rows with rowmask 0 must be exactly 0"
    else:
        ex = A.rel_err(x[:M], c.x_ref)
        worst = ex / F32_BAR
        assert ex <= F32_BAR, f"x after {c.kindv}: {ex:.3e} > {F32_BAR:.1e}"
    bar = F32_BAR if c.kind == L.LN2_F32 else BAR["layernorm"][c.dt]
    err = A.rel_err(o, c.ref)
    assert err <= bar, f"{c.kindv} M={M} {c.form}: max|out - ref| / max|ref| = {err:.3e} > {bar:.2e}"
    if c.w2 is None:   # an exactly constant row comes out as b1 (a zero row under rowmask)
        const = c.rk == 3
        if c.rowmask is not None:
            const = const & (c.rowmask != 0)
        if const.any():
            eb = ((o[const] - c.b1.double()).abs().max() / c.scale).item()
            assert eb <= bar, f"constant rows: |out - b| / max|ref| = {eb:.3e} > {bar:.2e}"
    return max(worst, err / bar)


@pytest.mark.parametrize("kindv", list(A.LN_KINDS))
@pytest.mark.parametrize("dt", A.DTS)
@pytest.mark.parametrize("d", A.DS)
def test_layernorm_kernels(L, d, dt, kindv):
    """every (M, residual form) of the case list for this kernel variant, d and type"""
    worst = max(_ln_check(L, A.ln_case(kindv, d, M, form, dt)) for M, form in A.ln_case_list(kindv))
    print(f"layernorm-op {kindv} {dt} d={d}: worst err = {worst:.3f} of the bar "
          f"({BAR['layernorm'][dt]:.2e}; f32 outputs {F32_BAR:.1e})")


@pytest.mark.parametrize("dt", A.DTS)
@pytest.mark.parametrize("d", A.DS)
def test_layernorm_defer_pair_is_bit_identical(L, d, dt):
    """the claim of the encoder's residual scheme (csrc/model.hip, "bit-identical x"): LN deferring branch y, then LN
    with (y, y2), leaves x bit-identical to LN storing y, then LN with y2 alone -- and the second LN's out as well"""
    for M in (7, 1001):
        two = A.ln_case("ln", d, M, "yy_m1", dt)
        a = SimpleNamespace(**vars(two))
        a.y2 = a.ymask2 = None
        a.f = A.LN_FORMS["y_m_defer"]
        rc, xa, _ = _ln_launch(L, a)                       # defer: x unwritten
        L.check(rc)
        assert torch.equal(xa[:M], two.x)
        rc, x1, o1 = _ln_launch(L, two)                    # (y, y2) on the unwritten x
        L.check(rc)
        b = SimpleNamespace(**vars(a))
        b.f = A.LN_FORMS["y_m"]
        rc, xb, _ = _ln_launch(L, b)                       # store x + alpha y
        L.check(rc)
        s = SimpleNamespace(**vars(two))
        s.x, s.y, s.ymask, s.y2, s.ymask2 = xb[:M], two.y2, None, None, None
        s.f = A.LN_FORMS["y"]
        rc, x2, o2 = _ln_launch(L, s, alpha=A.ALPHA2)      # the second branch alone, at its own scale
        L.check(rc)
        assert torch.equal(x1[:M], x2[:M]), "x differs between the deferred and the stored sequence"
        assert torch.equal(o1[:M], o2[:M]), "out differs between the deferred and the stored sequence"
        assert torch.equal(x1[:M], two.x_ref)


@pytest.mark.parametrize("kindv", list(A.LN_KINDS))
@pytest.mark.parametrize("dt", A.DTS)
def test_layernorm_refuses(L, dt, kindv):
    """a d the kernels do not take: nothing runs, x and out stay untouched, the message names the kernel"""
    c = A.ln_case(kindv, 128, 7, "yy_m12", dt)
    for bad_d in (64, 384, 1024):
        rc, x, out = _ln_launch(L, c, d_arg=bad_d)
        assert rc == L.CFM_ERR_ASSERT
        name = {"ln": "layernorm", "ln2_w2": "layernorm2", "ln2": "layernorm2", "ln2_f32": "layernorm2_f32"}[kindv]
        with pytest.raises(AssertionError, match=f"the {name} kernel"):
            L.check(rc)
        assert torch.equal(x[: c.M], c.x) and torch.isnan(out.float()).all(), "a refused call wrote to x / out"


# ------------------------------------------------------------------------------------------ conv module
def _conv_launch(L, c, d_arg=None):
    g = c.g
    glu, desc = c.glu.to("cuda"), g.desc.contiguous().to("cuda")
    out = torch.full((g.rows + A.GUARD, c.d), float("nan"), dtype=A.TDT[c.dt], device="cuda")
    w, b, lw, lb = _dev(c.wdw), _dev(c.bdw), _dev(c.lnw), _dev(c.lnb)
    rc = L.cfm_op_conv_module(_code(L, c.dt), glu.data_ptr(), desc.data_ptr(), desc.shape[0], d_arg or c.d, w.data_ptr(),
                              b.data_ptr(), lw.data_ptr(), lb.data_ptr(), A.EPS, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu()


@pytest.mark.parametrize("dt", A.DTS)
@pytest.mark.parametrize("d", A.DS)
@pytest.mark.parametrize("key", A.CONV_KEYS, ids=lambda k: "-".join(map(str, k)).replace(" ", ""))
def test_conv_module_kernels(L, key, d, dt):
    """GLU rows outside every descriptor's real range are NaN: a kernel that reads one masked column fails"""
    c = A.conv_case(key, d, dt)
    rc, out = _conv_launch(L, c)
    L.check(rc)
    o = out[: c.g.rows].float()
    assert torch.isnan(out[c.g.rows:].float()).all(), "guard rows after the last output row were written"
    covered = ~torch.isnan(c.ref[:, 0])
    assert torch.isfinite(o[covered]).all(), "non-finite output (a masked column was read?)"
    assert torch.isnan(o[~covered]).all(), "a row no descriptor covers was written"
    err, bar = A.rel_err(o, c.ref), BAR["conv_module"][dt]
    print(f"conv-module-op {key} {dt} d={d}: err {err:.3e} = {err / bar:.3f} of the bar {bar:.2e}")
    assert err <= bar, f"max|out - ref| / max|ref| = {err:.3e} > {bar:.2e}"


@pytest.mark.parametrize("dt", A.DTS)
def test_conv_module_refuses(L, dt):
    c = A.conv_case(("stream", 20, 16, 8), 128, dt)
    for bad_d in (64, 384):
        rc, out = _conv_launch(L, c, d_arg=bad_d)
        assert rc == L.CFM_ERR_ASSERT
        with pytest.raises(AssertionError, match="conv_dw_ln_silu"):
            L.check(rc)
        assert torch.isnan(out.float()).all(), "a refused call wrote to out"


# ------------------------------------------------------------------------------------------ pos_table
@pytest.mark.parametrize("dt", A.DTS)
@pytest.mark.parametrize("d", A.POS_D)
@pytest.mark.parametrize("name", A.POS_KEYS)
def test_pos_table_kernel(L, name, d, dt):
    c = A.pos_case(name, d)
    out = torch.full((c.p_rows + A.GUARD, d), float("nan"), dtype=A.TDT[dt], device="cuda")
    L.check(L.cfm_op_pos_table(_code(L, dt), d, c.p_rows, c.anchor, out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[c.p_rows:].float()).all(), "guard rows were written"
    o = out[: c.p_rows].double()
    assert torch.isfinite(o).all()
    bar = 4 * c.angle_ulp + torch.finfo(A.TDT[dt]).eps / 2
    ratio = ((o - c.ref).abs() / bar).max().item()
    print(f"pos-table-op {name} {dt} d={d}: worst |out - ref| = {ratio:.3f} of the per-element bar")
    assert ratio <= 1.0


def test_pos_table_refuses(L):
    out = torch.full((8, 128), float("nan"), dtype=torch.float32, device="cuda")
    rc = L.cfm_op_pos_table(L.DTYPE_F32, 127, 8, 3, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == L.CFM_ERR_ASSERT
    with pytest.raises(AssertionError, match="pos_table"):
        L.check(rc)
    assert torch.isnan(out).all()
