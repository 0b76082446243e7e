"""Kernel-level GPU parity of the front-end kernels, one at a time on a model's own weights (include/cfm_ops.h):
cfm_op_frontend_conv0_dw -- the three conv0 + ReLU + dw1 kernels of csrc/frontend.hip, each selected explicitly (VALU
f32 arithmetic; position-stationary MFMA; channel-stationary MFMA at 1, 2 and 5 chunks per workgroup) -- and
cfm_op_frontend_dw2 -- fe_dw2_kernel, and the fused pw1 + ReLU + dw2 weight-stationary GEMM (csrc/gemm_wst_impl.h,
EPI_DW2) -- against float64 references of the operators (oracle/frontend_op_ref.py) on the cases of
tests/frontend_op_cases.py.  A (dtype, d) a kernel does not take is an error, never another kernel.

Source feature rows at or past a window's NVALID are NaN and every output buffer starts as NaN with a guard: a
kernel that reads a padding row from memory, or writes past its window, fails.

Tolerance (the method of tests/test_gpu_ops_attention.py).  fp32: 1e-4 of the output's max-abs.  16-bit: the rounding
a correct kernel of that type must incur, E_round(kernel family, dtype), is computed on the CPU with no kernel
involved -- the maximum over the family's whole case list (every d) of max|ref(emulate=dtype) - ref| / max|ref|,
with one emulation per kernel (the rounding points are listed in oracle/frontend_op_ref.py) -- and the bar is
4 x E_round (accumulation order of the MFMA / dot2 sums).  tests/test_frontend_op_ref_cpu.py recomputes the table
and checks that the bars still see the listed mutations with a 10 x margin.

    E_round, measured (CPU, float64)             worst case
    conv0_dw VALU       bf16   3.657e-3          W 119, CMVN, packed, d 256
    conv0_dw VALU       fp16   4.403e-4          W 63, CMVN, packed, d 256
    conv0_dw MFMA_POS   bf16   4.899e-3          W 103, CMVN, packed, d 512
    conv0_dw MFMA_POS   fp16   5.980e-4          W 101, no CMVN, packed, d 128
    conv0_dw MFMA_CH    bf16   7.462e-3          W 102, no CMVN, table, d 512
    conv0_dw MFMA_CH    fp16   9.849e-4          W 63, no CMVN, packed, d 128
    dw2 UNFUSED         bf16   4.819e-3          T2 7, 1 window, d 256
    dw2 UNFUSED         fp16   6.503e-4          T2 15, 2 windows, d 512
    dw2 FUSED           bf16   5.396e-3          T2 3, 1 window, d 512
    dw2 FUSED           fp16   7.242e-4          T2 29, 1 window, d 512
"""
import pytest
import torch

import frontend_op_cases as A

pytestmark = pytest.mark.gpu

E_ROUND = {"valu": {"bf16": 3.66e-3, "fp16": 4.41e-4}, "pos": {"bf16": 4.90e-3, "fp16": 5.98e-4},
           "ch": {"bf16": 7.47e-3, "fp16": 9.85e-4}, "dw2": {"bf16": 4.82e-3, "fp16": 6.51e-4},
           "dw2_fused": {"bf16": 5.40e-3, "fp16": 7.25e-4}}
BAR = {fam: {"fp32": 1e-4, "bf16": 4 * e["bf16"], "fp16": 4 * e["fp16"]} for fam, e in E_ROUND.items()}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def models(L):
    """(d, dtype) -> encoder, built on first use and kept for the module"""
    from chunkformer_amd.encoder import ChunkFormerEncoder
    cache = {}

    def get(d, dt):
        if (d, dt) not in cache:
            cache[(d, dt)] = ChunkFormerEncoder(A.CFG[d], A.state_dict(d), device="cuda:0", dtype=dt)
        return cache[(d, dt)]
    return get


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_out(n, dt):
    return torch.full((n + A.GUARD,), float("nan"), dtype=A.TDT[dt], device="cuda")


# ------------------------------------------------------------------------------------------ conv0 + ReLU + dw1
def _conv_launch(L, enc, c, kname, dt):
    kern, k = A.KERNELS[kname]
    sel = {"valu": L.FE_VALU, "pos": L.FE_MFMA_POS, "ch": L.FE_MFMA_CH}[kern]
    n = A.NWIN * c.T2 * 19 * c.d
    out = _nan_out(n, dt)
    meta = c.meta.to("cuda")
    feats = tab = None
    if c.tab:
        utts = [u.to("cuda") for u in c.utts]
        tab = torch.tensor([u.data_ptr() for u in utts], dtype=torch.int64, device="cuda")
    else:
        feats = c.feats.to("cuda")
    rc = L.cfm_op_frontend_conv0_dw(enc._h, sel, k, int(c.cmvn), L.ptr(feats), L.ptr(tab), c.step, meta.data_ptr(), A.NWIN,
                                    c.W, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    out = out.cpu()
    return rc, out[:n].view(A.NWIN, c.T2, 19, c.d), out[n:]


def _conv_cases(dts):
    return [pytest.param(key, d, dt, id=f"W{key[0]}-{'cmvn' if key[1] else 'raw'}-{'tab' if key[2] else 'packed'}"
                                        f"-x{key[3]:g}-d{d}-{dt}") for key in A.CONV_KEYS for d in A.DS for dt in dts]


def _conv_check(L, models, key, d, dt, kname):
    c = A.conv_case(key, d)
    rc, out, guard = _conv_launch(L, models(d, dt), c, kname, dt)
    L.check(rc)
    assert torch.isnan(guard.float()).all(), "the guard after the last window was written"
    assert torch.isfinite(out.float()).all(), "non-finite output (a source row at or past NVALID was read?)"
    err, bar = A.rel_err(out, c.ref), BAR[A.KERNELS[kname][0]][dt]
    print(f"frontend-conv0-dw-op {kname} {dt} d={d} {key}: err {err:.3e} = {err / bar:.3f} of the bar {bar:.2e}")
    assert err <= bar, f"max|out - ref| / max|ref| = {err:.3e} > {bar:.2e}"


@pytest.mark.parametrize("key,d,dt", _conv_cases(A.DTS))
def test_conv0_dw_valu_kernel(L, models, key, d, dt):
    _conv_check(L, models, key, d, dt, "valu")


@pytest.mark.parametrize("key,d,dt", _conv_cases(["bf16", "fp16"]))
def test_conv0_dw_mfma_pos_kernel(L, models, key, d, dt):
    _conv_check(L, models, key, d, dt, "pos")


@pytest.mark.parametrize("kname", ["ch_k0", "ch_k1", "ch_k4"])
@pytest.mark.parametrize("key,d,dt", _conv_cases(["bf16", "fp16"]))
def test_conv0_dw_mfma_ch_kernel(L, models, key, d, dt, kname):
    _conv_check(L, models, key, d, dt, kname)


@pytest.mark.parametrize("kname", ["pos", "ch_k0"])
@pytest.mark.parametrize("d", A.DS)
def test_conv0_dw_refuses(L, models, d, kname):
    """the MFMA kernels on an fp32 model: nothing runs (in particular not the VALU kernel), out stays untouched"""
    c = A.conv_case(A.CONV_KEYS[4], d)
    rc, out, guard = _conv_launch(L, models(d, "fp32"), c, kname, "fp32")
    assert rc == L.CFM_ERR_ASSERT
    with pytest.raises(AssertionError, match="fe_conv0_dw_mfma2" if kname == "ch_k0" else "fe_conv0_dw_mfma "):
        L.check(rc)
    assert torch.isnan(out).all() and torch.isnan(guard).all(), "a refused call wrote to out"


# ------------------------------------------------------------------------------------------ dw2
def _dw2_launch(L, enc, c, mode, seg, src):
    n = c.nwin * c.T3 * 9 * c.d
    out = _nan_out(n, c.dt)
    x = src.contiguous().to("cuda")
    rc = L.cfm_op_frontend_dw2(enc._h, mode, x.data_ptr(), c.nwin, c.T2, seg, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    out = out.cpu()
    return rc, out[:n].view(c.nwin, c.T3, 9, c.d), out[n:]


def _dw2_cases():
    return [pytest.param(key, d, dt, id=f"T2_{key[0]}-n{key[1]}-d{d}-{dt}") for key in A.DW2_KEYS for d in A.DS for dt in A.DTS]


@pytest.mark.parametrize("key,d,dt", _dw2_cases())
def test_dw2_unfused_kernel(L, models, key, d, dt):
    """fe_dw2_kernel at 1, 4 and T3 + 3 row segments per walk"""
    c = A.dw2_case(key, d, dt)
    for seg in A.dw2_segs(c.T2):
        rc, out, guard = _dw2_launch(L, models(d, dt), c, L.FE_DW2_UNFUSED, seg, c.z)
        L.check(rc)
        assert torch.isnan(guard.float()).all() and torch.isfinite(out.float()).all()
        err, bar = A.rel_err(out, c.ref), BAR["dw2"][dt]
        print(f"frontend-dw2-op unfused seg={seg} {dt} d={d} {key}: err {err:.3e} = {err / bar:.3f} of the bar {bar:.2e}")
        assert err <= bar, f"seg {seg}: max|out - ref| / max|ref| = {err:.3e} > {bar:.2e}"


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("key", A.DW2_KEYS, ids=lambda k: f"T2_{k[0]}-n{k[1]}")
def test_dw2_fused_kernel(L, models, key, dt):
    """pw1 + ReLU + dw2 in one kernel (d = 512) against fp64, and bit-identical to the pw1 GEMM (cfm_op_gemm on the
    weight-stationary kernel at any M, as the model's "gemm_wst" 2) followed by fe_dw2_kernel"""
    d = 512
    c, w, enc = A.dw2_case(key, d, dt), A.weights(d), models(d, dt)
    rc, out, guard = _dw2_launch(L, enc, c, L.FE_DW2_FUSED, 0, c.a)
    L.check(rc)
    assert torch.isnan(guard.float()).all() and torch.isfinite(out.float()).all()
    err, bar = A.rel_err(out, c.ref_fused), BAR["dw2_fused"][dt]
    print(f"frontend-dw2-op fused {dt} d={d} {key}: err {err:.3e} = {err / bar:.3f} of the bar {bar:.2e}")
    assert err <= bar, f"max|out - ref| / max|ref| = {err:.3e} > {bar:.2e}"
    # the unfused pair on the same inputs
    M = c.nwin * c.T2 * 19
    a, pw1, b = c.a.contiguous().to("cuda"), c.pw1.contiguous().to("cuda"), w.b_pw1.contiguous().to("cuda")
    z = torch.full((M + 4, d), float("nan"), dtype=A.TDT[dt], device="cuda")
    code = {"bf16": L.DTYPE_BF16, "fp16": L.DTYPE_F16}[dt]
    L.check(L.cfm_op_gemm(code, 0, 1, a.data_ptr(), d, pw1.data_ptr(), d, M, d, d, b.data_ptr(), 1.0, z.data_ptr(), d, 0, 0,
                          0, 0, 0, 0, 2 << 18, _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(z[M:].float()).all() and torch.isfinite(z[:M].float()).all()
    rc, out2, _ = _dw2_launch(L, enc, c, L.FE_DW2_UNFUSED, 4, z[:M].view(c.nwin, c.T2, 19, d))
    L.check(rc)
    bad = (out != out2).flatten(0, 2).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, (f"fused != pw1 GEMM + fe_dw2_kernel in {bad.numel()} rows, first {bad[:8].tolist()}, "
                              f"max abs {(out.float() - out2.float()).abs().max().item():.3e}")


@pytest.mark.parametrize("d,dt", [(128, "bf16"), (256, "fp16"), (128, "fp32"), (256, "fp32"), (512, "fp32")])
def test_dw2_fused_refuses(L, models, d, dt):
    """where gemm_bf16_wst declines (d != 512, an fp32 model) FUSED launches nothing and says so"""
    c = A.dw2_case((7, 2), d, dt)
    rc, out, guard = _dw2_launch(L, models(d, dt), c, L.FE_DW2_FUSED, 0, c.a)
    assert rc == L.CFM_ERR_ASSERT
    with pytest.raises(AssertionError, match="fused pw1 \\+ dw2 kernel"):
        L.check(rc)
    assert torch.isnan(out.float()).all() and torch.isnan(guard.float()).all(), "a refused call wrote to out"
