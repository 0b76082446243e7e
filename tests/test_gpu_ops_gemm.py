"""Kernel-level GPU parity of the projection GEMM, one kernel at a time (cfm_op_gemm, include/cfm_ops.h): the
128 x 128 kernel (csrc/gemm.hip), the 256 x 256 persistent LDS-DMA kernel (csrc/gemm_bf16.hip) and the K = 512
weight-stationary kernel (csrc/gemm_wst_impl.h) against the float64 reference of the operator
(oracle/gemm_op_ref.py) on the cases of tests/gemm_op_cases.py: tile, row-tail and column-tail edges, every epilogue,
the persistent walk with more tiles than CUs at nk = K / 64 in {1, 2, 3, 5}, QKV at head dim 64 and 128, the
weight-stationary kernel below one tile per CU, the default routing edges, row pitches larger than the width.

Every case names its kernel and the route query must agree before the launch, so a moved threshold fails here instead
of silently moving a case to another kernel.  The pad columns of A and W and the rows after them are NaN, every
output starts as NaN: a kernel that reads a pad, or writes outside its rows and columns, fails.

Pass criterion: |out - ref| <= bar on EVERY element, the bar per element and derived without the kernels
(accumulation K 2^-23 S, the epilogue's derivative, exp2 / rcp, one output rounding: the derivation is the docstring
of oracle/gemm_op_ref.py; tests/test_gemm_op_ref_cpu.py shows that a correct f32 kernel stays inside it in any
summation order and that it sees the listed mutations with a 10 x margin).  One-hot cases must be bit-exact.

Worst err / bar measured on an MI355X (256 CUs) against the fp64 reference, per kernel, type and epilogue (store0-3:
STORE with act 0-3; glu0 / glu3: GLU with act 0 / 3; 243 tests, 5.4 s).  With a 16-bit output the bar is dominated by
the one rounding no kernel can avoid (half an ulp of the output), so a correctly rounded result sits just below 1;
the f32 outputs show the accumulation term alone, 0.2-6 % of its bound:

    kernel  type     store0    store1    store2    store3 store_f32     resid       qkv      glu0      glu3
       128   f32      0.045     0.007     0.051     0.012     0.054     0.054     0.029     0.002     0.030
       128  bf16      0.985     0.910     0.974     0.957     0.010     0.020     0.977     0.886     0.989
       128   f16      0.935     0.849     0.964     0.849     0.011     0.015     0.924     0.514     0.941
       256  bf16      0.987     0.989     0.992     0.970     0.008     0.022     0.987     0.971     0.974
       256   f16      0.977     0.869     0.914     0.784     0.020     0.026     0.938     0.894     0.885
       wst  bf16      0.949     0.936     0.918     0.915         -         -     0.958     0.912     0.905
       wst   f16      0.648     0.758     0.727     0.690         -         -     0.734     0.547     0.545
"""
import pytest
import torch

import gemm_op_cases as C

pytestmark = pytest.mark.gpu

N_CU = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
CASES = C.cases(N_CU)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def worst():
    """(kernel, epilogue, dtype) -> worst err / bar over the module's cases, printed at the end"""
    w = {}
    yield w
    for k in sorted(w):
        print(f"worst err / bar  {k[0]:>4} {k[1]:>10} {k[2]:>5}: {w[k]:.3f}")


def _run(L, c):
    """launch the case on the kernel it names; returns (status, inputs, buffers)"""
    assert C.route(L, c) == C.ROUTE_CODE[c.route], f"{c.id}: cfm_op_gemm_route says {C.route(L, c)}"
    inp = C.inputs(c, "cuda")
    b = C.buffers(c, inp)
    st = C.launch(L, c, inp, b, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, inp, b


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_gemm_case(L, worst, c):
    st, inp, b = _run(L, c)
    L.check(st)
    w = C.check(c, C.reference(c, inp), b)
    key = (c.route, C.EPI_NAME[c.epi] + (str(c.act) if c.epi in (C.STORE, C.GLU) else ""), c.dt)
    worst[key] = max(worst.get(key, 0.0), w)
    print(f"{c.id}: worst err / bar {w:.3f}")


# ---- refusals: the big kernels decline what their 16-B stores cannot take, and the call lands on 128 x 128 tiles
UNALIGNED = [
    C.Case(C.K128, dt, C.STORE, 257, 256, 128, act=2, variant=C.V_WST_OFF, row_off=3, o_pad=4, tag="ldo4")
    for dt in ("bf16", "f16")] + [
    C.Case(C.K128, "bf16", C.STORE, 200, 256, 512, act=1, variant=C.V_WST_ANY, row_off=2, o_pad=4, tag="wst-ldo4"),
    C.Case(C.K128, "f16", C.GLU, 200, 512, 512, act=3, variant=C.V_WST_ANY, row_off=2, o_pad=12, tag="wst-ldo12"),
    C.Case(C.K128, "bf16", C.GLU, 257, 512, 128, variant=C.V_WST_OFF, row_off=1, o_pad=4, tag="ldo4"),
    C.Case(C.K128, "bf16", C.STORE_F32, 257, 256, 192, alpha=22.625, variant=C.V_WST_OFF, row_off=1, o_pad=2, tag="ldo2"),
    C.Case(C.K128, "f16", C.RESID, 257, 256, 192, alpha=0.5, rowmask=True, variant=C.V_WST_OFF, o_pad=1, tag="ldx1"),
]
# an aligned pitch through an unaligned `out` (8 B into the row): the route query takes pointers as aligned, so
# only the result is checked
UNALIGNED_PTR = [
    C.Case(C.K256, "bf16", C.STORE, 257, 256, 128, variant=C.V_WST_OFF, row_off=3, o_pad=8, out_off=4, tag="out8B"),
    C.Case(C.KWST, "f16", C.STORE, 200, 256, 512, act=1, variant=C.V_WST_ANY, row_off=3, o_pad=8, out_off=4, tag="out8B"),
    C.Case(C.K256, "bf16", C.STORE_F32, 257, 256, 128, alpha=0.5, variant=C.V_WST_OFF, row_off=3, o_pad=4, out_off=2, tag="out8B"),
]


@pytest.mark.parametrize("c", UNALIGNED + UNALIGNED_PTR, ids=[c.id for c in UNALIGNED + UNALIGNED_PTR])
def test_unaligned_output_runs_on_128_tiles(L, c):
    if c.route == C.K128:   # the same call at the next aligned pitch is the big kernel's
        big = C.KWST if (c.variant >> 18) & 7 == 2 else C.K256
        pad = 8 if c.epi in (C.STORE, C.GLU) else 4
        assert C.route(L, C.replace(c, o_pad=(c.o_pad + pad - 1) // pad * pad)) == C.ROUTE_CODE[big]
    st, inp, b = _run(L, c)
    L.check(st)
    C.check(c, C.reference(c, inp), b)


@pytest.mark.parametrize("dt,K,variant", [("f32", 48, 0), ("bf16", 96, 0), ("bf16", 96, C.V_WST_OFF), ("f16", 32, C.V_SMALL),
                                          ("bf16", 544, C.V_WST_ANY)])
def test_k_off_the_step_is_an_error_and_writes_nothing(L, dt, K, variant):
    c = C.Case(C.K128, dt, C.STORE, 130, 256, K, variant=variant, row_off=2)
    assert C.route(L, c) == 0
    inp = C.inputs(c, "cuda")
    b = C.buffers(c, inp)
    st = C.launch(L, c, inp, b, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == L.CFM_ERR_RUNTIME
    with pytest.raises(RuntimeError):
        L.check(st)
    assert torch.isnan(b["out"]).all()
