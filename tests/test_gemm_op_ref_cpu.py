"""CPU-side guard of the projection GEMM's operator parity test (tests/test_gpu_ops_gemm.py): the float64 reference
(oracle/gemm_op_ref.py) is pinned to independent torch code, its per-element bar is shown to be wide enough for a
correct f32-accumulating kernel whatever its summation order, and narrow enough to see the errors a kernel can make
silently -- on the table's own inputs each mutation must exceed the bar 10 x on at least one element of every case it
applies to.  The route query of the library is checked on the whole table (host code: no GPU involved)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_op_cases as C
from oracle import attention_op_ref
from oracle import gemm_op_ref as R

MARGIN = 10.0
CASES = C.cases(256)
IDS = [c.id for c in CASES]


def _rows(c, limit=192):
    """all rows of a small case; of a large one the first rows, the whole last row tile and a stride through the rest
    (every check here is row-local, so a row subset checks every element of those rows)"""
    if c.M <= limit:
        return torch.arange(c.M)
    last = (c.M - 1) // C.TILE_ROWS[c.route] * C.TILE_ROWS[c.route]
    return torch.unique(torch.cat([torch.arange(66), torch.arange(max(last - 2, 0), c.M),
                                   torch.arange(0, c.M, max(1, c.M // 61))]))


@functools.lru_cache(maxsize=None)
def _sub(i):
    """(case restricted to _rows, inputs, reference)"""
    c = CASES[i]
    idx = _rows(c)
    inp = C.inputs(c)
    inp = {k: (v[idx] if v is not None and k in ("A", "x", "rowmask") else v) for k, v in inp.items()}
    sub = C.replace(c, M=len(idx))
    return sub, inp, C.reference(sub, inp), idx


# ------------------------------------------------------------------------------------------ (a) the reference, pinned
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_reference_matches_independent_torch(dt):
    g = torch.Generator().manual_seed(1)
    M, N, K = 37, 384, 192
    A = (0.5 * torch.randn(M, K, generator=g)).to(C.TDT[dt])
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(C.TDT[dt])
    b = torch.randn(N, generator=g)
    x = torch.randn(M, N, generator=g)
    rm = (torch.rand(M, generator=g) > 0.4).to(torch.uint8)
    z = F.linear(A.double(), W.double(), b.double())
    tol = dict(rtol=1e-12, atol=1e-12)
    for act, f in ((0, lambda t: t), (1, F.relu), (2, F.silu), (3, lambda t: -F.silu(-t * math.log(2.0)) / math.log(2.0))):
        r = R.gemm_op_ref(A, W, b, R.STORE, act)
        torch.testing.assert_close(r.y, f(z), **tol)
        torch.testing.assert_close(r.z, z, **tol)
    torch.testing.assert_close(R.gemm_op_ref(A, W, None, R.STORE).y, F.linear(A.double(), W.double()), **tol)
    torch.testing.assert_close(R.gemm_op_ref(A, W, b, R.STORE_F32, alpha=22.625).y, 22.625 * z, **tol)
    torch.testing.assert_close(R.gemm_op_ref(A, W, b, R.RESID, alpha=0.5, x=x, rowmask=rm).y,
                               x.double() + 0.5 * z * rm.double()[:, None], **tol)
    torch.testing.assert_close(R.gemm_op_ref(A, W, b, R.RESID, alpha=0.5, x=x).y, x.double() + 0.5 * z, **tol)
    # S bounds every partial sum: |z| <= S, and S of non-negative inputs is z
    r = R.gemm_op_ref(A.abs(), W.abs(), b.abs(), R.STORE)
    torch.testing.assert_close(r.S, r.z, **tol)
    assert (R.gemm_op_ref(A, W, b, R.STORE).S >= z.abs()).all()
    # GLU: channel 16 blk + i of the output pairs columns 32 blk + i (a) and 32 blk + 16 + i (gate)
    n = torch.arange(N)
    is_gate, ch = (n % 32) >= 16, (n // 32) * 16 + n % 16
    a, gt = torch.empty(M, N // 2, dtype=torch.float64), torch.empty(M, N // 2, dtype=torch.float64)
    a[:, ch[~is_gate]] = z[:, ~is_gate]
    gt[:, ch[is_gate]] = z[:, is_gate]
    torch.testing.assert_close(R.gemm_op_ref(A, W, b, R.GLU, 0).y, F.glu(torch.cat([a, gt], -1)), **tol)
    torch.testing.assert_close(R.gemm_op_ref(A, W, b, R.GLU, 3).y, a / (1 + 2.0 ** gt), **tol)


@pytest.mark.parametrize("dk", [64, 128])
@pytest.mark.parametrize("d", [128, 256, 512])
def test_kv_interleave_is_the_attention_operators(d, dk):
    """the K | V stream rows as cfm_op_attention's reference reads them: [H][K dk | V dk]"""
    M, H = 5, d // dk
    y = torch.arange(M * 3 * d, dtype=torch.float64).reshape(M, 3 * d)
    q, kv = R.qkv_split(y, d, dk)
    assert torch.equal(q, y[:, :d])
    kw = kv.view(M, H, 2 * dk)                                   # oracle/attention_op_ref.py: kw[..., :dk] K, [..., dk:] V
    assert torch.equal(kw[..., :dk].reshape(M, d), y[:, d: 2 * d])
    assert torch.equal(kw[..., dk:].reshape(M, d), y[:, 2 * d:])
    # and through the attention reference itself: one query on one key row returns that row's V
    qq = torch.zeros(1, d, dtype=torch.float64)
    desc = torch.tensor([[0, 1, 0, 0, 1, 0, 1, 0]])
    o = attention_op_ref.attention_op_ref(qq, kv[:1], torch.zeros(1, d, dtype=torch.float64), torch.zeros(d), torch.zeros(d),
                                          desc, H, dk)
    assert torch.equal(o, y[:1, 2 * d:])


# ------------------------------------------------------------------------- (b) the bar is not too tight: no kernel needed
def _emulate(c, inp, order):
    """a correct kernel in torch float32: products and sums in f32 in the given order, the epilogue in f32, one
    rounding to the output type"""
    A, W = inp["A"].float(), inp["W"].float()
    bias = inp["bias"] if inp["bias"] is not None else torch.zeros(c.N)
    if order == "forward":                       # the bias seeds the accumulator
        acc = bias.expand(c.M, c.N).clone()
        for k in range(c.K):
            acc = acc + A[:, k, None] * W[None, :, k]
    elif order == "reversed":                    # the bias comes last
        acc = torch.zeros(c.M, c.N)
        for k in reversed(range(c.K)):
            acc = acc + A[:, k, None] * W[None, :, k]
        acc = acc + bias
    else:                                        # 32-wide blocks (one MFMA each), the blocks in order
        acc = torch.zeros(c.M, c.N)
        for k in range(0, c.K, 32):
            acc = acc + A[:, k: k + 32] @ W[:, k: k + 32].t()
        acc = acc + bias
    if c.epi == C.STORE or c.epi == C.QKV:
        y = (acc if c.act == 0 else F.relu(acc) if c.act == 1 else acc * torch.sigmoid(acc) if c.act == 2
             else acc / (1 + torch.exp2(acc)))
    elif c.epi == C.STORE_F32:
        y = torch.tensor(c.alpha, dtype=torch.float32) * acc
    elif c.epi == C.RESID:
        m = inp["rowmask"].float()[:, None] if inp["rowmask"] is not None else 1.0
        y = inp["x"] + (torch.tensor(c.alpha, dtype=torch.float32) * acc) * m
    else:
        a, gt = R.glu_halves(acc)
        y = a * torch.sigmoid(gt) if c.act == 0 else a / (1 + torch.exp2(gt))
    return y


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_bar_admits_a_correct_f32_kernel(i):
    c, inp, ref, _ = _sub(i)
    worst = 0.0
    for order in ("forward", "reversed", "blocked32"):
        y = _emulate(c, inp, order).to(ref.out_dtype).double()
        if c.onehot:
            assert torch.equal(y, ref.y), f"{c.id}: the one-hot case is not exact in {c.dt} ({order})"
            continue
        ratio = ((y - ref.y).abs() / ref.bar).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{c.id}: a correct kernel ({order} summation) is {ratio:.2f} x the bar"
    print(f"{c.id}: worst emulated err / bar {worst:.3f}")


# --------------------------------------------------------------------------------- (c) the bar sees silent errors
def _swap_glu_halves(t):
    v = t.reshape(-1, 2, 16, *t.shape[1:])
    return torch.stack([v[:, 1], v[:, 0]], 1).reshape(t.shape)


def _mutations(c, inp, ref):
    """name -> mutated full-precision output (projection order for QKV), for every mutation that applies to the case"""
    step, out = c.step, {}
    run = lambda cc=c, **kw: C.reference(cc, {**inp, **kw}).y
    last = (c.M - 1) // C.TILE_ROWS[c.route] * C.TILE_ROWS[c.route]
    A = inp["A"]
    A2 = A.clone()
    A2[last:, c.K - step:] = 0
    out["last K step dropped for the last row tile"] = run(A=A2)
    if c.K >= 2 * step:
        A2 = A.clone()
        A2[:, step: 2 * step] = A[:, :step]
        out["K step 1 read from step 0's A"] = run(A=A2)
    if ref.y.shape[1] >= 32:
        y = ref.y.clone()
        y[:, :16], y[:, 16:32] = ref.y[:, 16:32], ref.y[:, :16]
        out["two 16-column blocks swapped"] = y
    if c.bias:
        out["bias shifted one column"] = run(bias=inp["bias"].roll(1))
    if c.rowmask and (inp["rowmask"] == 0).any():
        out["rowmask ignored"] = run(rowmask=None)
    if c.epi in (C.STORE_F32, C.RESID) and c.alpha != 1.0:
        out["alpha dropped"] = run(C.replace(c, alpha=1.0))
    if c.epi == C.GLU:
        out["GLU halves swapped"] = run(W=_swap_glu_halves(inp["W"]), bias=_swap_glu_halves(inp["bias"]))
    if c.act == 3:
        out["act 3 computed as act 2"] = run(C.replace(c, act=2))
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_bar_sees_silent_errors(i):
    c, inp, ref, idx = _sub(i)
    # the last row tile must be among the rows kept
    assert (c.M - 1) // C.TILE_ROWS[c.route] * C.TILE_ROWS[c.route] < c.M
    seen = {name: ((y - ref.y).abs() / ref.bar).max().item() for name, y in _mutations(c, inp, ref).items()}
    if c.epi == C.QKV and c.dk == 128:
        kv, bar = R.qkv_split(ref.y, c.d, 128)[1], R.qkv_split(ref.bar, c.d, 128)[1]
        seen["K | V interleave of dk 64 used for 128"] = ((R.qkv_split(ref.y, c.d, 64)[1] - kv).abs() / bar).max().item()
    assert seen
    for name, r in seen.items():
        print(f"{c.id}: {name}: {r:.3g} x the bar")
    for name, r in seen.items():
        assert r >= MARGIN, f"{c.id}: {name} moves the output by only {r:.3g} x the bar"


def test_every_mutation_is_exercised():
    names = set()
    for i, c in enumerate(CASES):
        if c.M <= 300:
            sub, inp, ref, _ = _sub(i)
            names |= set(_mutations(sub, inp, ref))
    assert names >= {"last K step dropped for the last row tile", "K step 1 read from step 0's A",
                     "two 16-column blocks swapped", "bias shifted one column", "rowmask ignored", "alpha dropped",
                     "GLU halves swapped", "act 3 computed as act 2"}
    assert any(c.epi == C.QKV and c.dk == 128 for c in CASES)


# ------------------------------------------------------------------------------------------ (d) routing, on the host
@pytest.fixture(scope="module")
def lib():
    from chunkformer_amd import build
    build.build()
    from chunkformer_amd import _lib
    return _lib


def route_of(L, c, **kw):
    a = dict(lda=c.K + c.a_pad, ldw=c.K + c.w_pad, ldo=0 if c.epi in (C.RESID, C.QKV) else c.out_cols + c.o_pad,
             ldx=c.N + c.o_pad if c.epi == C.RESID else 0, variant=c.variant, K=c.K)
    a.update(kw)
    return L.cfm_op_gemm_route(C.DT_CODE[c.dt], c.epi, c.act, a["lda"], a["ldw"], c.M, c.N, a["K"], int(c.bias), a["ldo"],
                               a["ldx"], a["variant"])


def test_route_of_every_case(lib):
    for n_cu in (256, 304, 64):
        for c in C.cases(n_cu):
            assert route_of(lib, c) == C.ROUTE_CODE[c.route], c.id


def test_route_guards(lib):
    """the big kernels decline pitches their 16-B stores cannot take; K off the step is an error"""
    by = {c.id: c for c in CASES}
    for c in CASES:
        if c.route == C.K128 or c.onehot or c.M > 600:
            continue
        if c.epi in (C.STORE, C.GLU):
            assert route_of(lib, c, ldo=c.out_cols + 4) == 1, c.id        # 8 B: not a 16-B multiple of 16-bit elements
            assert route_of(lib, c, ldo=c.out_cols + 8) == C.ROUTE_CODE[c.route], c.id
        if c.epi == C.STORE_F32:
            assert route_of(lib, c, ldo=c.N + 2) == 1, c.id
            assert route_of(lib, c, ldo=c.N + 4) == C.ROUTE_CODE[c.route], c.id
        if c.epi == C.RESID:
            assert route_of(lib, c, ldx=c.N + 1) == 1, c.id
        assert route_of(lib, c, lda=c.K + 4) == 0, c.id                   # no kernel loads 8-B rows
        assert route_of(lib, c, K=c.K + 32) == 0, c.id
    c = C.Case(route=C.K128, dt="f32", epi=C.STORE, M=5, N=8, K=32)
    assert route_of(lib, c) == 1 and route_of(lib, c, K=48) == 0 and route_of(lib, C.replace(c, M=0)) == 0
    assert route_of(lib, C.replace(c, epi=C.GLU, N=48)) == 0              # GLU pairs 16-column blocks
    assert route_of(lib, C.replace(c, epi=C.GLU, N=64, bias=False)) == 0
    assert by  # table not empty
