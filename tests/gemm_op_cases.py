"""The case table of the projection GEMM's op-level parity tests (tests/test_gpu_ops_gemm.py runs it on the GPU,
tests/test_gemm_op_ref_cpu.py guards the reference and the bar on the CPU): the smallest shapes at which each path of
the three kernels behind cfm_op_gemm can still go wrong.

Every case names the kernel it must run on (`route`, asserted against cfm_op_gemm_route before the launch).  Inputs:
A ~ 0.5 N(0, 1), W ~ N(0, 1) / sqrt(K), a distinct N(0, 1) bias per column; the buffers are laid out by buffers():
row pitches equal to or larger than the logical width with NaN in the pad columns, NaN guard rows after A's M rows
and W's N rows, outputs prefilled with NaN, row_off > 0 where the epilogue has one.

One-hot cases are exact: row m of A is one-hot at k = (7 m + 3) % K, W in [-100, 100] and bias in [-28, 28] are
integers (|z| <= 128: exact in bf16), x integers, alpha a power of two, so every output is representable and the
kernel must reproduce the reference bit for bit.
"""
from dataclasses import dataclass, replace

import torch

from oracle import gemm_op_ref as R

STORE, STORE_F32, RESID, QKV, GLU = R.STORE, R.STORE_F32, R.RESID, R.QKV, R.GLU
EPI_NAME = {STORE: "store", STORE_F32: "store_f32", RESID: "resid", QKV: "qkv", GLU: "glu"}
K128, K256, KWST = "128", "256", "wst"            # the kernels, as the route query numbers them: 1, 2, 3
ROUTE_CODE = {K128: 1, K256: 2, KWST: 3}
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DT_CODE = {"f32": 0, "bf16": 1, "f16": 2}
# variant bits (include/cfm_ops.h)
V_SMALL, V_SC1, V_NT, V_WST_ANY, V_WST_OFF, V_DK128 = 1, 1 << 16, 2 << 16, 2 << 18, 7 << 18, 1 << 21
V_COL_GROUP2 = 2 << 22
V_NEVER_256 = 15 << 24
TILE_ROWS = {K128: 128, K256: 256, KWST: 64}


@dataclass(frozen=True)
class Case:
    route: str
    dt: str
    epi: int
    M: int
    N: int
    K: int
    act: int = 0
    variant: int = 0
    bias: bool = True
    alpha: float = 1.0
    rowmask: bool = False
    row_off: int = 0
    a_pad: int = 0          # lda = K + a_pad, ldw = K + w_pad, ldo / ldx = logical output width + o_pad
    w_pad: int = 0
    o_pad: int = 0
    out_off: int = 0        # elements between the output allocation and `out`
    onehot: bool = False
    tag: str = ""

    @property
    def d(self):
        return self.N // 3 if self.epi == QKV else 0

    @property
    def dk(self):
        return 128 if self.variant & V_DK128 else 64

    @property
    def out_cols(self):
        return self.N // 2 if self.epi == GLU else self.N

    @property
    def step(self):
        return 32 if self.dt == "f32" else 64

    @property
    def id(self):
        s = f"{self.route}-{self.dt}-{EPI_NAME[self.epi]}{self.act}-{self.M}x{self.N}x{self.K}"
        for flag, name in ((not self.bias, "nobias"), (self.rowmask, "mask"), (self.a_pad, "lda"), (self.o_pad, "ldo"),
                           (self.onehot, "onehot"), (self.dk == 128 and self.epi == QKV, "dk128"), (self.tag, self.tag)):
            if flag:
                s += "-" + name
        return s


def _epi_kw(name):
    """shorthand -> Case fields of one epilogue flavour"""
    return {"s0": dict(epi=STORE, act=0, row_off=3), "s1": dict(epi=STORE, act=1, row_off=2),
            "s2": dict(epi=STORE, act=2, row_off=1), "s3": dict(epi=STORE, act=3, row_off=5),
            "s0nb": dict(epi=STORE, act=0, row_off=3, bias=False),
            "f32": dict(epi=STORE_F32, alpha=22.625, row_off=4), "f32nb": dict(epi=STORE_F32, alpha=0.5, row_off=1, bias=False),
            "res": dict(epi=RESID, alpha=0.5), "resm": dict(epi=RESID, alpha=0.5, rowmask=True),
            "resmnb": dict(epi=RESID, alpha=2.0, rowmask=True, bias=False),
            "q64": dict(epi=QKV, row_off=5), "q128": dict(epi=QKV, row_off=6), "q64nb": dict(epi=QKV, row_off=5, bias=False),
            "g0": dict(epi=GLU, act=0, row_off=7), "g3": dict(epi=GLU, act=3, row_off=2)}[name]


def _mk(route, dt, name, M, N, K, variant=0, **kw):
    f = _epi_kw(name)
    if name == "q128":
        variant |= V_DK128
    return Case(route=route, dt=dt, M=M, N=N, K=K, variant=variant, **{**f, **kw})


def _pads(i, dt, epi, big):
    """alternate pitches: equal to the width, and larger (the big kernels need 16-B multiples, the 128 x 128 kernel's
    scalar stores take any output pitch: odd there)"""
    a = (0, 8, 0, 16)[i % 4]
    w = (0, 0, 8, 24)[i % 4]
    o = (0, 16, 0, 8)[(i // 2) % 4] if big else (0, 5, 0, 3)[(i // 2) % 4]
    return dict(a_pad=a, w_pad=w, o_pad=0 if epi == QKV else o)     # QKV rows have the fixed pitches d and 2 d


def cases(n_cu=256):
    """the table; n_cu sizes the cases that need more tiles than CUs (the CPU tests take 256)"""
    n_cu = (n_cu + 7) // 8 * 8
    out = []

    def add(route, dt, name, M, N, K, variant=0, **kw):
        c = _mk(route, dt, name, M, N, K, variant, **kw)
        pads = _pads(len(out), dt, c.epi, route != K128)
        out.append(replace(c, **{k: v for k, v in pads.items() if k not in kw}))

    # ---- 128 x 128 kernel: every M x N, K and the epilogue cycling through them; N = 384 takes QKV (d = 128) / GLU
    flat = ["s0", "s1", "s2", "s3", "f32", "resm", "s0nb", "res", "f32nb", "resmnb"]
    wide = ["q64", "q128", "g0", "g3", "q64nb", "resm", "s2"]
    for dt in ("f32", "bf16", "f16"):
        step = 32 if dt == "f32" else 64
        v = 0 if dt == "f32" else V_SMALL
        i = 0
        for N in (8, 48, 136, 384):
            for M in (1, 63, 64, 65, 127, 129, 257):
                K = (step, 3 * step, 512)[i % 3]
                add(K128, dt, (wide if N == 384 else flat)[i % (7 if N == 384 else 10)], M, N, K, v)
                i += 1
        # RESID + rowmask and no-bias on an N tail, by name (the cycle above has them too)
        add(K128, dt, "resm", 129, 136, 3 * step, v, o_pad=3)
        add(K128, dt, "s0nb", 65, 136, step, v, o_pad=5)
        # the vocabulary head's remainder: N = 136 columns at pitch 5000 through an `out` offset of 4864 floats
        add(K128, dt, "f32", 65, 136, 512, v, o_pad=5000 - 136, out_off=4864, tag="vocab")
    # ---- 256 x 256 kernel (weight-stationary off): row tails x {one column tile, QKV at d = 256}, nk = K / 64 in
    # {1, 2, 3, 5} at one tile per block
    for dt in ("bf16", "f16"):
        # with the walk and policy cases below every epilogue runs on both types
        one = {"bf16": ["s0", "f32", "resm", "g0", "s1"], "f16": ["s3", "s1", "f32", "g3", "res"]}[dt]
        i = 0
        for M in (1, 255, 256, 257, 513):
            for N in (256, 768):
                name = ("q64", "q128")[(i // 2) % 2] if N == 768 else one[i // 2]
                add(K256, dt, name, M, N, 64 * (1, 2, 3, 5)[i % 4], V_WST_OFF)
                i += 1
        for name in ("q64", "q128"):                                   # QKV at d = 512
            add(K256, dt, name, 257, 1536, 128, V_WST_OFF)
        for name, N in (("s0nb", 256), ("f32nb", 256), ("resmnb", 256), ("q64nb", 768)):
            add(K256, dt, name, 257, N, 192, V_WST_OFF)
        for name, N, pol in (("s2", 256, V_NT), ("q64", 768, V_SC1), ("g0", 512, V_NT), ("g3", 512, V_SC1), ("q128", 768, V_NT)):
            add(K256, dt, name, 300, N, 128, V_WST_OFF | pol, tag="pol%d" % (pol >> 16))
        # persistent walk: more tiles than CUs, T % 8 != 0 (5 column tiles), every nk: the ring phase at a tile's
        # start differs from tile to tile for odd nk; nk = 1: the prologue's second A stage is the next tile's
        nbm = n_cu // 5 + 1
        while (5 * nbm) % 8 == 0:
            nbm += 1
        names = {"bf16": ("s2", "s0", "s1", "s3"), "f16": ("s0", "resm", "s2", "g0")}[dt]
        for nk, name in zip((1, 2, 3, 5), names):
            add(K256, dt, name, 256 * (nbm - 1) + 1, 1280, 64 * nk, V_WST_OFF, tag="walk")
        nbm = n_cu // 6 + 1                                            # and once with column groups of 2 (6 column tiles)
        while (6 * nbm) % 8 == 0:
            nbm += 1
        add(K256, dt, "s0" if dt == "bf16" else "q64", 256 * (nbm - 1) + 7, 1536, 192, V_WST_OFF | V_COL_GROUP2, tag="cg2")
    # ---- weight-stationary kernel (K = 512) at any M
    for dt in ("bf16", "f16"):
        i = 0
        for N, names in ((256, ["s0", "s1", "s2", "s3", "g0", "g3"]), (512, ["s2", "g3", "s0", "g0", "s3", "s1"]),
                         (1536, ["q64", "q128", "g0", "s2", "q128", "q64"])):
            for M, name in zip((1, 63, 64, 65, 200, 64 * n_cu + 5), names):
                if M > 4096 and (N == 512) == (dt == "bf16"):          # the large M: N = 256, 1536 (bf16), 512 (f16)
                    M = 200 + 64 * 3
                add(KWST, dt, name, M, N, 512, V_WST_ANY)
                i += 1
    # ---- default routing (variant 0): the weight-stationary kernel from 128 row tiles of 64 on, GLU from 512
    for dt, name, N in (("bf16", "s0", 512), ("bf16", "q64", 1536), ("f16", "s2", 256)):
        add(K256, dt, name, 8128, N, 512, tag="edge")
        add(KWST, dt, name, 8129, N, 512, tag="edge")
    add(K256, "bf16", "g0", 32704, 256, 512, tag="edge")
    add(KWST, "bf16", "g0", 32705, 256, 512, tag="edge")
    # "never the 256 x 256 kernel": a 256-eligible shape on 128 x 128 tiles without forcing them
    add(K128, "bf16", "s0", 300, 256, 128, V_WST_OFF | V_NEVER_256, tag="bigmin")
    # ---- one-hot exactness on every kernel and type
    for route, dts, v, M, N, Nq, K in ((K128, ("f32", "bf16", "f16"), V_SMALL, 140, 136, 384, 192),
                                       (K256, ("bf16", "f16"), V_WST_OFF, 257, 256, 768, 192),
                                       (KWST, ("bf16", "f16"), V_WST_ANY, 200, 256, 1536, 512)):
        for dt in dts:
            vv = 0 if dt == "f32" else v
            names = ("s0", "s1", "q64", "q128") if route == KWST else ("s0", "s1", "f32", "resm", "q64", "q128")
            for name in names:
                add(route, dt, name, M, Nq if name[0] == "q" else N, K, vv, onehot=True,
                    **({"alpha": 0.25} if name == "resm" else {"alpha": 0.5} if name == "f32" else {}))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out


def seed_of(c):
    return (c.M * 7919 + c.N * 104729 + c.K * 31 + c.epi * 5 + c.act + len(c.dt) + c.variant % 1013) % (2 ** 31)


def inputs(c, device="cpu"):
    """logical inputs: A [M, K], W [N, K] in the operand type; bias [N], x [M, N] f32; rowmask [M] uint8 (or None)"""
    g = torch.Generator().manual_seed(seed_of(c))
    tdt = TDT[c.dt]
    if c.onehot:
        A = torch.zeros(c.M, c.K)
        A[torch.arange(c.M), (7 * torch.arange(c.M) + 3) % c.K] = 1.0
        W = torch.randint(-100, 101, (c.N, c.K), generator=g).float()
        bias = torch.randint(-28, 29, (c.N,), generator=g).float()
        x = torch.randint(-64, 65, (c.M, c.N), generator=g).float()
    else:
        A = 0.5 * torch.randn(c.M, c.K, generator=g)
        W = torch.randn(c.N, c.K, generator=g) / c.K ** 0.5
        bias = torch.randn(c.N, generator=g)
        x = torch.randn(c.M, c.N, generator=g)
    rowmask = (torch.arange(c.M) % 3 != 1).to(torch.uint8) if c.rowmask else None
    return dict(A=A.to(tdt).to(device), W=W.to(tdt).to(device), bias=bias.to(device) if c.bias else None,
                x=x.to(device) if c.epi == RESID else None, rowmask=rowmask.to(device) if c.rowmask else None)


def reference(c, inp):
    return R.gemm_op_ref(inp["A"], inp["W"], inp["bias"], c.epi, c.act, c.alpha, inp["x"], inp["rowmask"])


GUARD = 3   # NaN rows after the rows a kernel may touch


def buffers(c, inp):
    """the device-layout buffers of a launch: A / W at their pitches with NaN pads and guard rows; outputs NaN-filled"""
    dev, tdt = inp["A"].device, TDT[c.dt]
    nan = float("nan")

    def pitched(t, pad):
        b = torch.full((t.shape[0] + GUARD, t.shape[1] + pad), nan, dtype=t.dtype, device=dev)
        b[: t.shape[0], : t.shape[1]] = t
        return b

    b = dict(A=pitched(inp["A"], c.a_pad), W=pitched(inp["W"], c.w_pad))
    rows = c.row_off + c.M + GUARD
    if c.epi == RESID:
        b["x"] = pitched(inp["x"], c.o_pad)
    elif c.epi == QKV:
        b["q"] = torch.full((c.M + GUARD, c.d), nan, dtype=tdt, device=dev)
        b["kv"] = torch.full((rows, 2 * c.d), nan, dtype=tdt, device=dev)
    else:
        odt = torch.float32 if c.epi == STORE_F32 else tdt
        b["out"] = torch.full((rows, c.out_cols + c.o_pad), nan, dtype=odt, device=dev)
    return b


def check(c, ref, b, what=""):
    """every output element within the bar (bit-equal for a one-hot case), everything else still NaN; returns the
    worst err / bar"""
    M, worst = c.M, 0.0

    def close(got, y, bar, name):
        nonlocal worst
        got = got.double()
        assert not torch.isnan(got).any(), f"{c.id} {name}: NaN in the output {what}"
        if c.onehot:
            assert torch.equal(got, y), f"{c.id} {name}: one-hot result not exact ({(got != y).sum().item()} elements) {what}"
            return
        ratio = (got - y).abs() / bar
        w = ratio.max().item()
        worst = max(worst, w)
        if w > 1.0:
            i = ratio.argmax().item()
            r, col = divmod(i, y.shape[1])
            raise AssertionError(f"{c.id} {name}: |out - ref| = {(got - y).abs().flatten()[i].item():.4e} > bar "
                                 f"{bar.flatten()[i].item():.4e} at ({r}, {col}) ({w:.2f} x; {(ratio > 1).sum().item()} "
                                 f"elements over) {what}")

    def untouched(t, r0, r1, c1, name, c0=0):
        mask = torch.ones_like(t, dtype=torch.bool)
        mask[r0:r1, c0:c1] = False
        assert torch.isnan(t[mask]).all(), f"{c.id} {name}: wrote outside its rows / columns {what}"

    if c.epi == QKV:
        (q, kv), (bq, bkv) = R.qkv_split(ref.y, c.d, c.dk), R.qkv_split(ref.bar, c.d, c.dk)
        close(b["q"][:M], q, bq, "q")
        close(b["kv"][c.row_off: c.row_off + M], kv, bkv, "kv")
        untouched(b["q"], 0, M, c.d, "q")
        untouched(b["kv"], c.row_off, c.row_off + M, 2 * c.d, "kv")
    elif c.epi == RESID:
        close(b["x"][:M, : c.N], ref.y, ref.bar, "x")
        untouched(b["x"], 0, M, c.N, "x")
    else:
        close(b["out"][c.row_off: c.row_off + M, c.out_off: c.out_off + c.out_cols], ref.y, ref.bar, "out")
        untouched(b["out"], c.row_off, c.row_off + M, c.out_off + c.out_cols, "out", c.out_off)
    return worst


def pitches(c):
    """(lda, ldw, ldo, ldx) of the launch"""
    return (c.K + c.a_pad, c.K + c.w_pad, 0 if c.epi in (RESID, QKV) else c.out_cols + c.o_pad,
            c.N + c.o_pad if c.epi == RESID else 0)


def route(L, c):
    """the kernel cfm_op_gemm_route names for the case's launch"""
    lda, ldw, ldo, ldx = pitches(c)
    return L.cfm_op_gemm_route(DT_CODE[c.dt], c.epi, c.act, lda, ldw, c.M, c.N, c.K, int(c.bias), ldo, ldx, c.variant)


def launch(L, c, inp, b, stream):
    """cfm_op_gemm on the buffers of buffers(); returns the status"""
    lda, ldw, ldo, ldx = pitches(c)
    out = out2 = x = 0
    if c.epi == RESID:
        x = b["x"].data_ptr()
    elif c.epi == QKV:
        out, out2 = b["q"].data_ptr(), b["kv"].data_ptr()
    else:
        out = b["out"].data_ptr() + c.out_off * b["out"].element_size()
    return L.cfm_op_gemm(DT_CODE[c.dt], c.epi, c.act, b["A"].data_ptr(), lda, b["W"].data_ptr(), ldw, c.M, c.N, c.K,
                         L.ptr(inp["bias"]), c.alpha, out, ldo, c.row_off, out2, c.d, x, ldx, L.ptr(inp["rowmask"]),
                         c.variant, stream)
