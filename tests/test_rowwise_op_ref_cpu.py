"""CPU-side guard of the row-wise operator parity tests (tests/test_gpu_ops_rowwise.py): the fp64 references are
pinned to independent code (oracle/encoder_ref.py, torch.nn.functional.layer_norm), the E_round tables the 16-bit
bars come from are recomputed, and the bars are shown to see the errors a kernel can make silently -- on the tests'
own inputs each mutation of the reference must move the output by at least 10 x the bar."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import rowwise_op_cases as A
from oracle import encoder_ref
from oracle import rowwise_op_ref as R
from test_gpu_ops_rowwise import BAR, E_ROUND, F32_BAR

MARGIN = 10.0
PIN = 1e-5


# ------------------------------------------------------------------------------------------ the references, pinned
def test_fmaf32_is_one_rounding():
    """against exact rational arithmetic: products whose sum with x falls on f32 rounding ties after a first
    rounding to float64 (the double-rounding trap) and random triples"""
    from fractions import Fraction
    g = torch.Generator().manual_seed(5)
    a = torch.randn(4000, generator=g)
    y = torch.randn(4000, generator=g)
    x = torch.randn(4000, generator=g) * torch.tensor([1.0, 1e-3, 1e3, 2.0 ** 20])[torch.arange(4000) % 4]
    # the double-rounding trap: a y = 2^6 - 2^-40 and x = 2^30 + 2^7 (odd significand, ulp 2^7).  The exact sum lies
    # just below the midpoint x + 2^6 and rounds to x; float64 addition rounds it onto the midpoint, and a second
    # rounding (ties to even) would give x + 2^7.  And its mirror image.
    a = torch.cat([a, torch.tensor([2.0 ** 3 + 2.0 ** -20, -(2.0 ** 3 + 2.0 ** -20)])])
    y = torch.cat([y, torch.tensor([2.0 ** 3 - 2.0 ** -20, 2.0 ** 3 - 2.0 ** -20])])
    x = torch.cat([x, torch.tensor([2.0 ** 30 + 2.0 ** 7, -(2.0 ** 30 + 2.0 ** 7)])])
    naive = (a.double() * y.double() + x.double()).float()
    assert (naive[-2:] != x[-2:]).all(), "the trap inputs no longer trap"
    got = R.fmaf32(a, y, x)
    for ai, yi, xi, gi in zip(a.tolist(), y.tolist(), x.tolist(), got.tolist()):
        exact = Fraction(ai) * Fraction(yi) + Fraction(xi)
        lo = torch.tensor(float(exact), dtype=torch.float64).float()            # a neighbour of the exact value
        inf = torch.tensor(float("inf"))
        cands = [torch.nextafter(lo, -inf).item(), lo.item(), torch.nextafter(lo, inf).item()]
        best = min(abs(Fraction(c) - exact) for c in cands)
        assert abs(Fraction(gi) - exact) == best, (ai, yi, xi, gi)


@pytest.mark.parametrize("kindv", list(A.LN_KINDS))
def test_layernorm_reference_matches_torch(kindv):
    for M, form in A.ln_case_list(kindv):
        c = A.ln_case(kindv, 128, M, form, "fp32")
        v = c.x.double()
        if c.y is not None:
            v = v + A.ALPHA * (c.ymask.double().view(-1, 1) if c.ymask is not None else 1.0) * c.y.double()
        if c.y2 is not None:
            v = v + A.ALPHA2 * (c.ymask2.double().view(-1, 1) if c.ymask2 is not None else 1.0) * c.y2.double()
        t = F.layer_norm(v, (c.d,), c.w1.double(), c.b1.double(), A.EPS)
        if c.kind == R.LN:
            exp = t if c.rowmask is None else t * c.rowmask.double().view(-1, 1)
            assert A.rel_err(c.x_ref, c.x.double() if (c.f.defer or c.y is None) else v) <= PIN
        else:
            assert A.rel_err(c.x_ref, t) <= PIN
            exp = F.layer_norm(t, (c.d,), c.w2.double(), c.b2.double(), A.EPS) if c.w2 is not None else t
        assert A.rel_err(c.ref, exp) <= PIN, (M, form)
        const = c.rk == 3
        if c.w2 is None and c.rowmask is None and const.any():
            assert torch.equal(c.ref[const], c.b1.double().expand(int(const.sum()), c.d)), "constant rows: out = b"


def test_conv_reference_matches_padded_oracle():
    """encoder_ref._conv_padded with pointwise_conv1 = (identity | gate saturated at sigmoid(40) = 1) and
    pointwise_conv2 = identity: the dynamic-chunk padded conv module on the GLU rows themselves; full attention and
    chunked, against this reference on plan_padded's descriptors"""
    d = 16
    for tp, C in ((70, -1), (33, -1), (70, 16), (1, -1)):
        g = A.conv_geometry(("padded", tp, C))
        gen = torch.Generator().manual_seed(tp + 7 * max(C, 0))
        lens_sub = torch.tensor([tp, max(1, 2 * tp // 3)])
        h = torch.randn(2, tp, d, generator=gen, dtype=torch.float64)
        c = "c."
        eye = torch.eye(d, dtype=torch.float64)
        sd = {c + "pointwise_conv1.weight": torch.cat([eye, torch.zeros(d, d, dtype=torch.float64)])[:, :, None],
              c + "pointwise_conv1.bias": torch.cat([torch.zeros(d), torch.full((d,), 40.0)]).double(),
              c + "depthwise_conv.weight": 0.3 * torch.randn(d, 1, 15, generator=gen, dtype=torch.float64),
              c + "depthwise_conv.bias": 0.3 * torch.randn(d, generator=gen, dtype=torch.float64),
              c + "norm.weight": 1 + 0.3 * torch.randn(d, generator=gen, dtype=torch.float64),
              c + "norm.bias": 0.3 * torch.randn(d, generator=gen, dtype=torch.float64),
              c + "pointwise_conv2.weight": eye[:, :, None], c + "pointwise_conv2.bias": torch.zeros(d).double()}
        exp = encoder_ref._conv_padded(h, sd, c, None, lens_sub, C)
        valid = torch.arange(tp)[None, :] < lens_sub[:, None]
        glu = (h * valid[..., None]).reshape(2 * tp, d)
        got = R.conv_module_op_ref(glu, g.desc, sd[c + "depthwise_conv.weight"][:, 0, :].t().contiguous(),
                                   sd[c + "depthwise_conv.bias"], sd[c + "norm.weight"], sd[c + "norm.bias"], A.EPS,
                                   g.rows).view(2, tp, d)
        assert torch.isfinite(got).all()
        assert ((got - exp)[valid].abs().max() / exp[valid].abs().max()).item() <= PIN, (tp, C)


def test_conv_reference_matches_masked_layer_oracle():
    """the masked-window path of encoder_ref.layer_masked: a layer whose FFNs and attention output are zero and
    whose pointwise convs are identities, so that its output is norm_final(x + mask * conv_module(norm_conv(x)))
    -- the conv module on plan_masked's descriptors, with a carried offset and a T < 15 utterance"""
    d, H, C, L_, Rc = 16, 2, 8, 16, 8
    key = ("masked", C, Rc, (5, 0, 9, 0, 1))
    g = A.conv_geometry(key)
    lens, offs = A.masked_lens(C), list(key[3])
    att_mask, mask_pad, nch = encoder_ref.masks_closed_form(lens, offs, C, L_, Rc)
    N = sum(nch)
    assert N * C == g.rows
    gen = torch.Generator().manual_seed(11)
    f64 = dict(generator=gen, dtype=torch.float64)
    p, eye, zero = "l.", torch.eye(d, dtype=torch.float64), torch.zeros(d, d, dtype=torch.float64)
    sd = {}
    for n in ("norm_ff_macaron", "norm_mha", "norm_conv", "norm_ff", "norm_final"):
        sd[p + n + ".weight"], sd[p + n + ".bias"] = torch.ones(d).double(), torch.zeros(d).double()
    for n in ("feed_forward_macaron", "feed_forward"):
        sd[p + n + ".w_1.weight"], sd[p + n + ".w_1.bias"] = eye, torch.zeros(d).double()
        sd[p + n + ".w_2.weight"], sd[p + n + ".w_2.bias"] = zero, torch.zeros(d).double()
    a = p + "self_attn."
    for n in ("linear_q", "linear_k", "linear_v"):
        sd[a + n + ".weight"], sd[a + n + ".bias"] = eye, torch.zeros(d).double()
    sd[a + "linear_out.weight"], sd[a + "linear_out.bias"] = zero, torch.zeros(d).double()
    sd[a + "linear_pos.weight"] = eye
    sd[a + "pos_bias_u"] = sd[a + "pos_bias_v"] = torch.zeros(H, d // H).double()
    c = p + "conv_module."
    sd[c + "pointwise_conv1.weight"] = torch.cat([eye, zero])[:, :, None]
    sd[c + "pointwise_conv1.bias"] = torch.cat([torch.zeros(d), torch.full((d,), 40.0)]).double()
    sd[c + "depthwise_conv.weight"] = 0.3 * torch.randn(d, 1, 15, **f64)
    sd[c + "depthwise_conv.bias"] = 0.3 * torch.randn(d, **f64)
    sd[c + "norm.weight"], sd[c + "norm.bias"] = 1 + 0.3 * torch.randn(d, **f64), 0.3 * torch.randn(d, **f64)
    sd[c + "pointwise_conv2.weight"], sd[c + "pointwise_conv2.bias"] = eye[:, :, None], torch.zeros(d).double()
    cfg = SimpleNamespace(d_model=d, n_heads=H, head_dim=d // H)
    # (layer_masked runs its softmax in f32: the layer in f32, this reference in float64 on the same f32 values)
    sd = {k: v.float() for k, v in sd.items()}
    x32 = torch.randn(N, C, d, generator=gen)
    pos = torch.zeros(L_ + 2 * C + Rc - 1, d)
    mp = torch.from_numpy(mask_pad).double()
    exp, _, _ = encoder_ref.layer_masked(x32, sd, p, cfg, torch.from_numpy(att_mask), mp.float(), pos, C, L_, Rc, None,
                                         None, 0)
    assert torch.isfinite(exp).all()
    exp, x = exp.double(), x32.double()
    # this reference: the GLU stream [7 zero rows | norm_conv(x) | 7 zero rows], the plan's descriptors
    hc = F.layer_norm(x, (d,)).reshape(N * C, d)
    glu = torch.cat([torch.zeros(7, d, dtype=torch.float64), hc, torch.zeros(7, d, dtype=torch.float64)])
    assert glu.shape[0] == g.glu_rows
    y = R.conv_module_op_ref(glu, g.desc, sd[c + "depthwise_conv.weight"][:, 0, :].t().contiguous(),
                             sd[c + "depthwise_conv.bias"], sd[c + "norm.weight"], sd[c + "norm.bias"], A.EPS, g.rows)
    assert torch.isfinite(y).all()
    got = F.layer_norm(x + (y.view(N, C, d) * mp[:, 7: 7 + C, None]), (d,))
    assert ((got - exp).abs().max() / exp.abs().max()).item() <= PIN


@pytest.mark.parametrize("d", A.POS_D)
def test_pos_table_reference_matches_encoder_oracle(d):
    pe = encoder_ref.pos_table(d).double()                    # row r <-> distance 4999 - r
    for name in A.POS_KEYS:
        c = A.pos_case(name, d)
        r0 = 4999 - c.anchor
        assert A.rel_err(c.ref, pe[r0: r0 + c.p_rows]) <= PIN, name


# ------------------------------------------------------------------------------------------ the E_round tables
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_e_round_table_layernorm(dt):
    worst = max((A.ln_e_round(*k, dt), k) for k in A.ln_all_cases())
    print(f"E_round(layernorm, {dt}) = {worst[0]:.3e} at {worst[1]}")
    assert 0.9 * E_ROUND["layernorm"][dt] <= worst[0] <= E_ROUND["layernorm"][dt]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_e_round_table_conv_module(dt):
    worst = max((A.conv_e_round(k, d, dt), k, d) for k, d in A.conv_all_cases())
    print(f"E_round(conv_module, {dt}) = {worst[0]:.3e} at {worst[1:]}")
    assert 0.9 * E_ROUND["conv_module"][dt] <= worst[0] <= E_ROUND["conv_module"][dt]


# ------------------------------------------------------------------------------------------ sensitivity: LayerNorm
def _ln_mut(c, unbiased=False, eps=A.EPS, **over):
    """the LN case's output with one thing wrong (plain float64; `over` replaces residual arguments)"""
    kw = dict(y=c.y, alpha=A.ALPHA, ymask=c.ymask, y2=c.y2, alpha2=A.ALPHA2, ymask2=c.ymask2)
    kw.update(over)
    v = R.resid_chain(c.x, **kw).double()

    def ln(t, w, b):
        m = t.mean(-1, keepdim=True)
        var = ((t - m) ** 2).sum(-1, keepdim=True) / (c.d - 1 if unbiased else c.d)
        return (t - m) / torch.sqrt(var + eps) * w.double() + b.double()
    t = ln(v, c.w1, c.b1)
    if c.kind != R.LN and c.w2 is not None:
        t = ln(t, c.w2, c.b2)
    return t


def _report(seen, bar, what):
    for name, e in seen.items():
        print(f"{what}: {name}: {e:.3e} = {e / bar:.0f} x the bar")
    for name, e in seen.items():
        assert e >= MARGIN * bar, f"{what}: {name} moves the output by {e:.3e} < {MARGIN} x the bar ({bar:.3e})"


@pytest.mark.parametrize("dt", A.DTS)
@pytest.mark.parametrize("d", A.DS)
def test_bar_sees_layernorm_errors(d, dt):
    bar, seen = BAR["layernorm"][dt], {}
    # eps dropped: on the small-variance rows.  (Rows of std 1e-2 alone move by 5 % of their values, sqrt(1.1) - 1:
    # 10 x the fp32 and fp16 bars but not 10 x the bf16 bar, which is why the table also has rows of std 2e-3.)
    c = A.ln_case("ln", d, 1001, "y", dt)
    small = (c.rk == 2) | (c.rk == 4)
    seen["eps dropped"] = ((_ln_mut(c, eps=0.0) - c.ref)[small].abs().max() / c.scale).item()
    only_1e2 = ((_ln_mut(c, eps=0.0) - c.ref)[c.rk == 2].abs().max() / c.scale).item()
    print(f"eps dropped, std 1e-2 rows alone: {only_1e2:.3e} = {only_1e2 / bar:.1f} x the bar")
    if dt != "bf16":
        seen["eps dropped (std 1e-2 rows)"] = only_1e2
    # a mask ignored (either branch), alpha2 on the wrong branch
    c = A.ln_case("ln", d, 1001, "yy_m12", dt)
    seen["ymask ignored"] = A.rel_err(_ln_mut(c, ymask=None), c.ref)
    seen["ymask2 ignored"] = A.rel_err(_ln_mut(c, ymask2=None), c.ref)
    seen["alpha / alpha2 swapped"] = A.rel_err(_ln_mut(c, alpha=A.ALPHA2, alpha2=A.ALPHA), c.ref)
    c = A.ln_case("ln", d, 1001, "yy_m12_rowmask", dt)
    seen["rowmask ignored"] = A.rel_err(_ln_mut(c), c.ref)
    # the last row of an odd M taken from its neighbour (ln2_kernel's row1 == row0 duplicate, one off)
    for kv in ("ln2_w2", "ln2", "ln2_f32"):
        for M in (3, 5, 7, 9, 1001):
            form = next(f for m, f in A.ln_case_list(kv) if m == M)
            c = A.ln_case(kv, d, M, form, dt)
            seen[f"last row of M={M} from its neighbour ({kv})"] = ((c.ref[M - 2] - c.ref[M - 1]).abs().max() / c.scale).item()
    _report(seen, bar, f"layernorm {dt} d={d}")


@pytest.mark.parametrize("d", A.DS)
def test_bar_sees_unbiased_variance(d):
    """the unbiased estimator scales every normalised value by sqrt((d - 1) / d): a relative 1 / (2 d), i.e. 3.9e-3,
    2.0e-3 and 9.8e-4 of the values at d = 128, 256, 512.  That is 10 x the f32 bar (every fp32 output, and the f32
    outputs of the 16-bit kernels: LN2_F32's out, ln2_kernel's x) at d = 128 and 256, 9 x at d = 512, and below the
    rounding of a 16-bit output at any d -- no input changes a ratio that depends on d alone, so the 16-bit outputs
    and d = 512 are asserted at what the estimator gives: the f32 bar itself."""
    c = A.ln_case("ln2_f32", d, 1001, "yy", "fp32")
    e = A.rel_err(_ln_mut(c, unbiased=True), c.ref)
    print(f"unbiased variance d={d}: {e:.3e} = {e / F32_BAR:.1f} x the f32 bar")
    assert e >= (MARGIN if d < 512 else 5.0) * F32_BAR


# ------------------------------------------------------------------------------------------ sensitivity: conv module
SENS_CONV = [("masked", 64, 8, (0, 3, 10, 0, 0)), ("masked", 128, 3, (0, 3, 10, 0, 0)), ("padded", 70, 16),
             ("padded", 130, -1), ("stream", 70, 64, 16)]


@pytest.mark.parametrize("dt", A.DTS)
@pytest.mark.parametrize("d", A.DS)
@pytest.mark.parametrize("key", SENS_CONV, ids=lambda k: "-".join(map(str, k)).replace(" ", ""))
def test_bar_sees_conv_module_errors(key, d, dt):
    """mutated descriptors / taps on the un-poisoned copy of the GLU stream (rows outside the real ranges hold a
    neighbour's data, 8 x larger, instead of NaN)"""
    c = A.conv_case(key, d, dt)
    g, bar, seen = c.g, BAR["conv_module"][dt], {}
    ref = R.conv_module_op_ref(c.glu_full, g.desc, c.wdw, c.bdw, c.lnw, c.lnb, A.EPS, g.rows)
    assert A.rel_err(ref, c.ref) == 0.0          # the poisoned rows are never read

    def mut(desc=None, wdw=None):
        out = R.conv_module_op_ref(c.glu_full, g.desc if desc is None else desc, c.wdw if wdw is None else wdw,
                                   c.bdw, c.lnw, c.lnb, A.EPS, g.rows)
        return A.rel_err(out, c.ref)
    nout, s0, jlo, jhi = g.desc[:, 1], g.desc[:, 2], g.desc[:, 3], g.desc[:, 4]
    d_ = g.desc.clone()
    clipped = (jlo > 0) & (jhi > jlo) & (s0 + jlo - 1 >= 0)
    if clipped.any():
        d_[clipped, 3] -= 1
        seen["J_LO - 1"] = mut(desc=d_)
    d_ = g.desc.clone()
    clipped = (jhi < nout + 14) & (jhi > jlo)
    if clipped.any():
        d_[clipped, 4] += 1
        seen["J_HI + 1"] = mut(desc=d_)
    assert "J_LO - 1" in seen or "J_HI + 1" in seen
    d_ = g.desc.clone()
    d_[:, 2] += 1
    seen["SRC_ROW0 + 1"] = mut(desc=d_)
    seen["tap order reversed"] = mut(wdw=c.wdw.flip(0))
    w = c.wdw.clone()
    w[14] = 0
    seen["tap 14 dropped"] = mut(wdw=w)
    _report(seen, bar, f"conv_module {key} {dt} d={d}")
