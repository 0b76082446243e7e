"""ORACLE — test infrastructure only.  Float64 reference of the projection GEMM *operator* (cfm_op_gemm,
include/cfm_ops.h), written from the contract alone, with a per-element error bar derived below.  It runs on whatever
device its inputs live on and shares no code with the kernels.

Inputs are taken exactly as stored in the operand type (A [M, K], W [N, K] in f32 / bf16 / f16; bias, x f32):

    z = A . W^T + bias                  S = |A| . |W|^T + |bias|           (both float64, [M, N])
    STORE      y = act(z)               act 0 none, 1 ReLU, 2 SiLU z / (1 + e^-z), 3 prescaled SiLU z / (1 + 2^z)
    STORE_F32  y = alpha z              (f32 output)
    RESID      y = x + alpha rowmask z  (f32 output)
    QKV        y = z, [M, 3 d]; qkv_split() maps it to q [M, d] and the K | V stream [M, 2 d]:
               K / V column cc of head cc // dk goes to (cc // dk) * 2 dk + {0, dk} + cc % dk
    GLU        W rows (and bias) interleaved [a16 | gate16] per 32 columns: y[:, 16 b + i] = a * sigmoid(gate)
               (act 0) or a / (1 + 2^gate) (act 3, the gate half prescaled by -log2 e); [M, N / 2]

The bar (pass criterion |out - y| <= bar on EVERY element), u = 2^-24:

  Accumulation  e_acc = K * 2^-23 * S.  A correct kernel forms z from K products and K additions (K - 1 between the
                products, one for the bias: first, as the accumulator's seed, or last) in f32, in any order.  With
                16-bit operands every product is exact in f32 (8 + 8 or 11 + 11 significant bits); with f32 operands
                it is rounded once, or fused into the addition.  That is at most 2 K rounding errors when every
                operation rounds to nearest, each at most u = 2^-24 of an intermediate that S bounds in magnitude
                (up to a factor 1 + O(K u), K u < 3e-4 here): 2 K u S = K 2^-23 S.  A kernel whose adder truncates
                (error up to 2^-23 per addition) stays inside the same bound when its products are exact, the 16-bit
                case: K additions of 2^-23 S each.  Nothing is assumed about the order.
  Epilogue      the accumulation error through the epilogue, by the mean value theorem with global derivative bounds:
                none / ReLU 1; both SiLU forms max |silu'| = 1.0998 < 1.1 (z / (1 + 2^z) is -silu(-z ln 2) / ln 2:
                the same derivative); STORE_F32 |alpha|; RESID |alpha| rowmask; GLU y = a s(g), |s'| <= 1/4:
                e_a (s + e_g / 4) + |a| e_g / 4.
  exp2 / rcp    the kernels evaluate the sigmoid as rcp(1 + exp2(t)) with t = -log2(e) * z formed in f32 (two roundings:
                |t| 2^-23, which exp2 turns into a relative ln 2 |t| 2^-23 <= |z| 2^-23), v_exp_f32 and v_rcp_f32 at one
                ulp each (2^-23), the add and the final multiply at half an ulp each: relative (|z| + 3) 2^-23 of the
                result, taken as (|z| + 4) 2^-23; the prescaled forms have no t rounding: 4 * 2^-23.
  Output        one rounding to the output type at magnitude |y| + e: half an ulp, at most 2^-p (|y| + e) with p = 8
                (bf16), 11 (f16; never below half the subnormal spacing, 2^-25), 24 (f32).  STORE_F32's one rounding is
                the product with alpha.  RESID rounds twice in f32: the product with alpha (exact when the compiler
                fuses it into the add) and the sum with x (csrc/gemm.hip `*xp + ep.alpha * v * m`, gemm_bf16_epi.h
                `*xp + (alpha mk) * acc`).
"""
from types import SimpleNamespace

import torch

STORE, STORE_F32, RESID, QKV, GLU = 0, 1, 2, 3, 4
U23 = 2.0 ** -23
PREC = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}
FLOOR = {torch.float32: 2.0 ** -150, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}


def half_ulp(v, dt):
    """bound on the round-to-nearest error of a value of magnitude <= v in type dt"""
    return (v * 2.0 ** -PREC[dt]).clamp_min(FLOOR[dt])


def act_ref(z, act):
    if act == 1:
        return z.clamp_min(0.0)
    if act == 2:
        return z / (1.0 + torch.exp(-z))
    if act == 3:
        return z / (1.0 + torch.exp2(z))
    return z


def glu_halves(t):
    """[M, N] in [a16 | gate16] blocks -> (a, gate), each [M, N / 2]"""
    v = t.reshape(t.shape[0], -1, 2, 16)
    return v[:, :, 0].reshape(t.shape[0], -1), v[:, :, 1].reshape(t.shape[0], -1)


def kv_cols(d, dk, device=None):
    """K | V stream column of [K (d) | V (d)] column c, as an index tensor [2 d]"""
    c = torch.arange(2 * d, device=device)
    which, cc = c // d, c % d
    return (cc // dk) * 2 * dk + which * dk + cc % dk


def qkv_split(y, d, dk):
    """y [M, 3 d] in projection order -> (q [M, d], kv [M, 2 d] in K | V stream order)"""
    kv = torch.empty_like(y[:, d:])
    kv[:, kv_cols(d, dk, y.device)] = y[:, d:]
    return y[:, :d], kv


def gemm_op_ref(A, W, bias, epi, act=0, alpha=1.0, x=None, rowmask=None):
    """-> z, S, y, bar (float64) and out_dtype; see the module docstring.  A, W in the operand type."""
    dt = A.dtype
    M, K = A.shape
    a64, w64 = A.double(), W.double()
    z = a64 @ w64.t()
    S = a64.abs() @ w64.abs().t()
    if bias is not None:
        z = z + bias.double()
        S = S + bias.double().abs()
    e_acc = K * U23 * S
    out_dt = torch.float32 if epi in (STORE_F32, RESID) else dt
    if epi == STORE or epi == QKV:
        a = act if epi == STORE else 0
        y = act_ref(z, a)
        e = e_acc * (1.1 if a >= 2 else 1.0)
        if a == 2:
            e = e + y.abs() * (z.abs() + 4.0) * U23
        if a == 3:
            e = e + y.abs() * 4.0 * U23
        bar = e + half_ulp(y.abs() + e, out_dt)
    elif epi == STORE_F32:
        y = alpha * z
        e = abs(alpha) * e_acc
        bar = e + half_ulp(y.abs() + e, out_dt)
    elif epi == RESID:
        m = rowmask.double()[:, None] if rowmask is not None else 1.0
        t = alpha * m * z
        y = x.double() + t
        e = abs(alpha) * m * e_acc
        e = e + half_ulp(t.abs() + e, out_dt)
        bar = e + half_ulp(y.abs() + e, out_dt)
    elif epi == GLU:
        (za, zg), (ea, eg) = glu_halves(z), glu_halves(e_acc)
        s = 1.0 / (1.0 + (torch.exp2(zg) if act == 3 else torch.exp(-zg)))
        y = za * s
        e = ea * (s + 0.25 * eg) + za.abs() * 0.25 * eg
        e = e + y.abs() * ((4.0 if act == 3 else zg.abs() + 4.0) * U23)
        bar = e + half_ulp(y.abs() + e, out_dt)
    else:
        raise ValueError(f"unknown epilogue {epi}")
    return SimpleNamespace(z=z, S=S, y=y, bar=bar, out_dtype=out_dt)
