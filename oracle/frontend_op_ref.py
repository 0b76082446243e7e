"""ORACLE — test infrastructure only.  Float64 CPU references of the front-end operators of include/cfm_ops.h
(cfm_op_frontend_conv0_dw, cfm_op_frontend_dw2), written from the operator contracts alone, with strided slices
instead of conv2d: no code is shared with the kernels or with oracle/encoder_ref.py.

emulate=<16-bit dtype> rounds exactly where a correct kernel of that type must round and nowhere else; it sizes
the tests' tolerance (E_round) and is never compared with a kernel.  The rounding points, per kernel:

  conv0 + ReLU + dw1 (csrc/frontend.hip)
    "valu"  fe_conv0_dw_kernel: f32 throughout (frontend.hip:86, 100); rounded: `out` alone (frontend.hip:101).
            An fp32 model rounds nothing.
    "pos"   fe_conv0_dw_mfma_kernel: the input after padding and CMVN (frontend.hip:168-170), w0 and b0
            (frontend.hip:209: the MFMA's 16-bit B operand; b0 multiplies the 1.0 of k = 9) are rounded; conv0
            accumulates in f32 and stays f32 through the ReLU; w1 and b1 stay f32 (frontend.hip:210, 214, 228);
            `out` is rounded (frontend.hip:236).
    "ch"    fe_conv0_dw_mfma2_kernel: the input (frontend.hip:415-422, the im2col rows), w0 and b0 (host-packed
            fragments, csrc/model.hip:643; the bf16 2^-24 scale is a power of two and changes no rounding), the
            post-ReLU conv0 value (frontend.hip:475-476: the second MFMA's 16-bit operand) and w1 (model.hip:651, x 2^24)
            are rounded; b1 stays f32 (model.hip:655: the accumulator seed); `out` is rounded (frontend.hip:496-497).
  pw1 + ReLU (the GEMM epilogue, csrc/gemm_bf16_epi.h / gemm_wst_impl.h): the operands arrive in the type; the
            output is rounded after the ReLU.
  dw2       fe_dw2_kernel and the fused epilogue share dw2_dot / dw2_wpack (csrc/cfm_common.h:113-127): the 9 taps
            are rounded to the type, the products accumulate in f32 on the f32 bias; `out` is rounded
            (frontend.hip:563).
"""
import torch

F0, F1, F2, F3 = 80, 39, 19, 9


def _rnd(emulate):
    return (lambda t: t.to(emulate).double()) if emulate is not None else (lambda t: t)


def sub_len(n):
    return (n - 3) // 2 + 1


def windows(feats, row0, nvalid, W, mean=None, istd=None, cmvn_before_padding=False):
    """[nwin, W, 80] float64: window n = rows row0[n] .. of `feats`, rows at or past nvalid[n] zero padding, then
    CMVN (after the padding: padding rows become -mean * istd).  Source rows past nvalid are never touched.
    cmvn_before_padding: the wrong order (a mutation for the tolerance guard)."""
    x = torch.zeros(len(row0), W, F0, dtype=torch.float64)
    cm = (lambda t: (t - mean.double()) * istd.double()) if mean is not None else (lambda t: t)
    for n, (r, nv) in enumerate(zip(row0, nvalid)):
        nv = max(0, min(int(nv), W))
        src = feats[r: r + nv].double()
        x[n, :nv] = cm(src) if cmvn_before_padding else src
    return x if cmvn_before_padding else cm(x)


def _strided3x3(x, w, b):
    """channels-last depthwise-style 3x3 stride-2 valid conv: x [n, T, F, C or 1], w [C, 3, 3], b [C] or None"""
    T, F = sub_len(x.shape[1]), sub_len(x.shape[2])
    out = 0.0
    for u in range(3):
        for v in range(3):
            out = out + x[:, u: u + 2 * T - 1: 2, v: v + 2 * F - 1: 2, :] * w[:, u, v]
    return out if b is None else out + b


def conv0_dw_op_ref(x, w0, b0, w1, b1, emulate=None, kernel="valu", relu=True):
    """x [nwin, W, 80] (padded, CMVN applied) -> [nwin, T2, 19, d] float64.  w0, w1 [d, 3, 3]."""
    rnd = _rnd(emulate)
    r_in = rnd if kernel in ("pos", "ch") else (lambda t: t)
    r_mid = rnd if kernel == "ch" else (lambda t: t)
    c0 = _strided3x3(r_in(x.double()).unsqueeze(-1), r_in(w0.double()), r_in(b0.double()))      # [n, T1, 39, d]
    if relu:
        c0 = c0.clamp_min(0.0)
    return rnd(_strided3x3(r_mid(c0), r_mid(w1.double()), b1.double()))


def pw1_relu_ref(a, w, b, emulate=None):
    """a [..., d] (the dw1 output, in the type), w [d, d] (in the type), b [d] f32 -> relu(a . w^T + b), rounded"""
    return _rnd(emulate)((a.double() @ w.double().t() + b.double()).clamp_min(0.0))


def dw2_op_ref(z, w2, b2, emulate=None, pitch=None, phase=0):
    """z [nwin, T2, 19, d] (the pw1 output) -> [nwin, T3, 9, d] float64; w2 [d, 3, 3].
    pitch / phase: mutations for the tolerance guard -- window n starts at row n * pitch of the flattened rows
    instead of n * T2; the stride-2 walk over the rows starts at row `phase`."""
    rnd = _rnd(emulate)
    nwin, T2 = z.shape[0], z.shape[1]
    T3 = sub_len(T2)
    z = z.double()
    if pitch is not None or phase:
        flat = z.reshape(nwin * T2, F2, -1)
        rows = torch.arange(nwin)[:, None] * (pitch or T2) + phase + torch.arange(2 * T3 + 1)[None, :]
        z = flat[rows]
    return rnd(_strided3x3(z[:, : 2 * T3 + 1], rnd(w2.double()), b2.double()))
