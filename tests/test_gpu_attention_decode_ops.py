"""Kernel-level parity of the attention decoding mode's attention kernels (cfm_op_decode_attention, include/cfm_ops.h;
csrc/attdec.hip), each selected explicitly -- a shape the selected kernel does not take is an error, never another
kernel -- against a float64 reference of the operator computed here:

  self-gather    one query per (row, head) over n_keys cached positions read through a shuffled ancestry table
                 (cached lengths 1, 32, 33, 65; positions past n_keys hold NaN and must not be read);
  cross-generic  the beams of an utterance over its encoder rows, key counts 0, 1, 31, 32, 33, 65, 200 in one call at
  cross-mfma     unaligned row offsets (NaN between them), beams 1, 3, 10, 16, key splits 1, 2, 3 (three parts of one key
                 or of none leave empty parts).

Bars, those of test_gpu_rescore_ops.py for the matching kernel kinds: max|out - ref| / max|ref| <= 1e-4 in fp32; in the
16-bit types 4 x E_round(dtype), E_round the rounding a correct kernel must incur, measured there on the CPU (bf16
2.42e-3, fp16 3.35e-4; the generic kernels round only inputs and output, the MFMA kernel also the probabilities).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 2
E_ROUND = {"bf16": 2.42e-3, "fp16": 3.35e-4}
BAR = {"fp32": 1e-4, "bf16": 4 * E_ROUND["bf16"], "fp16": 4 * E_ROUND["fp16"]}
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
KEYS = (0, 1, 31, 32, 33, 65, 200)
BEAMS = (1, 3, 10, 16)
SPLITS = (1, 2, 3)
CACHED = (1, 32, 33, 65)
GUARD = 4
SQ = 1.5      # scale of q: scores with a standard deviation of about 1.5, as in seg_attention_cases.py


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chunkformer_amd import _lib
    return _lib


def _code(L, dt):
    return {"fp32": L.DTYPE_F32, "bf16": L.DTYPE_BF16, "fp16": L.DTYPE_F16}[dt]


def _softmax_av(q, k, v, dk):
    """q [n, dk], k / v [m, dk] float64 -> [n, dk]; no key: zeros"""
    if k.shape[0] == 0:
        return torch.zeros(q.shape[0], dk, dtype=torch.float64)
    return torch.softmax(q @ k.T / dk ** 0.5, dim=-1) @ v


@functools.lru_cache(maxsize=None)
def cross_case(dt, dk, beam):
    d, B = H * dk, len(KEYS)
    gen = torch.Generator().manual_seed(2000 + dk + beam)
    starts, pos = [], 3
    for nk in KEYS:
        starts.append(pos)
        pos += nk + 1 + nk % 3
    kv = torch.randn(pos + 2, 2 * d, generator=gen)
    covered = torch.zeros(pos + 2, dtype=torch.bool)
    for s, nk in zip(starts, KEYS):
        covered[s: s + nk] = True
    kv[~covered] = float("nan")
    q = (SQ * torch.randn(B * beam, d, generator=gen)).to(TDT[dt])
    kv = kv.to(TDT[dt])
    ref = torch.zeros(B * beam, d, dtype=torch.float64)
    for u, (s, nk) in enumerate(zip(starts, KEYS)):
        for h in range(H):
            c = slice(h * dk, (h + 1) * dk)
            ref[u * beam: (u + 1) * beam, c] = _softmax_av(q[u * beam: (u + 1) * beam, c].double(), kv[s: s + nk, c].double(),
                                                           kv[s: s + nk, d + h * dk: d + (h + 1) * dk].double(), dk)
    return q, kv, starts, ref


def _run_cross(L, dt, dk, beam, kernel, n_split):
    q, kv, starts, ref = cross_case(dt, dk, beam)
    d, B, R = H * dk, len(KEYS), len(KEYS) * beam
    dev = "cuda"
    out = torch.full((R + GUARD, d), float("nan"), dtype=TDT[dt], device=dev)
    scratch = torch.full((n_split * R * (d + 2 * H) + 8,), float("nan"), dtype=torch.float32, device=dev)
    us = torch.tensor(starts, dtype=torch.int32, device=dev)
    ul = torch.tensor(KEYS, dtype=torch.int32, device=dev)
    qd, kvd = q.to(dev), kv.to(dev)
    rc = L.cfm_op_decode_attention(_code(L, dt), kernel, qd.data_ptr(), out.data_ptr(), B, beam, H, dk, kvd.data_ptr(),
                                   kv.shape[0], 0, 0, 0, us.data_ptr(), ul.data_ptr(), n_split, scratch.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu(), ref


def _check_cross(L, dt, dk, kernel, what):
    worst = 0.0
    for beam in BEAMS:
        for n_split in SPLITS:
            rc, out, ref = _run_cross(L, dt, dk, beam, kernel, n_split)
            L.check(rc)
            R = len(KEYS) * beam
            assert torch.isnan(out[R:].float()).all(), "guard rows after the last row were written"
            o = out[:R].double()
            assert torch.isfinite(o).all(), "non-finite output (a NaN row was read)"
            assert (o[:beam] == 0).all(), "an utterance without rows must give exactly 0"
            err = ((o - ref).abs().max() / ref.abs().max()).item()
            assert err <= BAR[dt], f"beam {beam} split {n_split}: max|out - ref| / max|ref| = {err:.3e} > {BAR[dt]:.2e}"
            worst = max(worst, err)
    print(f"decode-attention {what} {dt} dk={dk}: worst err {worst:.3e} = {worst / BAR[dt]:.3f} of the bar {BAR[dt]:.2e}")


@pytest.mark.parametrize("dk", [16, 64, 128])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_cross_generic_kernel(L, dt, dk):
    _check_cross(L, dt, dk, L.DEC_ATTN_CROSS_GENERIC, "cross-generic")


@pytest.mark.parametrize("dk", [64, 128])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_cross_mfma_kernel(L, dt, dk):
    _check_cross(L, dt, dk, L.DEC_ATTN_CROSS_MFMA, "cross-mfma")


@pytest.mark.parametrize("dk", [16, 64, 128])
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_self_gather_kernel(L, dt, dk):
    d, dev = H * dk, "cuda"
    worst = 0.0
    for beam in BEAMS:
        B = 3
        R, n_pos = B * beam, max(CACHED)
        gen = torch.Generator().manual_seed(3000 + dk + beam)
        q = (SQ * torch.randn(R, d, generator=gen)).to(TDT[dt])
        kv_all = torch.randn(n_pos, R, 2 * d, generator=gen).to(TDT[dt])
        anc = torch.randint(0, R, (R, n_pos + 3), generator=gen, dtype=torch.int32)   # any row: a shuffled table
        for n_keys in CACHED:
            kv = kv_all.clone()
            kv[n_keys:] = float("nan")                     # positions past the cached length must not be read
            ref = torch.zeros(R, d, dtype=torch.float64)
            for r in range(R):
                slots = anc[r, : n_keys - 1].long().tolist() + [r]
                rows = kv[torch.arange(n_keys), torch.tensor(slots)].double()      # [n_keys, 2d]
                for h in range(H):
                    c = slice(h * dk, (h + 1) * dk)
                    ref[r, c] = _softmax_av(q[r: r + 1, c].double(), rows[:, c], rows[:, d + h * dk: d + (h + 1) * dk], dk)[0]
            out = torch.full((R + GUARD, d), float("nan"), dtype=TDT[dt], device=dev)
            qd, kvd, ad = q.to(dev), kv.to(dev), anc.to(dev)
            rc = L.cfm_op_decode_attention(_code(L, dt), L.DEC_ATTN_SELF_GATHER, qd.data_ptr(), out.data_ptr(), B, beam, H, dk,
                                           kvd.data_ptr(), n_pos, ad.data_ptr(), anc.shape[1], n_keys, 0, 0, 1, 0,
                                           torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            L.check(rc)
            o = out.cpu()
            assert torch.isnan(o[R:].float()).all() and torch.isfinite(o[:R].float()).all()
            err = ((o[:R].double() - ref).abs().max() / ref.abs().max()).item()
            assert err <= BAR[dt], f"beam {beam} n_keys {n_keys}: {err:.3e} > {BAR[dt]:.2e}"
            if n_keys == 1:     # one key: the output is that key's value row (p = 1, l = 1: one rounding at most)
                one = (o[:R].double() - kv[0, :, d:].double()).abs().max().item()
                assert one <= 2.0 ** -22 * kv[0, :, d:].abs().max().item(), one
            worst = max(worst, err)
    print(f"decode-attention self-gather {dt} dk={dk}: worst err {worst:.3e} = {worst / BAR[dt]:.3f} of the bar {BAR[dt]:.2e}")


def test_kernels_refuse_what_they_do_not_take(L):
    for dt, dk in (("fp32", 64), ("bf16", 16)):
        rc, out, _ = _run_cross(L, dt, dk, 3, L.DEC_ATTN_CROSS_MFMA, 1)
        assert rc == L.CFM_ERR_ASSERT, f"status {rc}: the MFMA kernel must refuse this shape, not run or fall back"
        with pytest.raises(AssertionError, match="cross-mfma"):
            L.check(rc)
        assert torch.isnan(out.float()).all(), "a refused call wrote to out"


def test_mfma_matches_generic(L):
    for dt in ("bf16", "fp16"):
        for dk in (64, 128):
            _, a, ref = _run_cross(L, dt, dk, 10, L.DEC_ATTN_CROSS_GENERIC, 2)
            _, b, _ = _run_cross(L, dt, dk, 10, L.DEC_ATTN_CROSS_MFMA, 2)
            R = len(KEYS) * 10
            diff = ((a[:R].double() - b[:R].double()).abs().max() / ref.abs().max()).item()
            assert diff <= BAR[dt], (dt, dk, diff)
