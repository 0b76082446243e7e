"""CTC forced alignment: the Viterbi path of a known token sequence through CTC log-probs.

The reference aligns with `force_align` (utils/model_utils.py:103-117), which calls
torchaudio.functional.forced_align on the CPU, one utterance at a time.  torchaudio is not part of this
build, so the semantics are fixed here and parity with torchaudio is unpinned:

  states s = 0 .. 2L: blank at even s, y[s // 2] at odd s;
  alpha[0][0] = lp[0][blank], alpha[0][1] = lp[0][y[0]], the rest -inf;
  alpha[t][s] = max(stay alpha[t-1][s], step alpha[t-1][s-1], skip alpha[t-1][s-2]) + lp[t][label(s)],
  the skip only into an odd s >= 3 whose label differs from the one before; on exact ties the smallest
  jump wins (k = 0; if c1 > c[k]: k = 1; if c2 > c[k]: k = 2); a state whose chosen candidate is -inf
  stays -inf; the path ends in state 2L, or in 2L - 1 when that one is strictly better.
  alpha is f64, each log-prob converted exactly: host and device do the same IEEE operations in the
  same order, so paths and scores agree bit for bit.

Two implementations share that formulation:
  - device tensors: the trellis and backtrace kernels (csrc/ctc_align.hip), one workgroup per utterance
    of a packed batch;
  - CPU tensors: `force_align_host`, numpy f64 vectorised per frame (the subject of the CPU tests).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

STATUS_TEXT = {1: "no alignment exists (fewer frames than tokens plus adjacent repeats)",
               2: "a row or target range lies outside its array",
               3: "a target id is outside [0, V) or equal to the blank",
               4: "the end state is not finite (NaN / -inf log-probs)",
               5: "the workspace region or the device lengths do not match the plan"}
FRAME_SENTINEL = -7      # what align_packed_device_raw fills `frames` and `spans` with before the launch


class AlignResult:
    """One utterance's alignment: `frames` the label of every frame (what the reference's force_align
    returns), `tokens` the target, `spans` the (first, last) frame of each token's run (inclusive),
    `frame_logp` the log-prob of each frame's label, `score` the path's log-probability (f64)."""

    def __init__(self, frames: List[int], tokens: List[int], spans: List[Tuple[int, int]], frame_logp: List[float],
                 score: float):
        self.frames = frames
        self.tokens = tokens
        self.spans = spans
        self.frame_logp = frame_logp
        self.score = score

    def token_times(self, frame_s: float = 0.08) -> List[Tuple[float, float]]:
        """(start, end) of every token in seconds: 80 ms encoder frames (the frame of max_silence_frames),
        the end being the end of the token's last frame."""
        return [(a * frame_s, (b + 1) * frame_s) for a, b in self.spans]

    def words(self, char_dict: Dict[int, str], frame_s: float = 0.08) -> List[dict]:
        """Pieces merged into words: a piece that starts with "▁" opens a new word.
        -> [{"word", "start", "end"}] in seconds."""
        out: List[dict] = []
        for tok, (a, b) in zip(self.tokens, self.token_times(frame_s)):
            piece = char_dict[int(tok)]
            if piece.startswith("▁") or not out:
                out.append({"word": piece.lstrip("▁"), "start": a, "end": b})
            else:
                out[-1]["word"] += piece
                out[-1]["end"] = b
        return out

    def __eq__(self, other):
        return (isinstance(other, AlignResult) and self.frames == other.frames and self.tokens == other.tokens and
                self.spans == other.spans and self.frame_logp == other.frame_logp and self.score == other.score)

    def __repr__(self):
        return f"AlignResult(T={len(self.frames)}, L={len(self.tokens)}, score={self.score!r})"


def remove_duplicates_and_blank(frames: Sequence[int], blank_id: int = 0) -> List[int]:
    """utils/model_utils.py:23-32."""
    out, prev = [], None
    for f in frames:
        if f != prev and f != blank_id:
            out.append(int(f))
        prev = f
    return out


def _as_numpy(lp) -> np.ndarray:
    if isinstance(lp, torch.Tensor):
        lp = lp.detach().to("cpu", torch.float32).numpy()
    lp = np.ascontiguousarray(lp, dtype=np.float32)
    if lp.ndim != 2:
        raise ValueError("log-probs must be [T, V]")
    return lp


def _ids(y) -> List[int]:
    if isinstance(y, torch.Tensor):
        y = y.reshape(-1).tolist()
    return [int(v) for v in y]


def spans_of(frames: Sequence[int], states: Sequence[int], L: int) -> List[Tuple[int, int]]:
    first, last = [-1] * L, [-1] * L
    for t, s in enumerate(states):
        if s & 1:
            q = s >> 1
            if first[q] < 0:
                first[q] = t
            last[q] = t
    return list(zip(first, last))


def align_host_status(lp, y, blank_id: int = 0) -> Tuple[int, Optional[AlignResult]]:
    """The restatement with the kernel's status codes instead of exceptions: (status, result or None)."""
    lp = _as_numpy(lp)
    y = _ids(y)
    T, V = lp.shape
    L = len(y)
    blank = int(blank_id)
    if not 0 <= blank < V:
        raise ValueError(f"blank_id {blank} outside [0, {V})")
    if any(v < 0 or v >= V or v == blank for v in y):
        return 3, None
    R = sum(1 for i in range(1, L) if y[i] == y[i - 1])
    if T < L + R:
        return 1, None
    if T == 0:
        return 0, AlignResult([], [], [], [], 0.0)
    S = 2 * L + 1
    ya = np.asarray(y, dtype=np.int64)
    labels = np.full(S, blank, dtype=np.int64)
    labels[1::2] = ya
    skip = np.zeros(S, dtype=bool)
    if L > 1:
        skip[3::2] = ya[1:] != ya[:-1]
    ninf = -np.inf
    alpha = np.full(S, ninf, dtype=np.float64)
    alpha[0] = np.float64(lp[0, blank])
    if L:
        alpha[1] = np.float64(lp[0, y[0]])
    bp = np.zeros((T, S), dtype=np.uint8)
    c1 = np.empty(S, dtype=np.float64)
    c2 = np.empty(S, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, T):
            em = lp[t, labels].astype(np.float64)
            c1[0] = ninf
            c1[1:] = alpha[:-1]
            k1 = c1 > alpha
            best = np.where(k1, c1, alpha)
            c2[:2] = ninf
            c2[2:] = alpha[:-2]
            k2 = skip & (c2 > best)
            best = np.where(k2, c2, best)
            k = k1.astype(np.uint8)
            k[k2] = 2
            alpha = np.where(best == ninf, ninf, best + em)
            bp[t] = k
    end, score = S - 1, alpha[S - 1]
    if S > 1 and alpha[S - 2] > score:
        end, score = S - 2, alpha[S - 2]
    if not np.isfinite(score):
        return 4, None
    states = [0] * T
    s = end
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t:
            s = max(s - int(bp[t, s]), 0)
    frames = [int(labels[s]) for s in states]
    flp = lp[np.arange(T), np.asarray(frames, dtype=np.int64)].tolist()
    return 0, AlignResult(frames, list(y), spans_of(frames, states, L), flp, float(score))


def force_align_host(lp, y, blank_id: int = 0) -> AlignResult:
    """Forced alignment of target `y` to log-probs `lp` [T, V] on the host.  ValueError when the target
    holds the blank or an id outside the vocabulary, when no alignment exists, or when the log-probs
    leave no finite path."""
    st, res = align_host_status(lp, y, blank_id)
    if st:
        raise ValueError(f"forced alignment failed: {STATUS_TEXT[st]}")
    return res


def plan_workspace(row_len: Sequence[int], target_len: Sequence[int]) -> int:
    """Bytes of workspace cfm_ctc_align needs: 2-bit backpointers (4 bytes per frame and 16 states) and
    two alpha rows per utterance."""
    from . import _lib
    B = len(row_len)
    rl = (_lib.I32 * max(B, 1))(*[int(v) for v in row_len])
    tl = (_lib.I32 * max(B, 1))(*[int(v) for v in target_len])
    return int(_lib.cfm_ctc_align_plan(rl, tl, B, None))


def align_packed_device_raw(logp: torch.Tensor, row_start, row_len, targets: Sequence[Sequence[int]],
                            blank_id: int = 0, lds_max_states: int = -1, generic_strips: bool = False,
                            workspace_bytes: Optional[int] = None, max_workspace_bytes: Optional[int] = None):
    """One cfm_ctc_align call over packed device log-probs [rows, V]: utterance b = rows
    [row_start[b], row_start[b] + row_len[b]) aligned to targets[b].  Returns the device outputs as
    CPU tensors {frames [rows], frame_logp [rows], spans [n_targets, 2], score [B], status [B],
    target_start}: frames and spans are filled with FRAME_SENTINEL and frame_logp / score with NaN
    before the launch, so what the kernels did not write is recognisable.  `lds_max_states` /
    `generic_strips` choose the kernel paths and `workspace_bytes` overrides the workspace size (tests);
    `max_workspace_bytes` raises before anything is launched when the trellis needs more."""
    from . import _lib
    if logp.dim() != 2:
        raise ValueError("log-probs must be [rows, V]")
    dev = logp.device
    x = logp.to(torch.float32).contiguous()
    rows, V = x.shape
    B = len(row_start)
    if len(row_len) != B or len(targets) != B:
        raise ValueError("row_start, row_len and targets must have one entry per utterance")
    tg = [_ids(t) for t in targets]
    tl = [len(t) for t in tg]
    tstart = [0] * B
    for b in range(1, B):
        tstart[b] = tstart[b - 1] + tl[b - 1]
    n_t = sum(tl)
    flat = torch.tensor([v for t in tg for v in t] or [0], dtype=torch.int64)
    if int(flat.abs().max()) >= 1 << 31:
        raise ValueError("target ids must fit int32")
    rl_h = _lib.i32_host(list(row_len) or [0])
    tl_h = torch.tensor(tl or [0], dtype=torch.int32)
    rs_h = _lib.i32_host(list(row_start) or [0])
    ts_h = torch.tensor(tstart or [0], dtype=torch.int32)
    off_h = torch.zeros(max(B, 1), dtype=torch.int64)
    need = int(_lib.cfm_ctc_align_plan(rl_h.data_ptr(), tl_h.data_ptr(), B, off_h.data_ptr()))
    if max_workspace_bytes is not None and need > int(max_workspace_bytes):
        raise ValueError(f"forced alignment needs a {need}-byte trellis workspace ({need / 2 ** 20:.1f} MiB), more "
                         f"than max_workspace_bytes = {int(max_workspace_bytes)}")
    nbytes = need if workspace_bytes is None else int(workspace_bytes)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    frames = torch.full((max(rows, 1),), FRAME_SENTINEL, dtype=torch.int32, device=dev)
    flp = torch.full((max(rows, 1),), float("nan"), dtype=torch.float32, device=dev)
    spans = torch.full((max(n_t, 1), 2), FRAME_SENTINEL, dtype=torch.int32, device=dev)
    score = torch.full((max(B, 1),), float("nan"), dtype=torch.float64, device=dev)
    status = torch.full((max(B, 1),), -1, dtype=torch.int32, device=dev)
    d = [t.to(dev) for t in (rs_h, rl_h, flat.to(torch.int32), ts_h, tl_h, off_h)]
    with torch.cuda.device(dev):
        _lib.check(_lib.cfm_ctc_align(x.data_ptr(), rows, V, d[0].data_ptr(), d[1].data_ptr(), B, int(blank_id),
                                      d[2].data_ptr(), n_t, d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
                                      rl_h.data_ptr(), tl_h.data_ptr(), frames.data_ptr(), flp.data_ptr(),
                                      spans.data_ptr(), score.data_ptr(), status.data_ptr(), int(lds_max_states),
                                      _lib.CFM_ALIGN_GENERIC_STRIPS if generic_strips else 0, ws.data_ptr(), nbytes,
                                      torch.cuda.current_stream(dev).cuda_stream))
    return {"frames": frames.cpu()[:rows], "frame_logp": flp.cpu()[:rows], "spans": spans.cpu()[:n_t],
            "score": score.cpu()[:B], "status": status.cpu()[:B], "target_start": tstart, "targets": tg,
            "workspace_bytes": need}


def results_from_raw(raw, row_start, row_len) -> List[Optional[AlignResult]]:
    """Per utterance the AlignResult of a raw device result, None where its status is not 0."""
    out: List[Optional[AlignResult]] = []
    fr, fl, sp, sc = raw["frames"].tolist(), raw["frame_logp"].tolist(), raw["spans"].tolist(), raw["score"].tolist()
    for b, st in enumerate(raw["status"].tolist()):
        if st != 0:
            out.append(None)
            continue
        s0, n, t0, tg = int(row_start[b]), int(row_len[b]), raw["target_start"][b], raw["targets"][b]
        out.append(AlignResult(fr[s0:s0 + n], list(tg), [tuple(p) for p in sp[t0:t0 + len(tg)]], fl[s0:s0 + n],
                               sc[b]))
    return out


def raise_failed(status: Sequence[int]) -> None:
    """ValueError naming the utterances whose status is not 0."""
    bad = [(b, st) for b, st in enumerate(status) if st != 0]
    if bad:
        what = "; ".join(f"utterance {b}: {STATUS_TEXT.get(st, f'status {st}')}" for b, st in bad)
        raise ValueError(f"forced alignment failed for utterance(s) {[b for b, _ in bad]}: {what}")


def align_packed(logp: torch.Tensor, row_start, row_len, targets: Sequence[Sequence[int]], blank_id: int = 0,
                 max_workspace_bytes: Optional[int] = None, return_status: bool = False):
    """Forced alignment of a packed batch: log-probs [rows, V], utterance b = rows
    [row_start[b], row_start[b] + row_len[b]) aligned to the token ids targets[b].  Device tensors run
    the HIP kernels (one launch pair for the batch), CPU tensors the host restatement.  ValueError,
    naming the utterance indices, when a target holds the blank or an id outside the vocabulary, when
    an utterance has no alignment or no finite path -- raised after the others have been computed.
    `return_status`: no exception for those; returns (results with None for them, status per utterance)."""
    from . import _lib
    B = len(row_start)
    rows = logp.shape[0]
    rs, rl = (t.tolist() for t in _lib.packed_ranges(row_start, row_len, rows, "log-prob tensor"))
    if B == 0:
        return ([], []) if return_status else []
    if logp.is_cuda:
        raw = align_packed_device_raw(logp, rs, rl, targets, blank_id, max_workspace_bytes=max_workspace_bytes)
        status, res = raw["status"].tolist(), results_from_raw(raw, rs, rl)
    else:
        lp = _as_numpy(logp)
        pairs = [align_host_status(lp[s:s + n], y, blank_id) for s, n, y in zip(rs, rl, targets)]
        status, res = [st for st, _ in pairs], [r for _, r in pairs]
    if return_status:
        return res, status
    raise_failed(status)
    return res


def force_align(ctc_probs: torch.Tensor, y, blank_id: int = 0) -> List[int]:
    """The reference's signature (utils/model_utils.py:103): ctc_probs [T, V] log-probs, y [L] token ids
    -> the label of every frame.  A device tensor runs the HIP kernels, a CPU tensor the host."""
    if ctc_probs.dim() != 2:
        raise ValueError("ctc_probs must be [T, V]")
    return align_packed(ctc_probs, [0], [ctc_probs.shape[0]], [_ids(y)], blank_id)[0].frames
