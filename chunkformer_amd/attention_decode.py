"""The `attention` decoding mode: autoregressive beam search over the checkpoint's left attention decoder.

The reference's `attention_beam_search` (modules/search.py:252-355) on a batch of ONE utterance, beam size N
(DESIGN §9e holds the semantics and the note on what the reference needs to run this mode at all):

    start   N hypotheses [sos], scores [0, -inf, ...]
    step i = 1 .. limit: the length-i prefixes through the left decoder (positions 0 .. i-1), log_softmax of the
            last row; per row the top N log-probs (a finished beam -- last token eos -- contributes the one
            candidate (score + 0, eos)); the top N of the N * N candidates by (value descending, candidate index
            ascending); every new hypothesis is its parent plus the chosen token
    stop    when all N beams are finished, or after step `limit` = the utterance's encoder row count, or
            `max_len` when given
    end     score / (count of tokens != eos over the whole row, sos included) ** length_penalty; the first
            maximum wins (a NaN is the maximum, as torch.max has it); its tokens without sos and eos

Every utterance stops at its OWN limit: the result does not depend on what else is in the batch (the reference,
given a padded batch, would keep stepping the short utterances up to the longest one's length).

Two implementations:
  - device: AttentionDecoder over the cfm_aed handle of an AttentionRescorer (one handle, one copy of the
    weights): cfm_attdec_begin / _steps / _finish (csrc/attdec.hip), all utterances of the masked batch at once.
    The host loop enqueues POLL_STEPS steps per call and then reads the device word that counts the running
    utterances;
  - CPU tensors: `attention_beam_search_host`, a torch restatement on rescore.decoder_logp_padded (teacher-forced,
    no cache) in f32 or f64: the checker of the tests, and what runs when the encoder rows are on the CPU.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import rescore as R
from .search import DecodeResult

MAX_BEAM = 16
POLL_STEPS = 8     # decode steps enqueued between two reads of the running-utterance count (one host sync each)
_STATUS = {2: "an utterance's row range lies outside the encoder rows",
           5: "an utterance's step limit lies outside [0, max_steps]"}


def sharpened_decoder_state_dict(c: R.AEDConfig, seed: int, scale: float, eos_offset: float):
    """rescore.synthetic_decoder_state_dict with the left decoder's output layer (weight and bias) scaled by
    `scale` and `eos_offset` added to the eos bias.  The plain synthetic head is nearly flat (every token costs
    about log(1 / V), so a search ends after 0-1 tokens); a sharper head gives searches that run, and the eos
    offset moves where they end.  The recipe of tests/golden/attention.npz and tools/bench_attention_decode.py."""
    sd = R.synthetic_decoder_state_dict(c, seed)
    p = R.LEFT if c.bidirectional else "decoder."
    sd[p + "output_layer.weight"] = (sd[p + "output_layer.weight"] * float(scale)).contiguous()
    b = sd[p + "output_layer.bias"] * float(scale)
    b[c.eos] += float(eos_offset)
    sd[p + "output_layer.bias"] = b.contiguous()
    return sd


def step_limits(row_len: Sequence[int], max_len: Optional[int]) -> List[int]:
    """Per utterance: `max_len` when given (the reference's decode_maxlen), else its encoder row count."""
    if max_len is not None and int(max_len) < 0:
        raise ValueError("max_len must not be negative")
    lim = [int(max_len) if max_len is not None else int(n) for n in row_len]
    for n in lim:
        if n > R.MAX_POSITIONS:
            raise ValueError(f"an utterance would decode up to {n} steps, more than the decoder's {R.MAX_POSITIONS} "
                             "positions: pass max_len")
    return lim


def _check_beam(c: R.AEDConfig, beam_size: int) -> int:
    n = int(beam_size)
    if n < 1 or n > MAX_BEAM or n > c.vocab:
        raise ValueError(f"beam_size {beam_size}: 1 .. {MAX_BEAM}, at most the vocabulary")
    return n


def _first_max(vals: Sequence[float]) -> int:
    """torch.max's index: the first maximum, a NaN being the maximum."""
    best = 0
    for k in range(1, len(vals)):
        if vals[best] != vals[best]:
            break
        if vals[k] != vals[k] or vals[k] > vals[best]:
            best = k
    return best


def _rank(vals: Sequence[float]) -> List[int]:
    """Final-score order: NaN first (the maximum), then descending, ties in beam order."""
    return sorted(range(len(vals)), key=lambda k: (0, 0.0) if vals[k] != vals[k] else (1, -vals[k]))


def _result(c: R.AEDConfig, rows: Sequence[Sequence[int]], finals: Sequence[float], trace=None) -> DecodeResult:
    """rows: the N final hypotheses after the sos (eos tokens included)."""
    strip = lambda h: [int(t) for t in h if int(t) != c.eos]   # noqa: E731
    best = _first_max(finals)
    order = _rank(finals)
    r = DecodeResult(strip(rows[best]), float(finals[best]), nbest=[strip(rows[k]) for k in order],
                     nbest_scores=[float(finals[k]) for k in order])
    r.best_index = best
    r.beam_scores = [float(v) for v in finals]       # in beam order
    r.beam_rows = [[int(t) for t in h] for h in rows]
    r.steps = len(rows[0]) if rows else 0
    r.trace = trace
    return r


# ------------------------------------------------------------------------------------ host restatement
@dataclass
class HostSearch:
    """One utterance's search state on the CPU; `step()` is one decode step whatever the state (the stop rules
    are `run`'s), so that the tests can step past the end."""
    cfg: R.AEDConfig
    W: Dict[str, torch.Tensor]
    pe: torch.Tensor
    mem: torch.Tensor
    beam: int
    dtype: torch.dtype = torch.float32
    hyps: List[List[int]] = field(default_factory=list)
    scores: Optional[torch.Tensor] = None
    fin: List[bool] = field(default_factory=list)
    trace: List[Tuple[List[int], List[int], List[float]]] = field(default_factory=list)
    margin: float = math.inf
    step_margins: List[float] = field(default_factory=list)   # per step: the gap its prune decided by (inf: none)

    def __post_init__(self):
        n = self.beam
        self.hyps = [[self.cfg.sos] for _ in range(n)]
        self.scores = torch.tensor([0.0] + [-math.inf] * (n - 1), dtype=self.dtype)
        self.fin = [False] * n

    def last_logp(self, hyps: Sequence[Sequence[int]]) -> torch.Tensor:
        c = self.cfg
        ys = torch.tensor([list(h) for h in hyps], dtype=torch.long)
        lp = R.decoder_logp_padded(self.W, R.LEFT, c, c.num_blocks, ys, [ys.shape[1]] * ys.shape[0], self.mem, self.pe)
        return lp[:, -1]

    def candidates(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """[N, N] candidate values and tokens of the next step, and the [N] values of every row's (N+1)-th token
        (-inf for a finished row, or when the vocabulary has no more tokens): the best candidates the first prune
        drops."""
        c, n = self.cfg, self.beam
        v, i = torch.sort(self.last_logp(self.hyps), dim=-1, descending=True, stable=True)
        nxt = v[:, n].clone() if v.shape[1] > n else torch.full((n,), -math.inf, dtype=v.dtype)
        v, i = v[:, :n].clone(), i[:, :n].clone()
        for b in range(n):
            if self.fin[b]:
                v[b, 0], v[b, 1:] = 0.0, -math.inf
                i[b] = c.eos
                nxt[b] = -math.inf
        return self.scores.unsqueeze(1) + v, i, self.scores + nxt

    def step(self) -> None:
        n = self.beam
        val, tok, nxt = self.candidates()
        flat = val.reshape(-1)
        sv, si = torch.sort(flat, descending=True, stable=True)
        rest = torch.cat([sv[n:], nxt])
        rest = rest[torch.isfinite(rest)]
        gap = math.inf
        if rest.numel() > 0 and math.isfinite(float(sv[n - 1])):
            gap = float(sv[n - 1] - rest.max())
        self.step_margins.append(gap)
        self.margin = min(self.margin, gap)
        sel = si[:n].tolist()
        parents = [k // n for k in sel]
        toks = [int(tok.reshape(-1)[k]) for k in sel]
        self.hyps = [self.hyps[p] + [t] for p, t in zip(parents, toks)]
        self.scores = sv[:n].clone()
        self.fin = [t == self.cfg.eos for t in toks]
        self.trace.append((parents, toks, [float(x) for x in self.scores.tolist()]))

    def run(self, limit: int) -> None:
        for _ in range(int(limit)):
            if all(self.fin):
                break
            self.step()

    def finals(self, length_penalty: float) -> List[float]:
        """search.py:340-342: score / lengths.pow(length_penalty), lengths = tokens != eos of the whole row."""
        cnt = torch.tensor([sum(1 for t in h if t != self.cfg.eos) for h in self.hyps], dtype=self.dtype)
        return [float(x) for x in (self.scores / cnt.pow(length_penalty)).tolist()]

    def result(self, length_penalty: float) -> DecodeResult:
        f = self.finals(length_penalty)
        r = _result(self.cfg, [h[1:] for h in self.hyps], f, list(self.trace))
        margin = self.margin
        if len(f) > 1:
            top = sorted((x for x in f if x == x and x != -math.inf), reverse=True)
            if len(top) > 1:
                margin = min(margin, top[0] - top[1])
        r.margin = margin
        r.step_margins = list(self.step_margins)
        return r


def attention_beam_search_host(cfg: R.AEDConfig, sd: Dict[str, torch.Tensor], enc_rows: torch.Tensor, row_start,
                               row_len, beam_size: int = 10, length_penalty: float = 0.0,
                               max_len: Optional[int] = None, dtype=torch.float32) -> List[DecodeResult]:
    """The search on the CPU, utterance b = rows [row_start[b], + row_len[b]) of enc_rows [rows, d].  Every
    DecodeResult carries, beyond tokens / score / nbest / nbest_scores (final-score order): `trace` (per step the
    (parent, token, score) lists of the N kept beams), `margin` (the decision margin: the minimum over the steps of
    the gap between the N-th and the (N+1)-th finite candidate -- the candidates being every row's top N + 1, so
    that beam 1 has a margin too -- and at the end the gap between the best and the
    second-best final score), `steps`, `beam_scores` / `beam_rows` (beam order, eos included)."""
    from . import _lib
    n = _check_beam(cfg, beam_size)
    limits = step_limits(row_len, max_len)
    W = {k: v.detach().to("cpu", dtype) for k, v in R.native_names(cfg, sd).items()}
    pe = R.positional_table(cfg.d_model, R.MAX_POSITIONS, dtype)
    enc = enc_rows.detach().reshape(-1, cfg.d_model).to("cpu", dtype)
    rs, rl = (t.tolist() for t in _lib.packed_ranges(row_start, row_len, enc.shape[0], "encoder rows"))
    out = []
    for s, m, lim in zip(rs, rl, limits):
        hs = HostSearch(cfg, W, pe, enc[s: s + m], n, dtype)
        hs.run(lim)
        out.append(hs.result(float(length_penalty)))
    return out


# ------------------------------------------------------------------------------------ device
class AttentionDecoder:
    """The device search over an AttentionRescorer's cfm_aed handle (csrc/attdec.hip): no second copy of the
    decoder weights."""

    def __init__(self, rescorer: "R.AttentionRescorer"):
        self.rescorer = rescorer
        self.cfg, self.device, self.dtype = rescorer.cfg, rescorer.device, rescorer.dtype

    @torch.no_grad()
    def search(self, enc_rows: torch.Tensor, row_start, row_len, beam_size: int = 10, length_penalty: float = 0.0,
               max_len: Optional[int] = None, return_trace: bool = False, check_host: bool = True
               ) -> List[DecodeResult]:
        """One device search over the packed encoder rows enc_rows [rows, d] (utterance b = rows [row_start[b],
        + row_len[b])).  A row range outside the encoder rows raises ValueError (`check_host` False leaves that check
        to the device's status word: the call then raises after the search, such an utterance having been skipped,
        and the results of the others are in `last_results`)."""
        from . import _lib
        c, dev, h = self.cfg, self.device, self.rescorer._h
        n = _check_beam(c, beam_size)
        limits = step_limits(row_len, max_len)
        B = len(limits)
        if B == 0:
            return []
        enc = enc_rows.reshape(-1, c.d_model).to(dev, torch.float32).contiguous()
        rows = enc.shape[0]
        if check_host:
            rs, rl = _lib.packed_ranges(row_start, row_len, rows, "encoder rows")
        else:
            rs, rl = _lib.i32_host(row_start), _lib.i32_host(row_len)
        S = max(limits)
        Rn = B * n
        rs_d, rl_d, lim_d = rs.to(dev), rl.to(dev), torch.tensor(limits, dtype=torch.int32).to(dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            nbytes = int(_lib.cfm_attdec_workspace_bytes(h, B, n, rows, S))
            if nbytes == 0:
                raise ValueError("attention decoding: the library refuses this geometry")
            state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.last_workspace_bytes = nbytes
            _lib.check(_lib.cfm_attdec_begin(h, enc.data_ptr(), rows, rs_d.data_ptr(), rl_d.data_ptr(), lim_d.data_ptr(),
                                             B, n, S, state.data_ptr(), nbytes, stream))
            words = state[:8].view(torch.int32)
            step, polls = 1, 0
            while step <= S:
                running = int(words[1].item())        # synchronises (a rejected utterance never runs: the others go on)
                polls += 1
                if running == 0:
                    break
                k = min(POLL_STEPS, S - step + 1)
                _lib.check(_lib.cfm_attdec_steps(h, state.data_ptr(), B, n, rows, S, step, k, stream))
                step += k
            self.last_steps_enqueued, self.last_polls = step - 1, polls
            tokens = torch.zeros(Rn, max(S, 1), dtype=torch.int32, device=dev)
            lens = torch.zeros(Rn, dtype=torch.int32, device=dev)
            finals = torch.zeros(Rn, dtype=torch.float32, device=dev)
            best = torch.zeros(B, dtype=torch.int32, device=dev)
            tr = None
            if return_trace:
                tr = (torch.zeros(max(S, 1), Rn, dtype=torch.int32, device=dev),
                      torch.zeros(max(S, 1), Rn, dtype=torch.int32, device=dev),
                      torch.zeros(max(S, 1), Rn, dtype=torch.float32, device=dev))
            _lib.check(_lib.cfm_attdec_finish(h, state.data_ptr(), B, n, rows, S, float(length_penalty),
                                              tokens.data_ptr(), lens.data_ptr(), finals.data_ptr(), best.data_ptr(),
                                              _lib.ptr(tr[0]) if tr else 0, _lib.ptr(tr[1]) if tr else 0,
                                              _lib.ptr(tr[2]) if tr else 0, stream))
            status = int(words[0].item())
        tok_h, len_h, fin_h, best_h = tokens.cpu(), lens.cpu().tolist(), finals.cpu().tolist(), best.cpu().tolist()
        tr_h = [t.cpu() for t in tr] if tr else None
        out = []
        for b in range(B):
            m = len_h[b * n]
            hyps = [tok_h[b * n + j, :m].tolist() for j in range(n)]
            trace = None
            if tr_h is not None:
                trace = [(tr_h[0][t, b * n: b * n + n].tolist(), tr_h[1][t, b * n: b * n + n].tolist(),
                          tr_h[2][t, b * n: b * n + n].tolist()) for t in range(m)]
            r = _result(c, hyps, fin_h[b * n: b * n + n], trace)
            assert r.best_index == best_h[b], "device and host selection differ"
            out.append(r)
        self.last_results = out
        if status != 0:
            raise ValueError(f"attention decoding failed (status {status}): {_STATUS.get(status, 'internal')}")
        return out
