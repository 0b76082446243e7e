"""Transducer attention rescoring: the reference's modes rnnt_beam_attn_rescoring and ctc_beam_td_attn_rescoring
(bin/recognize.py --modes -> Transducer.transducer_attention_rescoring, transducer/transducer.py:257-391) for
`model: transducer` checkpoints: the n-best of a beam search re-ranked by three scores per hypothesis,

    total_i = attn_i * attn_weight + search_score_i * ctc_weight + td_i * transducer_weight,

the first strictly larger total winning.  `search_score_i` is the n-best score of whichever search produced the list
(the reference calls its weight ctc_weight in both modes), `attn_i` the attention decoder's score exactly as
rescore.combine forms `decoder_scores`, and `td_i` the full-sum transducer log-likelihood of the hypothesis
(_cal_transducer_score = -rnnt_loss), the only transducer score here that sums over all alignments.

Semantics.  For a hypothesis y = (y_1 .. y_U) of an utterance with encoder rows x_0 .. x_{T-1}, T >= 1:

    p_u     = predictor output after [blank, y_1 .. y_u], u = 0 .. U   (predictor(add_blank(hyps)); the recurrence of
              forward_step in the beam search)
    lp[t,u] = log_softmax(ffn_out(tanh(enc_ffn(x_t) + pred_ffn(p_u))))
    b[t,u]  = lp[t,u,blank],   k[t,u] = lp[t,u,y_{u+1}] (u < U)                       f32
    alpha[0,0] = 0,  alpha[t,u] = log_add(alpha[t-1,u] + b[t-1,u], alpha[t,u-1] + k[t,u-1])
    td      = alpha[T-1,U] + b[T-1,U]                                                   f64

An utterance with 0 rows keeps its search result untouched.  Deviations from the reference: it asserts
len(hyps) == beam_size, here a shorter final beam is rescored as it is; its batch size 1 becomes the whole masked
batch; parity of this td with torchaudio.functional.rnnt_loss is UNPINNED (torchaudio is not installed where the
fixtures are generated: the recursion is checked against brute-force enumeration of all alignments instead).

`lattice_logp_host` / `td_score_host` / `td_score_enum` / `rescore_host` restate it on the CPU; `TransducerRescorer`
is the device implementation over an RNNTGreedy's handle (csrc/rnnt_lattice.hip, cfm_rnnt_td_score): the reference
materialises the joint as [n_hyps, T, U + 1, V], the device writes eight bytes per lattice node.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .rescore import AEDConfig, combine, score_host, use_right
from .search import DecodeResult, log_add2

DEFAULT_MAX_LATTICE_BYTES = 1 << 30
_DT = {"fp32": 0, "bf16": 1, "fp16": 1}   # (the 16-bit lattice kernel has bf16 operands)


# ----------------------------------------------------------------------------- host restatement
def _host_rnn(m, dtype):
    """The HostTransducer's LSTM in `dtype` (built once per dtype and kept on the object)."""
    cache = m.__dict__.setdefault("_rnn_by_dtype", {})
    if dtype not in cache:
        cfg = m.cfg
        rnn = torch.nn.LSTM(cfg.embed_size, cfg.hidden, cfg.num_layers, bias=True, batch_first=True)
        rnn.load_state_dict({k[len("predictor.rnn."):]: v for k, v in m.sd.items() if k.startswith("predictor.rnn.")})
        cache[dtype] = rnn.to(dtype).eval()
    return cache[dtype]


@torch.no_grad()
def joint_projections_host(host_transducer, enc, hyp: Sequence[int], dtype=torch.float64):
    """(enc_ffn(x_t) [T, J], pred_ffn(p_u) [U + 1, J]) of hypothesis `hyp` over the encoder rows enc [T, enc_dim], in
    `dtype` over a transducer_beam.HostTransducer: the two operands of the joint."""
    m = host_transducer
    cfg = m.cfg
    W = {k: v.to(dtype) for k, v in m.sd.items()}
    lin = torch.nn.functional.linear
    x = torch.as_tensor(enc).reshape(-1, cfg.enc_dim).to(dtype)
    if cfg.stateless:   # state u = the context function of the last history_size + 1 ids of [blank, y_1 .. y_u]
        from .transducer_beam import hyp_windows
        p = m.predict_windows(hyp_windows(cfg, hyp), dtype)                                      # [U + 1, E]
    else:
        emb = W["predictor.embed.weight"][torch.tensor([cfg.blank] + [int(t) for t in hyp], dtype=torch.long)].unsqueeze(0)
        out, _ = _host_rnn(m, dtype)(emb)
        p = lin(out[0], W["predictor.projection.weight"], W["predictor.projection.bias"])        # [U + 1, P]
    e = lin(x, W["joint.enc_ffn.weight"], W["joint.enc_ffn.bias"])                               # [T, J]
    q = lin(p, W["joint.pred_ffn.weight"], W["joint.pred_ffn.bias"])                             # [U + 1, J]
    return e, q


@torch.no_grad()
def lattice_logp_host(host_transducer, enc, hyp: Sequence[int], dtype=torch.float64) -> Tuple[np.ndarray, np.ndarray]:
    """(b [T, U + 1], k [T, U]) of hypothesis `hyp` over the encoder rows enc [T, enc_dim], computed in `dtype` over a
    transducer_beam.HostTransducer."""
    m = host_transducer
    cfg = m.cfg
    y = [int(t) for t in hyp]
    U = len(y)
    e, q = joint_projections_host(m, enc, y, dtype)
    T = e.shape[0]
    lp = torch.nn.functional.linear(torch.tanh(e.unsqueeze(1) + q.unsqueeze(0)), m.sd["joint.ffn_out.weight"].to(dtype),
                                    m.sd["joint.ffn_out.bias"].to(dtype)).log_softmax(-1)        # [T, U + 1, V]
    b = lp[:, :, cfg.blank]
    k = lp[:, :U, :].gather(2, torch.tensor(y, dtype=torch.long).view(1, U, 1).expand(T, U, 1))[:, :, 0]
    return b.numpy(), k.numpy().reshape(T, U)


def td_score_host(b, k) -> float:
    """td of a lattice: b [T, U + 1], k [T, U]; the recursion in Python f64 with the reference's log_add."""
    b = np.asarray(b, dtype=np.float64)
    T, U1 = b.shape
    k = np.asarray(k, dtype=np.float64).reshape(T, U1 - 1)
    if T < 1:
        raise ValueError("a lattice needs at least one frame")
    bl, kl = b.tolist(), k.tolist()
    prev = [0.0] * U1
    for u in range(1, U1):
        prev[u] = prev[u - 1] + kl[0][u - 1]
    for t in range(1, T):
        cur = [prev[0] + bl[t - 1][0]] + [0.0] * (U1 - 1)
        for u in range(1, U1):
            cur[u] = log_add2(prev[u] + bl[t - 1][u], cur[u - 1] + kl[t][u - 1])
        prev = cur
    return prev[U1 - 1] + bl[T - 1][U1 - 1]


def td_score_enum(b, k) -> float:
    """td by brute force: the log of the summed probabilities of every alignment (every order of T - 1 blanks and U
    tokens, then the final blank).  For tiny lattices only."""
    b = np.asarray(b, dtype=np.float64)
    T, U1 = b.shape
    k = np.asarray(k, dtype=np.float64).reshape(T, U1 - 1)
    paths: List[float] = []

    def walk(t: int, u: int, lp: float) -> None:
        if t == T - 1 and u == U1 - 1:
            paths.append(lp + float(b[t, u]))
            return
        if t < T - 1:
            walk(t + 1, u, lp + float(b[t, u]))
        if u < U1 - 1:
            walk(t, u + 1, lp + float(k[t, u]))

    walk(0, 0, 0.0)
    mx = max(paths)
    return mx + math.log(math.fsum(math.exp(v - mx) for v in paths))


def _check_weights(ctc_weight, attn_weight, transducer_weight) -> Tuple[float, float, float]:
    cw, aw, tw = float(ctc_weight), float(attn_weight), float(transducer_weight)
    if not (cw >= 0 and aw >= 0 and tw >= 0):
        raise ValueError("ctc_weight, attn_weight and transducer_weight must be >= 0")
    return cw, aw, tw


def combine_td(aed_cfg: Optional[AEDConfig], scored, td: Sequence[Sequence[float]], results: Sequence[DecodeResult],
               ctc_weight: float, attn_weight: float, transducer_weight: float, reverse_weight: float = 0.0,
               return_nbest: bool = False, attn_scores=None) -> List[DecodeResult]:
    """transducer.py:369-391 in Python f64.  `scored[b][i]` = the decoder's (l2r, r2l) rows as rescore.score_host returns
    them (None without a decoder: attn is 0 and attn_weight must be 0), or `attn_scores[b][i]` = decoder scores that
    were formed elsewhere (they take the place of `scored`); td[b][i] the transducer scores.  Results shaped
    like rescore.combine's: `best_index`, `nbest_scores` = the totals, the times of the chosen hypothesis, and
    `td_scores` / `decoder_scores`.  An utterance whose td list is None (no rows) keeps its result."""
    cw, aw, tw = _check_weights(ctc_weight, attn_weight, transducer_weight)
    if scored is None and attn_scores is None and aw > 0:
        raise ValueError("attn_weight > 0 needs the attention decoder's scores")
    out = []
    for b, res in enumerate(results):
        if res.nbest is None or res.nbest_scores is None:
            raise ValueError("transducer attention rescoring needs the n-best of a beam search")
        if td[b] is None:
            out.append(res)
            continue
        n = len(res.nbest)
        attn = [0.0] * n
        if attn_scores is not None:
            attn = [float(v) for v in attn_scores[b]]
            if len(attn) != n:
                raise ValueError("one decoder score per hypothesis")
        elif scored is not None:
            # the decoder score exactly as rescore.combine forms decoder_scores
            attn = combine(aed_cfg, [scored[b]], [res], 0.0, reverse_weight)[0].decoder_scores
        totals = [attn[i] * aw + float(res.nbest_scores[i]) * cw + float(td[b][i]) * tw for i in range(n)]
        best = 0
        for i in range(1, n):
            if totals[i] > totals[best]:
                best = i
        times = res.nbest_times
        order = sorted(range(n), key=lambda i: -totals[i]) if return_nbest else list(range(n))
        r = DecodeResult(list(res.nbest[best]), totals[best], times=times[best] if times is not None else None,
                         nbest=[res.nbest[i] for i in order], nbest_scores=[totals[i] for i in order],
                         nbest_times=[times[i] for i in order] if times is not None else None)
        r.best_index = best
        r.td_scores = [float(v) for v in td[b]]
        r.decoder_scores = list(attn)
        out.append(r)
    return out


def rescore_host(host_transducer, aed: Optional[Tuple[AEDConfig, dict]], enc_rows, row_start, row_len,
                 results: Sequence[DecodeResult], ctc_weight: float = 0.5, attn_weight: Optional[float] = None,
                 transducer_weight: float = 0.5, reverse_weight: float = 0.0, dtype=torch.float64,
                 return_nbest: bool = False) -> List[DecodeResult]:
    """The whole mode on the CPU: `results` are a beam search's DecodeResults for the utterances whose encoder rows are
    [row_start[b], + row_len[b]) of enc_rows; `aed` = (AEDConfig, decoder state dict) or None (attn_weight then
    defaults to 0).  The lattice and the decoder run in `dtype`."""
    aw = (0.5 if aed is not None else 0.0) if attn_weight is None else float(attn_weight)
    enc = torch.as_tensor(enc_rows).detach().cpu().reshape(-1, host_transducer.cfg.enc_dim)
    td = []
    for b, res in enumerate(results):
        s, n = int(row_start[b]), int(row_len[b])
        if n < 1:
            td.append(None)
            continue
        td.append([td_score_host(*lattice_logp_host(host_transducer, enc[s: s + n], h, dtype)) for h in res.nbest])
    scored = None
    if aed is not None and aw > 0:
        c, sd = aed
        scored = score_host(c, sd, enc, row_start, row_len, [r.nbest for r in results], use_right(c, reverse_weight), dtype)
    return combine_td(aed[0] if aed is not None else None, scored, td, results, ctc_weight, aw, transducer_weight,
                      reverse_weight, return_nbest)


# ----------------------------------------------------------------------------- device
def _groups(nodes: Sequence[int], max_bytes: int) -> List[List[int]]:
    """Consecutive hypotheses whose lattice buffers (8 bytes per node) fit max_bytes; one larger than that runs alone."""
    out, cur, used = [], [], 0
    for i, n in enumerate(nodes):
        if cur and used + 8 * n > max_bytes:
            out.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += 8 * n
    if cur:
        out.append(cur)
    return out


class TransducerRescorer:
    """cfm_rnnt_td_score over an RNNTGreedy's handle (no second handle, no second upload from Python) and, with a
    rescore.AttentionRescorer, the attention decoder's scores of the same hypotheses.  dtype "fp32" runs the joint
    lattice on exact f32 MFMA operands, "bf16" / "fp16" on bf16 operands with f32 accumulation."""

    def __init__(self, rnnt, rescorer=None, dtype: str = "fp32", max_lattice_bytes: int = DEFAULT_MAX_LATTICE_BYTES):
        if dtype not in _DT:
            raise ValueError(f"dtype {dtype!r}: fp32, bf16 or fp16")
        self.rnnt, self.rescorer, self.dtype = rnnt, rescorer, dtype
        self.cfg = rnnt.cfg
        self.device = rnnt.device
        self.max_lattice_bytes = int(max_lattice_bytes)
        self.last_error = 0      # the device's status word of the last call (4: a non-finite lattice node)
        self.last_groups = 0     # device calls the last td_scores took
        self.last_workspace_bytes = 0

    def _layout(self, hyps: Sequence[Tuple[int, int, Sequence[int]]]):
        """Descriptor arrays of hypotheses (utterance, T, tokens): tokens per state, desc [n, 4], node0 [n + 1]."""
        blank = self.cfg.blank
        toks, desc, node0 = [], [], [0]
        for utt, T, y in hyps:
            desc.append([utt, len(toks), len(y) + 1, 0])
            toks.append(blank)
            toks.extend(int(t) for t in y)
            node0.append(node0[-1] + T * (len(y) + 1))
        return toks, desc, node0

    def _check_tokens(self, nbest) -> None:
        for hyps in nbest:
            for h in hyps:
                if any(int(t) < 0 or int(t) >= self.cfg.vocab for t in h):
                    raise ValueError("a hypothesis holds a token id outside [0, vocab)")

    @torch.no_grad()
    def td_scores(self, enc_rows: torch.Tensor, row_start, row_len, nbest: Sequence[Sequence[Sequence[int]]]
                  ) -> List[Optional[List[float]]]:
        """td[b][i] (f64) of hypothesis i of utterance b = rows [row_start[b], + row_len[b]) of enc_rows
        [rows, enc_dim]; None for an utterance without rows.  Hypotheses go to the device in groups whose lattice
        buffers fit `max_lattice_bytes`."""
        from . import _lib
        cfg, dev = self.cfg, self.device
        self._check_tokens(nbest)
        enc = enc_rows.reshape(-1, cfg.enc_dim).to(dev, torch.float32).contiguous()
        rows = enc.shape[0]
        rs, rl = (t.tolist() for t in _lib.packed_ranges(row_start, row_len, rows, "encoder rows"))
        if len(nbest) != len(rs):
            raise ValueError("one n-best list per utterance")
        flat = [(b, i) for b, hyps in enumerate(nbest) if rl[b] >= 1 for i in range(len(hyps))]
        out: List[Optional[List[float]]] = [None if rl[b] < 1 else [0.0] * len(h) for b, h in enumerate(nbest)]
        self.last_error, self.last_groups = 0, 0
        if not flat:
            return out
        nodes = [rl[b] * (len(nbest[b][i]) + 1) for b, i in flat]
        stream = torch.cuda.current_stream(dev).cuda_stream
        for grp in _groups(nodes, self.max_lattice_bytes):
            # the group's utterances, renumbered from 0
            utts = sorted({flat[j][0] for j in grp})
            local = {b: q for q, b in enumerate(utts)}
            toks, desc, node0 = self._layout([(local[flat[j][0]], rl[flat[j][0]], nbest[flat[j][0]][flat[j][1]])
                                              for j in grp])
            n_hyp, n_states, total = len(grp), len(toks), node0[-1]
            max_u1 = max(d[2] for d in desc)
            i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)   # noqa: E731
            tok_d, desc_d = i32(toks), i32(desc)
            node0_d = torch.tensor(node0, dtype=torch.int64).to(dev)
            # only the rows the group's utterances span go to the call (enc_ffn and the row-sized workspace regions
            # are per call); the dtype is an argument, the handle's state is not touched
            r0, r1 = min(rs[b] for b in utts), max(rs[b] + rl[b] for b in utts)
            enc_g, rows_g = enc[r0:r1], r1 - r0
            rs_d, rl_d = i32([rs[b] - r0 for b in utts]), i32([rl[b] for b in utts])
            td = torch.zeros(n_hyp, dtype=torch.float64, device=dev)
            nbytes = int(_lib.cfm_rnnt_td_workspace_bytes(self.rnnt._h, rows_g, n_hyp, n_states, max_u1, total))
            if nbytes == 0:
                raise ValueError("transducer rescoring: rows / hypotheses / nodes outside what the workspace can hold")
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.cfm_rnnt_td_score(self.rnnt._h, enc_g.data_ptr(), rows_g, rs_d.data_ptr(),
                                                  rl_d.data_ptr(), len(utts), tok_d.data_ptr(), n_states,
                                                  desc_d.data_ptr(), node0_d.data_ptr(), n_hyp, max_u1, total,
                                                  _DT[self.dtype], td.data_ptr(), ws.data_ptr(), nbytes, stream))
                td_h = td.cpu().tolist()   # (synchronises the stream: the inputs above are consumed)
                err = int(_lib.cfm_rnnt_beam_error(ws.data_ptr()))
            self.last_groups += 1
            self.last_workspace_bytes = nbytes
            if err not in (0, 4):
                raise RuntimeError(f"transducer rescoring: device status word {err}")
            self.last_error = max(self.last_error, err)
            for j, v in zip(grp, td_h):
                out[flat[j][0]][flat[j][1]] = v
        return out

    def rescore(self, results: Sequence[DecodeResult], enc_rows: torch.Tensor, row_start, row_len,
                ctc_weight: float = 0.5, attn_weight: Optional[float] = None, transducer_weight: float = 0.5,
                reverse_weight: Optional[float] = None, return_nbest: bool = False, attn_scores=None
                ) -> List[DecodeResult]:
        """transducer_attention_rescoring of a beam search's `results` (see combine_td).  attn_weight defaults to 0.5
        with an attention decoder and 0 without; reverse_weight to the decoder's model_conf value.  `attn_scores[b][i]`:
        decoder scores of the hypotheses formed elsewhere (the device decoder is then not run and need not exist)."""
        for r in results:
            if r.nbest is None or r.nbest_scores is None:
                raise ValueError("transducer attention rescoring needs the n-best of a beam search")
        have_attn = self.rescorer is not None or attn_scores is not None
        aw = (0.5 if have_attn else 0.0) if attn_weight is None else float(attn_weight)
        cw, aw, tw = _check_weights(ctc_weight, aw, transducer_weight)
        if aw > 0 and not have_attn:
            raise ValueError("attn_weight > 0 needs an attention decoder (the checkpoint holds no decoder.* tensors)")
        nbest = [r.nbest for r in results]
        td = self.td_scores(enc_rows, row_start, row_len, nbest)
        scored, c, rw = None, None, 0.0
        if aw > 0 and attn_scores is None:
            c = self.rescorer.cfg
            rw = c.reverse_weight if reverse_weight is None else float(reverse_weight)
            scored = self.rescorer.score(enc_rows, row_start, row_len, nbest, use_right(c, rw))
        return combine_td(c, scored, td, results, cw, aw, tw, rw, return_nbest, attn_scores)

    # ---- the single kernels (include/cfm_ops.h), for the op tests and tools
    @torch.no_grad()
    def lattice(self, enc_proj: torch.Tensor, pred_proj: torch.Tensor, row_start, row_len,
                hyps: Sequence[Tuple[int, Sequence[int]]], dtype: Optional[str] = None):
        """cfm_op_rnnt_lattice: enc_proj [rows, J] and pred_proj [n_states, J] f32 (the states of hypotheses
        (utterance, tokens) in order, U + 1 each) -> per hypothesis (b [T, U + 1], k [T, U]) f32 on the host."""
        from . import _lib
        dev = self.device
        e = enc_proj.to(dev, torch.float32).contiguous()
        p = pred_proj.to(dev, torch.float32).contiguous()
        rs, rl = _lib.packed_ranges(row_start, row_len, e.shape[0], "encoder rows")
        rll = rl.tolist()
        toks, desc, node0 = self._layout([(u, rll[u], y) for u, y in hyps])
        if p.shape[0] != len(toks):
            raise ValueError("pred_proj must hold U + 1 states per hypothesis")
        total = node0[-1]
        i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)   # noqa: E731
        tok_d, desc_d, rs_d, rl_d = i32(toks), i32(desc), rs.to(dev), rl.to(dev)
        node0_d = torch.tensor(node0, dtype=torch.int64).to(dev)
        b = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
        k = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.cfm_op_rnnt_lattice(self.rnnt._h, _DT[dtype or self.dtype], e.data_ptr(), e.shape[0],
                                                p.data_ptr(), p.shape[0], tok_d.data_ptr(), rs_d.data_ptr(),
                                                rl_d.data_ptr(), rs.numel(), desc_d.data_ptr(), node0_d.data_ptr(),
                                                len(desc), total, b.data_ptr(), k.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream))
            bh, kh = b.cpu().numpy(), k.cpu().numpy()
        out = []
        for (u, y), d, n0 in zip(hyps, desc, node0):
            T, U1 = rll[u], d[2]
            out.append((bh[n0: n0 + T * U1].reshape(T, U1), kh[n0: n0 + T * U1].reshape(T, U1)[:, : U1 - 1]))
        return out


@torch.no_grad()
def alpha_device(lattices: Sequence[Tuple[np.ndarray, np.ndarray]], device) -> Tuple[List[float], int]:
    """cfm_op_rnnt_alpha over lattices (b [T, U + 1], k [T, U]): (td per lattice, the status word)."""
    from . import _lib
    dev = torch.device(device)
    bs, ks, ht, hu, node0 = [], [], [], [], [0]
    for b, k in lattices:
        b = np.asarray(b, dtype=np.float32)
        T, U1 = b.shape
        kk = np.zeros((T, U1), dtype=np.float32)
        kk[:, : U1 - 1] = np.asarray(k, dtype=np.float32).reshape(T, U1 - 1)
        bs.append(b.reshape(-1))
        ks.append(kk.reshape(-1))
        ht.append(T)
        hu.append(U1)
        node0.append(node0[-1] + T * U1)
    b_d = torch.from_numpy(np.concatenate(bs)).to(dev)
    k_d = torch.from_numpy(np.concatenate(ks)).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)   # noqa: E731
    ht_d, hu_d = i32(ht), i32(hu)
    node0_d = torch.tensor(node0, dtype=torch.int64).to(dev)
    n, mu = len(ht), max(hu)
    td = torch.zeros(n, dtype=torch.float64, device=dev)
    nbytes = int(_lib.cfm_op_rnnt_alpha_workspace_bytes(n, mu))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.cfm_op_rnnt_alpha(b_d.data_ptr(), k_d.data_ptr(), ht_d.data_ptr(), hu_d.data_ptr(),
                                          node0_d.data_ptr(), n, mu, node0[-1], td.data_ptr(), ws.data_ptr(), nbytes,
                                          torch.cuda.current_stream(dev).cuda_stream))
        out = td.cpu().tolist()
        err = int(_lib.cfm_rnnt_beam_error(ws.data_ptr()))
    return out, err
