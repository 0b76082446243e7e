"""Transducer prefix beam search: the reference's mode rnnt_beam_search (bin/recognize.py --modes ->
Transducer.beam_search -> PrefixBeamSearch.prefix_beam_search, transducer/search/prefix_beam_search.py:41-146) for
`model: transducer` checkpoints, on the device for every utterance of a packed batch at once (csrc/rnnt_beam.hip,
cfm_rnnt_beam_search in include/cfm.h) and restated on the CPU.

Semantics.  Per utterance the beam starts as one hypothesis [blank] with score 0 and a zero LSTM state;
every encoder frame runs exactly one step:

  1. predictor.forward_step(last token, cache) and the joint against the frame for each of the n <= K hypotheses,
     log_softmax over V;
  2. fusion in f32: logp = log(tw * exp(logp) + cw * exp(ctc_logp[frame]));
  3. first prune: per hypothesis the top K of the fused row (value descending, index ascending); candidate score
     f32(score) + logp in f32 (the reference rebuilds an f32 score tensor from Python floats every frame);
  4. expansion in the order (hypothesis ascending, rank ascending): blank keeps the hypothesis and its old cache, a
     token appends it and takes the new cache;
  5. prefix fusion: a candidate whose token list equals an earlier candidate's is folded into the earlier one
     (log_add of the two scores in f64; the earlier one's position and cache are kept);
  6. second prune: stable sort by score descending (ties: creation order), keep K;
  7. result beam[0]; the whole final beam is the n-best.

`beam_step_host` is steps 3-6, `prefix_beam_search_host` the whole search with the predictor and joint in torch f32,
`RNNTBeamSearch` the device search over an RNNTGreedy's handle.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .search import DecodeResult, log_add2, nbest_results
from .transducer import RNNTConfig

MAX_BEAM = 16
NEG_INF = float("-inf")


def _check_args(beam_size: int, vocab: int, ctc_weight: float, transducer_weight: float, has_ctc: bool) -> None:
    if not 1 <= int(beam_size) <= MAX_BEAM or int(beam_size) > vocab:
        raise ValueError(f"beam_size {beam_size}: 1 .. {MAX_BEAM} and at most the vocabulary ({vocab})")
    if not (ctc_weight >= 0 and transducer_weight >= 0) or not (ctc_weight + transducer_weight > 0):
        raise ValueError("ctc_weight and transducer_weight must be >= 0 and not both 0")
    if ctc_weight > 0 and not has_ctc:
        raise ValueError("ctc_weight > 0 needs the CTC log-probs (ctc_logp)")


# ----------------------------------------------------------------------------- the step on the host
def topk_rows_host(fused: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per row the k largest values by (value descending, index ascending): values [n, k] f32, ids [n, k] int32."""
    fused = np.asarray(fused, dtype=np.float32)
    ids = np.argsort(-fused, axis=1, kind="stable")[:, :k].astype(np.int32)
    return np.take_along_axis(fused, ids.astype(np.int64), axis=1), ids


def beam_step_host(hyps: Sequence[Tuple[int, ...]], scores: Sequence[float], topv, topi, beam_size: int,
                   blank: int = 0):
    """One expand / fuse / prune step (prefix_beam_search.py:102-144) of a beam `hyps` (token tuples without the
    leading blank) with `scores`, given each hypothesis' top-K fused log-probs topv [n, K] (f32) and ids topi [n, K].
    Returns (kept, gap): kept = the new beam as (hyp, score, parent slot, token, appended) in order -- token is the
    blank for an unchanged hypothesis, appended says whether the survivor takes the parent's new predictor state --
    and gap = the smallest difference between adjacent candidates among ranks 0 .. K of the sorted fused list (inf
    when there is one candidate only)."""
    K = int(beam_size)
    topv = np.asarray(topv, dtype=np.float32).reshape(len(hyps), K)
    topi = np.asarray(topi).reshape(len(hyps), K)
    sc32 = np.asarray(list(scores), dtype=np.float64).astype(np.float32)   # torch.tensor([floats]) is f32
    fused: List[list] = []
    index: Dict[Tuple[int, ...], int] = {}
    for h, hyp in enumerate(hyps):
        for j in range(K):
            u = int(topi[h, j])
            s = float(np.float32(sc32[h] + topv[h, j]))
            if s != s:
                s = NEG_INF   # the device ranks NaN as -inf
            new = tuple(hyp) if u == blank else tuple(hyp) + (u,)
            at = index.get(new)
            if at is None:
                index[new] = len(fused)
                fused.append([new, s, h, u, u != blank])
            else:
                fused[at][1] = log_add2(fused[at][1], s)
    order = sorted(range(len(fused)), key=lambda i: -fused[i][1])   # stable: ties keep creation order
    top = [fused[i][1] for i in order[: K + 1]]
    gap = min((a - b for a, b in zip(top, top[1:]) if a != NEG_INF), default=math.inf)
    return [tuple(fused[i]) for i in order[:K]], gap


# ----------------------------------------------------------------------------- predictor and joint on the host
_ACTS = {"relu": torch.relu, "swish": torch.nn.functional.silu, "tanh": torch.tanh, "gelu": torch.nn.functional.gelu}


def hyp_windows(cfg: RNNTConfig, hyp: Sequence[int]) -> np.ndarray:
    """The id windows [U + 1, history_size + 1] of the states of [blank, y_1 .. y_U] (oldest id first, -1 = a position
    before the sos: a zero vector)."""
    seq = [-1] * cfg.history_size + [cfg.blank] + [int(t) for t in hyp]
    K = cfg.context
    return np.array([seq[u: u + K] for u in range(len(hyp) + 1)], dtype=np.int64).reshape(len(hyp) + 1, K)


class HostTransducer:
    """The reference's predictor (RNNPredictor lstm, EmbeddingPredictor or ConvPredictor) + TransducerJoint math in
    torch f32 on the CPU, from a state dict."""

    def __init__(self, cfg: RNNTConfig, state_dict: Dict[str, torch.Tensor]):
        self.cfg = cfg
        sd = {k: v.detach().to("cpu", torch.float32) for k, v in state_dict.items()
              if k.startswith(("predictor.", "joint."))}
        self.sd = sd
        if cfg.stateless:
            return
        self.rnn = torch.nn.LSTM(cfg.embed_size, cfg.hidden, cfg.num_layers, bias=True, batch_first=True)
        self.rnn.load_state_dict({k[len("predictor.rnn."):]: v for k, v in sd.items() if k.startswith("predictor.rnn.")})
        self.rnn.eval()

    # ---- the stateless predictors: the state of a hypothesis is its id window
    def _context_rows(self, windows, dtype) -> torch.Tensor:
        """[n, K] ids (-1 = before the sos) -> their embedding rows [n, K, E] in `dtype`, zero vectors for -1."""
        w = torch.as_tensor(np.asarray(windows), dtype=torch.long).reshape(-1, self.cfg.context)
        rows = self.sd["predictor.embed.weight"].to(dtype)[w.clamp(min=0)]
        return rows * (w >= 0).unsqueeze(-1).to(dtype)

    def _norm_act(self, x: torch.Tensor, dtype) -> torch.Tensor:
        cfg = self.cfg
        y = torch.nn.functional.layer_norm(x, (cfg.embed_size,), self.sd["predictor.norm.weight"].to(dtype),
                                           self.sd["predictor.norm.bias"].to(dtype), cfg.ln_eps)
        return _ACTS[cfg.act](y)

    @torch.no_grad()
    def predict_windows(self, windows, dtype=torch.float64) -> torch.Tensor:
        """The predictor as a pure context function: windows [n, K] -> outputs [n, E] in `dtype`.
        embedding: x = sum_c (c_c . q_c) c_c / (n_head K), q_c the heads of pos_embed summed; y = act(LN(ffn(x))).
        conv: x[d] = sum_c w[d, 0, c] c_c[d] (+ bias); y = act(LN(x))."""
        cfg = self.cfg
        E, K = cfg.embed_size, cfg.context
        c = self._context_rows(windows, dtype)                                               # [n, K, E]
        if cfg.predictor == "embedding":
            q = self.sd["predictor.pos_embed.weight"].to(dtype).view(cfg.n_head, E, K).sum(0).t()   # [K, E]
            x = ((c * q).sum(-1, keepdim=True) * c).sum(1) / (cfg.n_head * K)
            x = torch.nn.functional.linear(x, self.sd["predictor.ffn.weight"].to(dtype),
                                           self.sd["predictor.ffn.bias"].to(dtype))
        else:
            x = (c * self.sd["predictor.conv.weight"].to(dtype)[:, 0, :].t()).sum(1)
            if cfg.conv_bias:
                x = x + self.sd["predictor.conv.bias"].to(dtype)
        return self._norm_act(x, dtype)

    @torch.no_grad()
    def step_windows(self, windows) -> torch.Tensor:
        """forward_step in f32 with the reference's tensor shapes (predictor.py:322-362, 450-471): windows [n, K] ->
        the predictor outputs [n, 1, E]."""
        cfg = self.cfg
        E, K = cfg.embed_size, cfg.context
        ctx = self._context_rows(windows, torch.float32)                                     # [n, K, E]
        if cfg.predictor == "embedding":
            ex = ctx.unsqueeze(1).unsqueeze(2)                                               # [n, 1, 1, K, E]
            pos = self.sd["predictor.pos_embed.weight"].view(cfg.n_head, E, K).permute(0, 2, 1)
            wgt = (ex * pos).sum(dim=-1).unsqueeze(3)                                        # [n, 1, heads, 1, K]
            out = wgt.matmul(ex).squeeze(dim=3).sum(dim=2) / (cfg.n_head * K)                # [n, 1, E]
            out = torch.nn.functional.linear(out, self.sd["predictor.ffn.weight"], self.sd["predictor.ffn.bias"])
        else:
            out = torch.nn.functional.conv1d(ctx.permute(0, 2, 1), self.sd["predictor.conv.weight"],
                                             self.sd.get("predictor.conv.bias") if cfg.conv_bias else None,
                                             groups=E).permute(0, 2, 1)
        return self._norm_act(out, torch.float32)

    @torch.no_grad()
    def step(self, tokens: Sequence[int], h: torch.Tensor, c: torch.Tensor):
        """forward_step: tokens [n], state h / c [layers, n, hidden] -> (predictor output [n, 1, P], h', c')."""
        emb = self.sd["predictor.embed.weight"][torch.as_tensor(list(tokens), dtype=torch.long)].unsqueeze(1)
        out, (hn, cn) = self.rnn(emb, (h.contiguous(), c.contiguous()))
        out = torch.nn.functional.linear(out, self.sd["predictor.projection.weight"], self.sd["predictor.projection.bias"])
        return out, hn, cn

    @torch.no_grad()
    def log_probs(self, enc_row: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
        """joint(frame [E], predictor outputs [n, 1, P]).log_softmax(-1) -> [n, V], with the tensor shapes of
        forward_decoder_one_step (one frame [1, 1, E] against [n, 1, P]) so that the f32 roundings are the same."""
        lin = torch.nn.functional.linear
        e = lin(enc_row.reshape(1, 1, -1), self.sd["joint.enc_ffn.weight"], self.sd["joint.enc_ffn.bias"])
        p = lin(pred, self.sd["joint.pred_ffn.weight"], self.sd["joint.pred_ffn.bias"])
        z = torch.tanh(e.unsqueeze(2) + p.unsqueeze(1))
        out = lin(z, self.sd["joint.ffn_out.weight"], self.sd["joint.ffn_out.bias"]).log_softmax(dim=-1)
        return out.squeeze(1).squeeze(1)


def fuse_host(logp: torch.Tensor, ctc_row: Optional[torch.Tensor], ctc_weight: float, transducer_weight: float):
    """prefix_beam_search.py:95-100 in f32 (no CTC row: the second term is 0)."""
    second = ctc_weight * torch.exp(ctc_row.unsqueeze(0)) if ctc_row is not None else torch.zeros(1, 1)
    return torch.log(torch.add(transducer_weight * torch.exp(logp), second))


def _search_one_host(m: HostTransducer, enc: torch.Tensor, ctc: Optional[torch.Tensor], K: int, cw: float, tw: float):
    cfg = m.cfg
    T = enc.shape[0]
    hyps: List[Tuple[int, ...]] = [()]
    scores, times = [0.0], [()]
    sl = cfg.stateless
    if sl:
        hist = [(-1,) * cfg.history_size]   # per hypothesis the ids before its last token
    else:
        h = torch.zeros(cfg.num_layers, 1, cfg.hidden)
        c = torch.zeros(cfg.num_layers, 1, cfg.hidden)
    tr = {"parent": np.full((T, K), -1, np.int32), "token": np.full((T, K), -1, np.int32),
          "score": np.zeros((T, K), np.float64), "topv": np.zeros((T, K, K), np.float32),
          "topi": np.full((T, K, K), -1, np.int32), "n": np.zeros(T, np.int32)}
    margin, fusions = math.inf, 0
    for t in range(T):
        last = [hyp[-1] if hyp else cfg.blank for hyp in hyps]
        if sl:
            wins = [hs + (tk,) for hs, tk in zip(hist, last)]
            pred = m.step_windows(wins)
        else:
            pred, hn, cn = m.step(last, h, c)
        fused = fuse_host(m.log_probs(enc[t], pred), ctc[t] if ctc is not None else None, cw, tw).numpy()
        topv, topi = topk_rows_host(fused, K)
        n = len(hyps)
        kept, gap = beam_step_host(hyps, scores, topv, topi, K, cfg.blank)
        margin = min(margin, gap)
        # (b) a token just outside a hypothesis' top K that would have come within 1.0 of the last kept score
        if fused.shape[1] > K:
            srt = -np.sort(-fused, axis=1)
            sc32 = np.asarray(scores, dtype=np.float64).astype(np.float32)
            for j in range(n):
                if float(sc32[j] + srt[j, K]) > kept[-1][1] - 1.0:
                    margin = min(margin, float(srt[j, K - 1] - srt[j, K]))
        fusions += n * K - len({(tuple(hyps[j]) if int(topi[j, q]) == cfg.blank else tuple(hyps[j]) + (int(topi[j, q]),))
                                for j in range(n) for q in range(K)})
        tr["topv"][t, :n], tr["topi"][t, :n], tr["n"][t] = topv, topi, len(kept)
        for r, (hyp, s, par, u, app) in enumerate(kept):
            tr["parent"][t, r], tr["token"][t, r], tr["score"][t, r] = par, u, s
        if sl:   # a token extension shifts the window by the parent's last token, a blank keeps it
            hist = [wins[k[2]][1:] if k[4] else hist[k[2]] for k in kept]
        else:
            par = torch.as_tensor([k[2] for k in kept], dtype=torch.long)
            app = torch.as_tensor([k[4] for k in kept]).view(1, -1, 1)
            h = torch.where(app, hn[:, par], h[:, par])
            c = torch.where(app, cn[:, par], c[:, par])
        times = [times[k[2]] + (t,) if k[4] else times[k[2]] for k in kept]
        hyps, scores = [k[0] for k in kept], [k[1] for k in kept]
    res = DecodeResult(list(hyps[0]), scores[0], times=list(times[0]), nbest=[list(x) for x in hyps],
                       nbest_scores=list(scores), nbest_times=[list(x) for x in times])
    res.trace, res.margin, res.fusions = tr, margin, fusions
    return res


def prefix_beam_search_host(model, enc_rows: torch.Tensor, ctc_logp: Optional[torch.Tensor], row_start, row_len,
                            beam_size: int = 5, ctc_weight: float = 0.3, transducer_weight: float = 0.7,
                            return_trace: bool = False) -> List[DecodeResult]:
    """The search restated on the CPU over a HostTransducer (or a (RNNTConfig, state_dict) pair): RNNTBeamSearch.
    search_packed's arguments and results.  Every result also carries `trace` (per frame the kept beam's parent slot /
    token / score, each hypothesis' top-K fused values and ids, the count), `margin` (the smallest decision gap of the
    search: adjacent candidates among ranks 0 .. K, and a hypothesis' K-th against (K+1)-th fused log-prob where the
    latter would have come within 1.0 of the last kept score) and `fusions` (prefix fusions that occurred)."""
    m = model if isinstance(model, HostTransducer) else HostTransducer(*model)
    enc = torch.as_tensor(enc_rows, dtype=torch.float32).reshape(-1, m.cfg.enc_dim).cpu()
    ctc = None if ctc_logp is None else torch.as_tensor(ctc_logp, dtype=torch.float32).cpu()
    ctc_weight, transducer_weight = float(ctc_weight), float(transducer_weight)
    _check_args(beam_size, m.cfg.vocab, ctc_weight, transducer_weight, ctc is not None)
    if ctc is not None and tuple(ctc.shape) != (enc.shape[0], m.cfg.vocab):
        raise ValueError("ctc_logp must be [rows, vocab]")
    from . import _lib
    rs, rl = (t.tolist() for t in _lib.packed_ranges(row_start, row_len, enc.shape[0], "encoder rows"))
    use_ctc = ctc is not None and ctc_weight > 0
    del return_trace   # the host search always records it
    return [_search_one_host(m, enc[s: s + n], ctc[s: s + n] if use_ctc else None, int(beam_size), ctc_weight,
                             transducer_weight) for s, n in zip(rs, rl)]


@torch.no_grad()
def greedy_host(model, enc_rows: torch.Tensor, row_start, row_len, n_steps: int = 64):
    """basic_greedy_search (transducer/search/greedy_search.py) per utterance of a packed batch over a HostTransducer (or
    a (RNNTConfig, state_dict) pair), any predictor kind: the predictor is re-evaluated only after a non-blank decision
    and a frame ends on blank or after n_steps non-blanks.  Returns (dense [rows, n_steps] int32 as
    RNNTGreedy.greedy_packed, the smallest top-1 - top-2 logit gap over all decisions)."""
    m = model if isinstance(model, HostTransducer) else HostTransducer(*model)
    cfg = m.cfg
    enc = torch.as_tensor(enc_rows, dtype=torch.float32).reshape(-1, cfg.enc_dim).cpu()
    from . import _lib
    rs, rl = (t.tolist() for t in _lib.packed_ranges(row_start, row_len, enc.shape[0], "encoder rows"))
    lin = torch.nn.functional.linear
    dense = np.zeros((enc.shape[0], int(n_steps)), np.int32)
    gap = math.inf
    for s, n in zip(rs, rl):
        if cfg.stateless:
            win = (-1,) * cfg.history_size + (cfg.blank,)
            pred = m.step_windows([win])
        else:
            h = torch.zeros(cfg.num_layers, 1, cfg.hidden)
            c = torch.zeros(cfg.num_layers, 1, cfg.hidden)
            pred, hn, cn = m.step([cfg.blank], h, c)
        for t in range(n):
            e = lin(enc[s + t].reshape(1, 1, -1), m.sd["joint.enc_ffn.weight"], m.sd["joint.enc_ffn.bias"])
            for step in range(int(n_steps)):
                p = lin(pred, m.sd["joint.pred_ffn.weight"], m.sd["joint.pred_ffn.bias"])
                logits = lin(torch.tanh(e + p), m.sd["joint.ffn_out.weight"], m.sd["joint.ffn_out.bias"]).reshape(-1)
                top = torch.topk(logits, 2).values
                gap = min(gap, float(top[0] - top[1]))
                k = int(torch.argmax(logits))
                if k == cfg.blank:
                    break
                dense[s + t, step] = k
                if cfg.stateless:
                    win = win[1:] + (k,)
                    pred = m.step_windows([win])
                else:
                    h, c = hn, cn
                    pred, hn, cn = m.step([k], h, c)
    return dense, gap


# ----------------------------------------------------------------------------- the device search
class RNNTBeamSearch:
    """cfm_rnnt_beam_search over an RNNTGreedy's handle (no second handle, no second upload from Python)."""

    def __init__(self, rnnt):
        self.rnnt = rnnt
        self.cfg = rnnt.cfg
        self.device = rnnt.device
        self.last_error = 0   # the device's error word of the last search (4: a NaN score was ranked as -inf)

    @torch.no_grad()
    def search_packed(self, enc_rows: torch.Tensor, ctc_logp: Optional[torch.Tensor], row_start, row_len,
                      beam_size: int = 5, ctc_weight: float = 0.3, transducer_weight: float = 0.7,
                      return_trace: bool = False) -> List[DecodeResult]:
        """Utterance b = rows [row_start[b], + row_len[b]) of enc_rows [rows, enc_dim]; ctc_logp [rows, vocab] f32
        (encoder.ctc_log_softmax) or None with ctc_weight 0.  One DecodeResult per utterance: tokens, score, times (the
        frame at which each token was appended) and the final beam as nbest / nbest_scores / nbest_times; with
        `return_trace` also `trace` (parent / token / score [T, K], topv / topi [T, K, K] per utterance)."""
        from . import _lib
        cfg, dev = self.cfg, self.device
        K = int(beam_size)
        ctc_weight, transducer_weight = float(ctc_weight), float(transducer_weight)
        _check_args(K, cfg.vocab, ctc_weight, transducer_weight, ctc_logp is not None)
        enc = enc_rows.reshape(-1, cfg.enc_dim).to(dev, torch.float32).contiguous()
        rows = enc.shape[0]
        rs, rl = _lib.packed_ranges(row_start, row_len, rows, "encoder rows")
        B = rs.numel()
        ctc = None
        if ctc_logp is not None and ctc_weight > 0:
            ctc = ctc_logp.reshape(-1, ctc_logp.shape[-1]).to(dev, torch.float32).contiguous()
            if tuple(ctc.shape) != (rows, cfg.vocab):
                raise ValueError("ctc_logp must be [rows, vocab]")
        if B == 0:
            return []
        i32 = dict(dtype=torch.int32, device=dev)
        out_tok = torch.zeros(K, max(rows, 1), **i32)
        out_time = torch.zeros(K, max(rows, 1), **i32)
        out_len = torch.zeros(B, K, **i32)
        out_score = torch.zeros(B, K, dtype=torch.float64, device=dev)
        n_hyps = torch.zeros(B, **i32)
        tr = None
        if return_trace:
            r1 = max(rows, 1)
            tr = (torch.empty(r1, K, **i32), torch.empty(r1, K, **i32), torch.empty(r1, K, dtype=torch.float64, device=dev),
                  torch.empty(r1, K, K, dtype=torch.float32, device=dev), torch.empty(r1, K, K, **i32))
        nbytes = int(_lib.cfm_rnnt_beam_workspace_bytes(self.rnnt._h, rows, B, K))
        if nbytes == 0:
            raise ValueError("rnnt beam search: rows / utterances / beam outside what the workspace can hold")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rs_d, rl_d = rs.to(dev), rl.to(dev)
        tp = [t.data_ptr() for t in tr] if tr else [0] * 5
        with torch.cuda.device(dev):
            _lib.check(_lib.cfm_rnnt_beam_search(
                self.rnnt._h, enc.data_ptr(), rows, _lib.ptr(ctc), rs_d.data_ptr(), rl_d.data_ptr(), B, int(rl.max()), K,
                ctc_weight, transducer_weight, out_tok.data_ptr(), out_time.data_ptr(), out_len.data_ptr(),
                out_score.data_ptr(), n_hyps.data_ptr(), *tp, ws.data_ptr(), nbytes,
                torch.cuda.current_stream(dev).cuda_stream))
            host = [t.cpu() for t in (out_tok, out_time, out_len, out_score, n_hyps)]   # (synchronises the stream)
            self.last_error = int(_lib.cfm_rnnt_beam_error(ws.data_ptr()))
        if self.last_error not in (0, 4):
            raise RuntimeError(f"rnnt beam search: device error word {self.last_error}")
        results = nbest_results(*host, rs)
        if tr:
            tr_h = [t.cpu().numpy() for t in tr]
            for res, s, n in zip(results, rs.tolist(), rl.tolist()):
                res.trace = {k: v[s: s + n] for k, v in zip(("parent", "token", "score", "topv", "topi"), tr_h)}
        return results

    # ---- the single kernels (include/cfm_ops.h), for the op tests and tools
    @torch.no_grad()
    def lstm_step(self, tokens: torch.Tensor, h: torch.Tensor, c: torch.Tensor):
        """tokens [R], h / c [layers, R, hidden] -> (h', c', pred_ffn(projection(h'_top)) [R, join_dim])."""
        from . import _lib
        cfg, dev = self.cfg, self.device
        R = int(tokens.numel())
        tok = tokens.to(dev, torch.int32).contiguous()
        h = h.to(dev, torch.float32).contiguous()
        c = c.to(dev, torch.float32).contiguous()
        if tuple(h.shape) != (cfg.num_layers, R, cfg.hidden) or h.shape != c.shape:
            raise ValueError("h / c must be [layers, R, hidden]")
        ho, co = torch.empty_like(h), torch.empty_like(c)
        pj = torch.empty(R, cfg.join_dim, dtype=torch.float32, device=dev)
        nbytes = int(_lib.cfm_op_rnnt_lstm_step_workspace_bytes(self.rnnt._h, R))
        ws = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.cfm_op_rnnt_lstm_step(self.rnnt._h, tok.data_ptr(), h.data_ptr(), c.data_ptr(), R,
                                                  ho.data_ptr(), co.data_ptr(), pj.data_ptr(), ws.data_ptr(), nbytes,
                                                  torch.cuda.current_stream(dev).cuda_stream))
            torch.cuda.current_stream(dev).synchronize()
        return ho, co, pj

    @torch.no_grad()
    def predictor_step(self, tokens_ctx):
        """cfm_op_rnnt_predictor_step (a stateless handle): id windows [R, history_size + 1] (oldest first, -1 = before
        the sos) -> (predictor output [R, embed_size], its pred_ffn projection [R, join_dim]) on the device."""
        from . import _lib
        cfg, dev = self.cfg, self.device
        win = tokens_ctx if isinstance(tokens_ctx, torch.Tensor) else torch.as_tensor(np.asarray(tokens_ctx))
        win = win.reshape(-1, cfg.context).to(dev, torch.int32).contiguous()
        R = int(win.shape[0])
        y = torch.empty(R, cfg.embed_size, dtype=torch.float32, device=dev)
        pj = torch.empty(R, cfg.join_dim, dtype=torch.float32, device=dev)
        nbytes = int(_lib.cfm_op_rnnt_predictor_step_workspace_bytes(self.rnnt._h, R))
        ws = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.cfm_op_rnnt_predictor_step(self.rnnt._h, win.data_ptr(), R, y.data_ptr(), pj.data_ptr(),
                                                       ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream))
            torch.cuda.current_stream(dev).synchronize()
        return y, pj


@torch.no_grad()
def fused_topk_device(logits: torch.Tensor, ctc_logp: Optional[torch.Tensor], k: int, ctc_weight: float,
                      transducer_weight: float):
    """cfm_op_rnnt_fused_topk: logits [R, V] f32 on the device (ctc_logp [R, V] or None) -> values [R, k] f32, ids
    [R, k] int32 of log(tw * softmax + cw * exp(ctc)) by value descending, index ascending."""
    from . import _lib
    dev = logits.device
    x = logits.to(torch.float32).contiguous()
    R, V = x.shape
    c = None if ctc_logp is None else ctc_logp.to(dev, torch.float32).contiguous()
    if c is not None and c.shape != x.shape:
        raise ValueError("ctc_logp must match the logits")
    vals = torch.empty(R, int(k), dtype=torch.float32, device=dev)
    ids = torch.empty(R, int(k), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.cfm_op_rnnt_fused_topk(x.data_ptr(), _lib.ptr(c), R, V, int(k), float(ctc_weight),
                                               float(transducer_weight), vals.data_ptr(), ids.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.current_stream(dev).synchronize()
    return vals, ids


@torch.no_grad()
def beam_prune_device(topv: torch.Tensor, topi: torch.Tensor, blank: int = 0):
    """cfm_op_rnnt_beam_prune: T frames of the expand / fuse / prune step of one utterance from the start state;
    topv / topi [T, K, K] on the device -> (parent [T, K], token [T, K], score [T, K] f64, count [T]) on the host."""
    from . import _lib
    dev = topv.device
    T, K, _ = topv.shape
    v = topv.to(torch.float32).contiguous()
    i = topi.to(dev, torch.int32).contiguous()
    par = torch.empty(max(T, 1), K, dtype=torch.int32, device=dev)
    tok = torch.empty(max(T, 1), K, dtype=torch.int32, device=dev)
    sc = torch.empty(max(T, 1), K, dtype=torch.float64, device=dev)
    n = torch.zeros(max(T, 1), dtype=torch.int32, device=dev)
    nbytes = int(_lib.cfm_op_rnnt_beam_prune_workspace_bytes(T, K))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.cfm_op_rnnt_beam_prune(v.data_ptr(), i.data_ptr(), T, K, int(blank), par.data_ptr(),
                                               tok.data_ptr(), sc.data_ptr(), n.data_ptr(), ws.data_ptr(), nbytes,
                                               torch.cuda.current_stream(dev).cuda_stream))
        out = (par[:T].cpu().numpy(), tok[:T].cpu().numpy(), sc[:T].cpu().numpy(), n[:T].cpu().numpy())
        err = int(_lib.cfm_rnnt_beam_error(ws.data_ptr()))
    if err not in (0, 4):
        raise RuntimeError(f"beam prune: device error word {err}")
    return out
