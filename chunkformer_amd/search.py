"""CTC prefix beam search with n-best, token times and hotword biasing.

The semantics are the reference's `ctc_prefix_beam_search` (modules/search.py:131-249) with
`PrefixScore.score()` read as `log_add([s, ns])` (as shipped it calls `log_add(s, ns)` and raises), and
the Aho-Corasick `ContextGraph` of utils/context_graph.py.

Two implementations share one formulation:
  - device tensors: a per-frame top-k kernel followed by the beam kernel (csrc/ctc_beam.hip), one
    workgroup per utterance;
  - CPU tensors: `beam_search_topk_host`, a plain-Python restatement (the subject of the CPU tests).

Both identify a prefix by a canonical trie node: a map (parent node, token) -> node that lives for the
whole utterance, so that a prefix that leaves the beam and is created again gets its old node back
and still merges with its live descendants.  Viterbi times are persistent linked lists
(previous, frame): a copy shares a pointer, an append or a replace-last makes one node.
"""
from __future__ import annotations

import math
import re
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import torch

NEG_INF = float("-inf")
MAX_BEAM = 16


class DecodeResult:
    """The reference's DecodeResult (modules/search.py:33-64)."""

    def __init__(self, tokens: List[int], score: float = 0.0, confidence: float = 0.0,
                 tokens_confidence: Optional[List[float]] = None, times: Optional[List[int]] = None,
                 nbest: Optional[List[List[int]]] = None, nbest_scores: Optional[List[float]] = None,
                 nbest_times: Optional[List[List[int]]] = None):
        self.tokens = tokens
        self.score = score
        self.confidence = confidence
        self.tokens_confidence = tokens_confidence
        self.times = times
        self.nbest = nbest
        self.nbest_scores = nbest_scores
        self.nbest_times = nbest_times


def log_add2(a: float, b: float) -> float:
    """log(exp(a) + exp(b)) as the reference's log_add([a, b]) evaluates it."""
    if a == NEG_INF and b == NEG_INF:
        return NEG_INF
    m = a if a > b else b
    return m + math.log(0 + math.exp(a - m) + math.exp(b - m))


# ------------------------------------------------------------------------------------ context graph
_CJK = re.compile(r"([\u4e00-\u9fff])")


def _bpe_tokens(sp, text: str) -> List[str]:
    out: List[str] = []
    for part in _CJK.split(text):
        if not part.strip():
            continue
        if _CJK.fullmatch(part):
            out.append(part)
        else:
            out.extend(sp.encode_as_pieces(part))
    return out


class ContextGraph:
    """Aho-Corasick biasing graph over token-id phrases (utils/context_graph.py:105-272).

    Nodes are flat arrays indexed by node id, in the reference's creation order with the root as 0;
    a state is a node id.  As in the reference, a node is an end node (and carries an output score)
    only if a phrase ended there when the node was created."""

    def __init__(self, context_list: Sequence[Sequence[int]], context_score: float = 6.0):
        self.context_score = float(context_score)
        self.context_list = [[int(t) for t in p] for p in context_list]
        self.next: List[Dict[int, int]] = [{}]
        self.token = [-1]
        self.fail = [0]
        self.token_score = [0.0]
        self.node_score = [0.0]
        self.output_score = [0.0]
        self.is_end = [False]
        for phrase in self.context_list:
            node = 0
            for i, tok in enumerate(phrase):
                nxt = self.next[node].get(tok)
                if nxt is None:
                    nxt = len(self.token)
                    end = i == len(phrase) - 1
                    ns = self.node_score[node] + self.context_score
                    self.next[node][tok] = nxt
                    self.next.append({})
                    self.token.append(tok)
                    self.fail.append(0)
                    self.token_score.append(self.context_score)
                    self.node_score.append(ns)
                    self.output_score.append(ns if end else 0.0)
                    self.is_end.append(end)
                node = nxt
        self._fill_fail()
        self._tables = None
        self._dev_handles: Dict[Tuple[str, Optional[int]], "_DeviceContext"] = {}   # one cfm_ctx per device

    @property
    def root(self) -> int:
        return 0

    @property
    def num_nodes(self) -> int:
        return len(self.token) - 1

    @classmethod
    def from_file(cls, path: str, symbol_table: Dict[str, int], bpe_model: Optional[str] = None,
                  context_score: float = 6.0) -> "ContextGraph":
        """One phrase per line, tokenised per character (a space becomes "▁") or, with `bpe_model` (a
        sentencepiece model file), into BPE pieces; unknown tokens map to "<unk>" when the table has it
        and are dropped otherwise (utils/context_graph.py:25-59)."""
        sp = None
        if bpe_model is not None:
            try:
                import sentencepiece
            except ImportError as e:
                raise ImportError("a bpe_model needs the sentencepiece package") from e
            sp = sentencepiece.SentencePieceProcessor()
            sp.load(bpe_model)
        phrases = []
        with open(path, "r", encoding="utf-8") as f:
            for line in f:
                labels = []
                text = line.strip()
                # with a BPE model (text/tokenize_utils.py:26-63): every CJK ideograph is a token of its
                # own, the runs between them are encoded into pieces
                tokens = _bpe_tokens(sp, text) if sp is not None else ["▁" if ch == " " else ch for ch in text]
                for ch in tokens:
                    if ch in symbol_table:
                        labels.append(symbol_table[ch])
                    elif "<unk>" in symbol_table:
                        labels.append(symbol_table["<unk>"])
                phrases.append(labels)
        return cls(phrases, context_score)

    def _step_fail(self, node: int, tok: int) -> int:
        """Follow fail arcs from `node` until a node with a `tok` arc or the root; take the arc if any."""
        while tok not in self.next[node] and node != 0:
            node = self.fail[node]
        return self.next[node].get(tok, node)

    def _fill_fail(self) -> None:
        queue = list(self.next[0].values())
        head = 0
        while head < len(queue):
            cur = queue[head]
            head += 1
            for tok, node in self.next[cur].items():
                self.fail[node] = self._step_fail(self.fail[cur], tok)
                out = self.fail[node]
                while out != 0 and not self.is_end[out]:
                    out = self.fail[out]
                if out != 0:
                    self.output_score[node] += self.output_score[out]
                queue.append(node)

    def forward_one_step(self, state: int, token: int) -> Tuple[float, int]:
        """(bonus, next state) of context_graph.py:215-254."""
        nxt = self.next[state].get(token)
        if nxt is not None:
            return self.token_score[nxt] + self.output_score[nxt], nxt
        node = self._step_fail(self.fail[state], token)
        return (self.node_score[node] - self.node_score[state]) + self.output_score[node], node

    def finalize(self, state: int) -> Tuple[float, int]:
        return -self.node_score[state], 0

    def device_tables(self) -> Dict[str, torch.Tensor]:
        """Flat host arrays of cfm_ctx_create: per node fail / token_score / node_score / output_score,
        and the transitions (node, token, next) sorted by (node, token)."""
        if self._tables is None:
            tr = sorted((n, t, c) for n, d in enumerate(self.next) for t, c in d.items())
            self._tables = {
                "fail": torch.tensor(self.fail, dtype=torch.int32),
                "token_score": torch.tensor(self.token_score, dtype=torch.float64),
                "node_score": torch.tensor(self.node_score, dtype=torch.float64),
                "output_score": torch.tensor(self.output_score, dtype=torch.float64),
                "trans_node": torch.tensor([x[0] for x in tr], dtype=torch.int32),
                "trans_token": torch.tensor([x[1] for x in tr], dtype=torch.int32),
                "trans_next": torch.tensor([x[2] for x in tr], dtype=torch.int32),
            }
        return self._tables


# ------------------------------------------------------------------------------------ host fallback
def topk_host(logp: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row top-k of logp [rows, V] ordered by value descending, index ascending (a stable sort:
    ties are defined, unlike torch.topk)."""
    V = logp.shape[-1]
    _check_k(k, V)
    idx = torch.sort(logp, dim=-1, descending=True, stable=True).indices[..., :k]
    return torch.gather(logp, -1, idx), idx.to(torch.int32)


def _check_k(k: int, V: int) -> None:
    if not 1 <= k <= MAX_BEAM:
        raise ValueError(f"beam size {k}: 1 .. {MAX_BEAM}")
    if k > V:
        raise ValueError(f"beam size {k} exceeds the vocabulary ({V})")


class _Cand:
    __slots__ = ("node", "parent", "tok", "s", "ns", "v_s", "v_ns", "cur_p", "t_s", "t_ns", "ctx", "csc", "has_ctx")

    def __init__(self, node, parent, tok):
        self.node, self.parent, self.tok = node, parent, tok
        self.s = self.ns = self.v_s = self.v_ns = self.cur_p = NEG_INF
        self.t_s = self.t_ns = None      # linked lists (previous, frame); None = []
        self.ctx, self.csc, self.has_ctx = 0, 0.0, False

    def score(self):
        return log_add2(self.s, self.ns)

    def viterbi(self):
        return self.v_s if self.v_s > self.v_ns else self.v_ns

    def times(self):
        return self.t_s if self.v_s > self.v_ns else self.t_ns

    def total(self):
        return self.score() + self.csc


def _unlink(lst) -> List[int]:
    out = []
    while lst is not None:
        out.append(lst[1])
        lst = lst[0]
    return out[::-1]


def _search_one(vals: List[List[float]], ids: List[List[int]], k: int, blank: int,
                cg: Optional[ContextGraph], on_prune=None):
    """One utterance over its per-frame top-k lists; returns (nbest, scores, times).
    `on_prune(previous beam, ranked candidates, k, node_parent)` is called after every frame's sort."""
    node_parent, node_tok = [-1], [-1]          # canonical trie: node 0 = the empty prefix
    child: Dict[Tuple[int, int], int] = {}
    first = _Cand(0, -1, -1)
    first.s, first.v_s, first.v_ns = 0.0, 0.0, 0.0
    cur = [first]
    for t in range(len(vals)):
        nxt: Dict[object, _Cand] = {}           # key: node id, or (parent, token) for a new prefix

        def unchanged(h):
            c = nxt.get(h.node)
            if c is None:
                c = nxt[h.node] = _Cand(h.node, h.parent, h.tok)
            if cg is not None and not c.has_ctx:
                c.ctx, c.csc, c.has_ctx = h.ctx, h.csc, True
            return c

        def extended(h, u):
            n = child.get((h.node, u))
            key = (h.node, u) if n is None else n
            c = nxt.get(key)
            if c is None:
                c = nxt[key] = _Cand(n, h.node, u)
            if cg is not None and not c.has_ctx:
                bonus, c.ctx = cg.forward_one_step(h.ctx, u)
                c.csc, c.has_ctx = h.csc + bonus, True
            return c

        for u, p in zip(ids[t], vals[t]):
            for h in cur:
                if u == blank:
                    c = unchanged(h)
                    c.s = log_add2(c.s, h.score() + p)
                    c.v_s = h.viterbi() + p
                    c.t_s = h.times()
                elif u == h.tok:
                    c = unchanged(h)            # *uu -> *u
                    c.ns = log_add2(c.ns, h.ns + p)
                    if c.v_ns < h.v_ns + p:
                        c.v_ns = h.v_ns + p
                        if c.cur_p < p:
                            c.cur_p = p
                            c.t_ns = (h.t_ns[0], t)
                    c = extended(h, u)          # *u-u -> *uu
                    c.ns = log_add2(c.ns, h.s + p)
                    if c.v_ns < h.v_s + p:
                        c.v_ns, c.cur_p, c.t_ns = h.v_s + p, p, (h.t_s, t)
                else:
                    c = extended(h, u)
                    c.ns = log_add2(c.ns, h.score() + p)
                    if c.v_ns < h.viterbi() + p:
                        c.v_ns, c.cur_p, c.t_ns = h.viterbi() + p, p, (h.times(), t)
        prev = cur
        cands = list(nxt.values())
        totals = [c.total() for c in cands]
        if any(x != x for x in totals):   # NaN has no rank; the kernel sets its error word for the same
            raise RuntimeError(f"CTC beam search: a score is NaN at frame {t} (non-finite log-probs)")
        ranked = [cands[i] for i in sorted(range(len(cands)), key=totals.__getitem__, reverse=True)]
        cur = ranked[:k]
        if on_prune is not None:
            on_prune(prev, ranked, k, node_parent)
        for c in cur:
            if c.node is None:                  # survivors only: the map stays O(k) per frame
                c.node = len(node_parent)
                node_parent.append(c.parent)
                node_tok.append(c.tok)
                child[(c.parent, c.tok)] = c.node
    if cg is not None:
        for c in cur:
            c.csc, c.ctx = cg.finalize(c.ctx)
    nbest = []
    for c in cur:
        toks, n = [], c.node
        while n > 0:
            toks.append(node_tok[n])
            n = node_parent[n]
        nbest.append(toks[::-1])
    return nbest, [c.total() for c in cur], [_unlink(c.times()) for c in cur]


def beam_search_topk_host(topk_logp, topk_ids, row_start, row_len, beam_size: int,
                          context_graph: Optional[ContextGraph] = None, blank_id: int = 0) -> List[DecodeResult]:
    """The search over packed per-frame top-k rows [rows, k]: utterance b = rows
    [row_start[b], row_start[b] + row_len[b])."""
    vals = torch.as_tensor(topk_logp).to(torch.float32).cpu()
    ids = torch.as_tensor(topk_ids).cpu()
    k = int(beam_size)
    if vals.dim() != 2 or vals.shape != ids.shape or vals.shape[1] != k:
        raise ValueError("top-k arrays must be [rows, beam_size]")
    if not 1 <= k <= MAX_BEAM:
        raise ValueError(f"beam size {k}: 1 .. {MAX_BEAM}")
    from . import _lib
    rs, rl = _lib.packed_ranges(row_start, row_len, vals.shape[0], "top-k arrays")
    out = []
    for s0, n in zip(rs.tolist(), rl.tolist()):
        nbest, scores, times = _search_one(vals[s0:s0 + n].tolist(), ids[s0:s0 + n].tolist(), k, int(blank_id),
                                           context_graph)
        out.append(DecodeResult(tokens=nbest[0], score=scores[0], times=times[0], nbest=nbest, nbest_scores=scores,
                                nbest_times=times))
    return out


# ------------------------------------------------------------------------------------ device path
def nbest_results(tok, times, lens, scores, counts, row_start) -> List[DecodeResult]:
    """The packed n-best of a device search as DecodeResults, from host arrays: token and time planes [K, rows]
    (hypothesis n of utterance b at [n, row_start[b] : row_start[b] + lens[b][n]]; `times` None: no times), lengths and
    scores [B, K], hypotheses per utterance `counts` [B].  The first hypothesis is the result."""
    tok, lens, scores = torch.as_tensor(tok), torch.as_tensor(lens).tolist(), torch.as_tensor(scores).tolist()
    times = None if times is None else torch.as_tensor(times)
    out = []
    for b, (s0, n_hyp) in enumerate(zip(torch.as_tensor(row_start).tolist(), torch.as_tensor(counts).tolist())):
        nbest = [tok[n, s0:s0 + lens[b][n]].tolist() for n in range(n_hyp)]
        nbest_times = None if times is None else [times[n, s0:s0 + lens[b][n]].tolist() for n in range(n_hyp)]
        sc = scores[b][:n_hyp]
        out.append(DecodeResult(tokens=nbest[0], score=sc[0], times=None if times is None else nbest_times[0],
                                nbest=nbest, nbest_scores=sc, nbest_times=nbest_times))
    return out


class _DeviceContext:
    """cfm_ctx handle of a ContextGraph on one device (cached on the graph)."""

    def __init__(self, cg: ContextGraph, device: torch.device):
        import ctypes

        from . import _lib
        t = cg.device_tables()
        h = ctypes.c_void_p()
        _lib.check(_lib.cfm_ctx_create(len(cg.token), t["fail"].data_ptr(), t["token_score"].data_ptr(),
                                       t["node_score"].data_ptr(), t["output_score"].data_ptr(),
                                       t["trans_node"].numel(), t["trans_node"].data_ptr(),
                                       t["trans_token"].data_ptr(), t["trans_next"].data_ptr(),
                                       device.index if device.index is not None else torch.cuda.current_device(),
                                       ctypes.byref(h)))
        self.h = h
        weakref.finalize(self, _lib.cfm_ctx_destroy, h)


def _device_context(cg: Optional[ContextGraph], device: torch.device):
    if cg is None:
        return None
    key = (device.type, device.index)
    if key not in cg._dev_handles:
        cg._dev_handles[key] = _DeviceContext(cg, device)
    return cg._dev_handles[key]


def topk_logp_device(logp: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row top-k (value descending, index ascending) of device log-probs [rows, V]: the top-k
    kernel without the log-sum-exp."""
    from . import _lib
    V = logp.shape[-1]
    _check_k(k, V)
    x = logp.reshape(-1, V).to(torch.float32).contiguous()
    rows = x.shape[0]
    vals = torch.empty(rows, k, dtype=torch.float32, device=x.device)
    ids = torch.empty(rows, k, dtype=torch.int32, device=x.device)
    if rows:
        with torch.cuda.device(x.device):
            _lib.check(_lib.cfm_ctc_topk_logp(x.data_ptr(), rows, V, k, vals.data_ptr(), ids.data_ptr(),
                                              torch.cuda.current_stream(x.device).cuda_stream))
    return vals, ids


def beam_search_topk_device(topk_logp: torch.Tensor, topk_ids: torch.Tensor, row_start, row_len, beam_size: int,
                            context_graph: Optional[ContextGraph] = None, blank_id: int = 0,
                            with_times: bool = True, workspace_bytes: Optional[int] = None) -> List[DecodeResult]:
    """cfm_ctc_beam_search over packed device top-k rows [rows, k]; one device -> host copy of the
    compacted n-best.  `workspace_bytes` overrides the workspace size (tests)."""
    from . import _lib
    dev = topk_logp.device
    k = int(beam_size)
    if topk_logp.dim() != 2 or topk_logp.shape != topk_ids.shape or topk_logp.shape[1] != k:
        raise ValueError("top-k arrays must be [rows, beam_size]")
    vals = topk_logp.to(torch.float32).contiguous()
    ids = topk_ids.to(torch.int32).contiguous()
    rows = vals.shape[0]
    rs, rl = _lib.packed_ranges(row_start, row_len, rows, "top-k arrays")
    B = rs.numel()
    if B == 0:
        return []
    ctx = _device_context(context_graph, dev)
    n_ctx = 0 if context_graph is None else len(context_graph.token)
    need = int(_lib.cfm_ctc_beam_workspace_bytes(rows, B, k, int(with_times), n_ctx))
    nbytes = need if workspace_bytes is None else int(workspace_bytes)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    tok = torch.empty(k, max(rows, 1), dtype=torch.int32, device=dev)
    tim = torch.empty(k, max(rows, 1), dtype=torch.int32, device=dev) if with_times else None
    ln = torch.zeros(B, k, dtype=torch.int32, device=dev)
    sc = torch.zeros(B, k, dtype=torch.float64, device=dev)
    nh = torch.zeros(B, dtype=torch.int32, device=dev)
    rs_d, rl_d = rs.to(dev), rl.to(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.cfm_ctc_beam_search(vals.data_ptr(), ids.data_ptr(), rows, k, rs_d.data_ptr(), rl_d.data_ptr(),
                                            B, int(blank_id), None if ctx is None else ctx.h, tok.data_ptr(),
                                            _lib.ptr(tim), ln.data_ptr(), sc.data_ptr(), nh.data_ptr(), ws.data_ptr(),
                                            nbytes, torch.cuda.current_stream(dev).cuda_stream))
    err = int(ws[:4].view(torch.int32).item())
    if err != 0:
        what = {1: "an utterance's row range lies outside the top-k arrays",
                4: "a score is NaN (non-finite log-probs)"}.get(err, "internal pool overflow")
        raise RuntimeError(f"CTC beam search failed (error word {err}): {what}")
    return nbest_results(tok.cpu(), tim.cpu() if with_times else None, ln.cpu(), sc.cpu(), nh.cpu(), rs)


def ctc_prefix_beam_search(ctc_probs: torch.Tensor, ctc_lens, beam_size: int,
                           context_graph: Optional[ContextGraph] = None, blank_id: int = 0) -> List[DecodeResult]:
    """The reference's signature: ctc_probs [B, T, V] log-probs, ctc_lens [B].  Device tensors run the
    HIP kernels, CPU tensors the host fallback."""
    if ctc_probs.dim() != 3:
        raise ValueError("ctc_probs must be [B, T, V]")
    B, T, V = ctc_probs.shape
    k = int(beam_size)
    _check_k(k, V)
    lens = [int(v) for v in ctc_lens]
    if len(lens) != B or any(n < 0 or n > T for n in lens):
        raise ValueError("ctc_lens must hold B lengths in 0 .. T")
    starts = [b * T for b in range(B)]
    flat = ctc_probs.reshape(B * T, V)
    if ctc_probs.is_cuda:
        vals, ids = topk_logp_device(flat, k)
        return beam_search_topk_device(vals, ids, starts, lens, k, context_graph, blank_id)
    vals, ids = topk_host(flat.to(torch.float32), k)
    return beam_search_topk_host(vals, ids, starts, lens, k, context_graph, blank_id)
