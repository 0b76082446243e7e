"""Generate tests/golden/rnnt_stateless.npz from the REFERENCE's stateless transducer predictors (CPU).

Runs only where the reference checkout is available (CHUNKFORMER_REF, default: the directory gen_golden_beam.py
uses); it imports the reference through the namespace shim, the empty `torchaudio` stub and the three adapters of
gen_golden_rnnt_beam.py (a predictor wrapper that drops the stray `padding` argument, an encoder stub, a CTC stub).

    python tests/golden/gen_golden_stateless.py

Recipe: the reference's EmbeddingPredictor, ConvPredictor, TransducerJoint, basic_greedy_search and
PrefixBeamSearch.prefix_beam_search run unmodified, loaded with the weights of
chunkformer_amd.transducer.synthetic_transducer_state_dict; the full-sum scores come from the reference's
Transducer._cal_transducer_score (predictor `forward`, joint) on a small object that carries what it reads, with
the rnnt_loss stand-in of gen_golden_td_rescore.py's kind (torchaudio is not installed: log-softmax in f64 and the
restatement's recursion -- the reference pins the predictor / joint inputs, not the loss recursion).  Nothing of the
reference's text is copied; only arrays are stored.

Models (enc_dim 32), per kind `embedding` and `conv`: v17 (V 17, history 0, width 32), v37 (37, 2, 32), v130 (130, 4,
64), v1024 (1024, 1, 64); n_head 1 and 4, conv bias on and off, the four activations, one model with ln_eps 1e-3 and
one embedding model whose pos_embed has a bias (which the reference never reads).  Encoder rows are k / 64, k int8.

Stored per model:
  - `win`: id windows [n, K] (-1 = before the sos) -- the progression from the sos, then seeded full windows -- with the
    reference's f32 forward_step outputs `pred` [n, E] and `e_ref` = max |pred - f64 restatement| (the reference's own
    f32 error: the bar of the device's op test is 4 e_ref); `forward` (the training form) is asserted equal to them;
  - greedy cases (rows 1, 7, 33, 48 and a packed batch of 3 uneven utterances, n_steps 1 and 4): the reference's token
    list per utterance, the restatement's dense decisions and its smallest top-1 - top-2 logit gap;
  - beam cases (rows, beam, (ctc_weight, transducer_weight)): the reference's final beam, the restatement's trace, its
    margin and fusions, and the td / totals / choice of rescore_host (no decoder, weights 0.5 / 0 / 0.5) over that beam;
  - td cases: hypotheses with 0, 1, K - 1, K and K + 1 tokens packed back to back, the reference's td per hypothesis
    and the restatement's (f64).

Conditions (seeds advance until they hold, the number of tries is bounded and asserted):
  - per model the greedy decisions (48 rows, n_steps 4) contain blank-only frames, a frame with 1 - 3 tokens ended by a
    blank and a frame that hits the n_steps cap;
  - every greedy decision has a logit gap >= 1e-3, and the restatement's decisions flatten to the reference's list;
  - the restatement reproduces the reference's whole final beam (tokens equal, scores within 1e-9) in every beam case;
    every case meant for token equality has margin >= 2 (rows + 1) DEV, DEV = 1e-5;
  - at least 3 token-equality beam cases with a prefix fusion per kind;
  - the reference's td is within (T + U + 1) * 1e-5 of the restatement's.

The archive is written with fixed zip timestamps so that it regenerates bit-identically.
"""
from __future__ import annotations

import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import gen_golden_rnnt_beam as GB  # noqa: E402  (the shim, the stub and the adapters)
from chunkformer.transducer.joint import TransducerJoint  # noqa: E402
from chunkformer.transducer.predictor import ConvPredictor, EmbeddingPredictor  # noqa: E402
from chunkformer.transducer.search.greedy_search import basic_greedy_search  # noqa: E402
from chunkformer.transducer.search.prefix_beam_search import PrefixBeamSearch  # noqa: E402
from chunkformer.transducer.transducer import Transducer  # noqa: E402

from chunkformer_amd import transducer_beam as TB  # noqa: E402
from chunkformer_amd import transducer_rescore as TR  # noqa: E402
from chunkformer_amd.transducer import RNNTConfig, synthetic_transducer_state_dict  # noqa: E402

torch.set_num_threads(4)
OUT = os.path.join(HERE, "rnnt_stateless.npz")
DEV = 1e-5
GAP = 1e-3
WEIGHTS = ((0.3, 0.7), (0.0, 1.0), (1.0, 0.0))
BLANK_BIAS = {"v17": 3.72, "v37": 3.72, "v130": 3.72, "v1024": 7.0}
CTC_ROWS = 48


def _cfg(vocab, hist, width, **kw):
    return dict(vocab=vocab, enc_dim=32, embed_size=width, hidden=0, num_layers=0, pred_out=width, join_dim=width,
                history_size=hist, **kw)


MODELS = {
    # name: (RNNTConfig kwargs, first weight seed)
    "emb_v17": (_cfg(17, 0, 32, predictor="embedding", n_head=1, activation="tanh"), 0),
    "emb_v37": (_cfg(37, 2, 32, predictor="embedding", n_head=4, activation="swish", pos_bias=True), 0),
    "emb_v130": (_cfg(130, 4, 64, predictor="embedding", n_head=4, activation="gelu", ln_eps=1e-3), 0),
    "emb_v1024": (_cfg(1024, 1, 64, predictor="embedding", n_head=1, activation="relu"), 0),
    "conv_v17": (_cfg(17, 0, 32, predictor="conv", activation="gelu"), 0),
    "conv_v37": (_cfg(37, 2, 32, predictor="conv", activation="relu", conv_bias=True), 0),
    "conv_v130": (_cfg(130, 4, 64, predictor="conv", activation="swish"), 0),
    "conv_v1024": (_cfg(1024, 1, 64, predictor="conv", activation="tanh", conv_bias=True), 0),
}
# greedy: (rows per utterance, n_steps)
GREEDY = [([48], 4), ([48], 1), ([33], 4), ([7], 4), ([7], 1), ([1], 4), ([1], 1), ([7, 33, 1], 4), ([33, 1, 7], 1)]
# beam: (rows, beam, index into WEIGHTS, token equality asked)
BEAM = {
    17: [(1, 16, 0, True), (7, 16, 0, True), (7, 16, 1, True), (7, 16, 2, True), (33, 5, 0, True), (33, 5, 1, True),
         (48, 1, 0, True), (33, 16, 0, False)],
    0: [(1, 1, 1, True), (1, 5, 0, True), (7, 5, 0, True), (7, 16, 0, True), (7, 1, 2, True), (33, 5, 0, True),
        (33, 5, 1, True), (33, 1, 0, True), (33, 5, 2, True), (48, 5, 0, True), (33, 16, 0, False)],
}


def rnnt_loss_stand_in(logits, targets, logit_lengths, target_lengths, blank=-1, reduction="none", **kw):
    """-td of each hypothesis from the reference's joint tensor [n, T, U + 1, V]: log-softmax in f64, then the
    restatement's recursion.  NOT torchaudio's loss: its parity is unpinned."""
    lp = logits.double().log_softmax(-1)
    out = []
    for i in range(lp.shape[0]):
        T, U = int(logit_lengths[i]), int(target_lengths[i])
        b = lp[i, :T, : U + 1, blank]
        k = lp[i, :T, :U].gather(-1, targets[i, :U].long().view(1, U, 1).expand(T, U, 1))[..., 0]
        out.append(-TR.td_score_host(b.numpy(), k.numpy().reshape(T, U)))
    return torch.tensor(out, dtype=torch.float64)


sys.modules["torchaudio"].functional.rnnt_loss = rnnt_loss_stand_in


class RefModel:
    """What basic_greedy_search and Transducer._cal_transducer_score read of a Transducer."""
    ignore_id = -1
    _cal_transducer_score = Transducer._cal_transducer_score

    def __init__(self, cfg, pred, joint):
        self.blank, self.predictor, self.joint = cfg.blank, pred, joint


def ref_modules(cfg: RNNTConfig, sd):
    bias = cfg.conv_bias or cfg.pos_bias
    if cfg.predictor == "embedding":
        pred = EmbeddingPredictor(cfg.vocab, cfg.embed_size, cfg.pred_out, 0.0, cfg.n_head, cfg.history_size, cfg.act,
                                  bias, cfg.ln_eps)
    else:
        pred = ConvPredictor(cfg.vocab, cfg.embed_size, cfg.pred_out, 0.0, cfg.history_size, cfg.act, bias, cfg.ln_eps)
    joint = TransducerJoint(cfg.vocab, cfg.enc_dim, cfg.pred_out, cfg.join_dim)
    pred.load_state_dict({k[len("predictor."):]: v for k, v in sd.items() if k.startswith("predictor.")}, strict=True)
    joint.load_state_dict({k[len("joint."):]: v for k, v in sd.items() if k.startswith("joint.")}, strict=True)
    return pred.eval(), joint.eval()


def enc_rows(cfg, rows, seed):
    g = np.random.default_rng(seed)
    q = g.integers(-128, 128, size=(rows, cfg.enc_dim), dtype=np.int64).astype(np.int8)
    return q, torch.from_numpy(q.astype(np.float32) / 64.0)


@torch.no_grad()
def predictor_points(cfg, pred, host, seed):
    """The id windows, the reference's f32 forward_step outputs on them and its own error against the f64 restatement."""
    K = cfg.context
    g = np.random.default_rng(seed)
    seq = g.integers(1, cfg.vocab, size=K + 3).tolist()
    wins = TB.hyp_windows(cfg, seq).tolist()                       # from the sos on: windows that start before it
    wins += g.integers(0, cfg.vocab, size=(24, K)).tolist()        # full windows, the blank among the ids
    wins = np.array(wins, np.int64).reshape(-1, K)
    emb = pred.embed.weight
    outs = []
    for w in wins:
        hist = torch.stack([emb[i] if i >= 0 else torch.zeros(cfg.embed_size) for i in w[:-1]]).reshape(1, K - 1, -1) \
            if K > 1 else torch.zeros(1, 0, cfg.embed_size)
        out, cache = pred.forward_step(torch.tensor([[int(w[-1])]]), [hist])
        outs.append(out.reshape(-1))
    ref = torch.stack(outs)
    # the training form over the sos progression gives the same values
    fwd = pred(torch.tensor([[cfg.blank] + seq]))[0]
    assert torch.allclose(fwd, ref[: len(seq) + 1], rtol=0, atol=2e-6), float((fwd - ref[: len(seq) + 1]).abs().max())
    f64 = host.predict_windows(wins, torch.float64)
    e_ref = float((ref.double() - f64).abs().max())
    assert torch.equal(host.step_windows(wins).reshape(ref.shape), ref) or \
        float((host.step_windows(wins).reshape(ref.shape) - ref).abs().max()) <= 1e-6
    assert 0 < e_ref < 1e-5, e_ref
    return wins, ref.numpy(), e_ref


@torch.no_grad()
def greedy_case(cfg, ref, host, lens, n_steps, seed):
    rows = sum(lens)
    q, enc = enc_rows(cfg, rows, seed)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int).tolist()
    dense, gap = TB.greedy_host(host, enc, starts, lens, n_steps)
    if not gap >= GAP:
        return None
    toks = []
    for s, n in zip(starts, lens):
        got = basic_greedy_search(ref, enc[s: s + n].unsqueeze(0), torch.tensor(n), n_steps)[0]
        mine = dense[s: s + n].reshape(-1)
        assert [int(t) for t in got] == mine[mine != cfg.blank].tolist(), "greedy restatement differs from the reference"
        toks.append([int(t) for t in got])
    return dict(seed=seed, lens=list(lens), n_steps=n_steps, enc_q=q, tokens=toks, dense=dense, gap=float(gap))


def frame_mix(dense, n_steps):
    cnt = (dense != 0).sum(1)
    return int((cnt == 0).sum()), int(((cnt >= 1) & (cnt <= min(3, n_steps - 1))).sum()), int((cnt == n_steps).sum())


@torch.no_grad()
def beam_case(cfg, pred, joint, host, ctc_all, rows, beam, cw, tw, seed, equality):
    q, enc = enc_rows(cfg, rows, seed)
    ctc_off = seed % ctc_all.shape[0]
    ctc = torch.roll(ctc_all, -ctc_off, 0)[:rows].contiguous()
    bs = PrefixBeamSearch(GB.EncoderStub(), GB.PredictorAdapter(pred), joint, GB.CtcStub(ctc), cfg.blank)
    ref_beam, _ = bs.prefix_beam_search(enc.unsqueeze(0), torch.tensor([rows]), beam_size=beam, ctc_weight=cw,
                                        transducer_weight=tw)
    ref_tok = [[int(t) for t in s.hyp[1:]] for s in ref_beam]
    ref_sc = [float(s.score) for s in ref_beam]
    res = TB.prefix_beam_search_host(host, enc, ctc, [0], [rows], beam, cw, tw)[0]
    assert res.nbest == ref_tok and np.allclose(res.nbest_scores, ref_sc, rtol=0, atol=1e-9), \
        "beam restatement differs from the reference"
    if equality and not res.margin >= 2 * (rows + 1) * DEV:
        return None
    return dict(seed=seed, ctc_off=ctc_off, rows=rows, beam=beam, cw=cw, tw=tw, equality=equality, enc_q=q, tokens=ref_tok,
                scores=ref_sc, trace=res.trace, margin=float(min(res.margin, 1e30)), fusions=int(res.fusions), res=res,
                enc=enc)


@torch.no_grad()
def td_case(cfg, ref, host, rows, seed):
    """Hypotheses with 0, 1, K - 1, K, K + 1 tokens, packed back to back by the tests in this order."""
    K = cfg.context
    g = np.random.default_rng(seed)
    q, enc = enc_rows(cfg, rows, seed)
    lens = [0, 1, K - 1, K, K + 1]
    hyps = [g.integers(1, cfg.vocab, size=n).tolist() for n in lens]
    n, U = len(hyps), max(lens)
    pad = torch.full((n, U), -1, dtype=torch.long)
    for i, h in enumerate(hyps):
        pad[i, : len(h)] = torch.tensor(h, dtype=torch.long)
    td_ref = ref._cal_transducer_score(enc.unsqueeze(0).repeat(n, 1, 1), torch.ones(n, 1, rows, dtype=torch.bool),
                                       torch.tensor(lens), pad).tolist()
    td = [TR.td_score_host(*TR.lattice_logp_host(host, enc, h, torch.float64)) for h in hyps]
    for a, b, h in zip(td_ref, td, hyps):
        assert abs(a - b) <= (rows + len(h) + 1) * 1e-5, (a, b)
    return dict(seed=seed, rows=rows, enc_q=q, hyps=hyps, td_ref=td_ref, td=td)


def build(name):
    kw, wseed0 = MODELS[name]
    cfg = RNNTConfig(**kw)
    vname = name.split("_")[1]
    # the weight seed advances until the greedy mix holds
    for wseed in range(wseed0, wseed0 + 12):
        sd = synthetic_transducer_state_dict(cfg, seed=wseed, blank_bias=BLANK_BIAS[vname])
        pred, joint = ref_modules(cfg, sd)
        host = TB.HostTransducer(cfg, sd)
        ref = RefModel(cfg, pred, joint)
        first = None
        for seed in range(1000 * wseed, 1000 * wseed + 6):
            first = greedy_case(cfg, ref, host, [48], 4, seed)
            if first is not None and min(frame_mix(first["dense"], 4)) >= 1:
                break
            first = None
        if first is not None:
            break
    assert first is not None, f"{name}: no weight seed gives the greedy mix"
    greedy = [first]
    seed = first["seed"] + 1
    for lens, n_steps in GREEDY[1:]:
        for _ in range(40):
            c = greedy_case(cfg, ref, host, lens, n_steps, seed)
            seed += 1
            if c is not None:
                break
        assert c is not None, (name, lens, n_steps)
        greedy.append(c)
    wins, pred_ref, e_ref = predictor_points(cfg, pred, host, 7000 + wseed)
    g = torch.Generator().manual_seed(1000 + wseed)
    ctc_all = (torch.randn(CTC_ROWS, cfg.vocab, generator=g) * 2.0).log_softmax(-1).to(torch.float32)
    beams = []
    seed = 50000 + 1000 * wseed
    for rows, beam, wi, equality in BEAM.get(cfg.vocab, BEAM[0]):
        cw, tw = WEIGHTS[wi]
        want_fusion = equality and rows >= 7 and beam >= 5 and tw > 0
        first_ok, c = None, None
        for _ in range(200):
            c = beam_case(cfg, pred, joint, host, ctc_all, rows, beam, cw, tw, seed, equality)
            seed += 1
            if c is None:
                continue
            first_ok = first_ok or c
            if not want_fusion or c["fusions"] > 0:
                break
        c = c if c is not None and (not want_fusion or c["fusions"] > 0) else first_ok
        assert c is not None, (name, rows, beam)
        got = TR.rescore_host(host, None, c["enc"], [0], [rows], [c["res"]], 0.5, 0.0, 0.5)[0]
        srt = sorted(got.nbest_scores, reverse=True)
        c.update(td=got.td_scores, totals=got.nbest_scores, best_index=int(got.best_index),
                 td_margin=float(srt[0] - srt[1]) if len(srt) > 1 else 1e30)
        beams.append(c)
    tds = [td_case(cfg, ref, host, rows, 90000 + 10 * wseed + i) for i, rows in enumerate((1, 7))]
    return cfg, wseed, dict(wins=wins, pred=pred_ref, e_ref=e_ref, ctc=ctc_all, greedy=greedy, beams=beams, tds=tds)


def main():
    arrays, meta = {}, {"dev": DEV, "gap": GAP, "models": {}}
    fus = {"embedding": 0, "conv": 0}
    for name in MODELS:
        cfg, wseed, d = build(name)
        vname = name.split("_")[1]
        mm = {"config": {k: getattr(cfg, k) for k in ("vocab", "enc_dim", "embed_size", "hidden", "num_layers", "pred_out",
                                                       "join_dim", "blank", "predictor", "history_size", "n_head",
                                                       "activation", "ln_eps", "conv_bias", "pos_bias")},
              "weight_seed": wseed, "blank_bias": BLANK_BIAS[vname], "e_ref": d["e_ref"], "greedy": [], "beam": [], "td": []}
        p = name + "/"
        arrays[p + "win"] = d["wins"].astype(np.int16)
        arrays[p + "pred"] = d["pred"].astype(np.float32)
        arrays[p + "ctc"] = d["ctc"].numpy()
        for i, c in enumerate(d["greedy"]):
            q = f"{p}g{i}/"
            mm["greedy"].append({"lens": c["lens"], "n_steps": c["n_steps"], "seed": c["seed"], "gap": c["gap"]})
            arrays[q + "enc_q"] = c["enc_q"]
            arrays[q + "dense"] = c["dense"].astype(np.int16)
            arrays[q + "ref_lens"] = np.array([len(t) for t in c["tokens"]], np.int32)
            arrays[q + "ref_tokens"] = np.array([t for h in c["tokens"] for t in h], np.int16)
        for i, c in enumerate(d["beams"]):
            q = f"{p}b{i}/"
            mm["beam"].append({k: c[k] for k in ("rows", "beam", "cw", "tw", "seed", "ctc_off", "equality", "margin", "fusions",
                                                 "best_index", "td_margin")})
            fus[cfg.predictor] += int(c["equality"] and c["fusions"] > 0)
            arrays[q + "enc_q"] = c["enc_q"]
            arrays[q + "lens"] = np.array([len(t) for t in c["tokens"]], np.int32)
            arrays[q + "tokens"] = np.array([t for h in c["tokens"] for t in h], np.int16)
            arrays[q + "scores"] = np.array(c["scores"], np.float64)
            arrays[q + "tr_parent"] = c["trace"]["parent"].astype(np.int8)
            arrays[q + "tr_token"] = c["trace"]["token"].astype(np.int16)
            arrays[q + "tr_score"] = c["trace"]["score"]
            arrays[q + "td"] = np.array(c["td"], np.float64)
            arrays[q + "totals"] = np.array(c["totals"], np.float64)
        for i, c in enumerate(d["tds"]):
            q = f"{p}t{i}/"
            mm["td"].append({"rows": c["rows"], "seed": c["seed"]})
            arrays[q + "enc_q"] = c["enc_q"]
            arrays[q + "lens"] = np.array([len(h) for h in c["hyps"]], np.int32)
            arrays[q + "tokens"] = np.array([t for h in c["hyps"] for t in h], np.int16)
            arrays[q + "td_ref"] = np.array(c["td_ref"], np.float64)
            arrays[q + "td"] = np.array(c["td"], np.float64)
        meta["models"][name] = mm
        print(name, "weight seed", wseed, "e_ref %.2e" % d["e_ref"], "greedy mix", frame_mix(d["greedy"][0]["dense"], 4),
              "min gap %.2e" % min(c["gap"] for c in d["greedy"]), "fusions", [c["fusions"] for c in d["beams"]])
    assert min(fus.values()) >= 3, fus
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 1000000


if __name__ == "__main__":
    main()
