"""Generate tests/golden/td_rescore.npz: transducer attention rescoring (the reference's modes
rnnt_beam_attn_rescoring / ctc_beam_td_attn_rescoring) over the models and recorded beams of rnnt_beam.npz (CPU).

Runs only where the reference checkout is available (CHUNKFORMER_REF, default: the directory gen_golden_beam.py
uses); it imports the reference through the namespace shim of gen_golden_rnnt_beam.py / gen_golden_rescore.py.

    python tests/golden/gen_golden_td_rescore.py

Recipe.  Every case of rnnt_beam.npz with 1 .. 70 rows gives one case here, alternately with the n-best of the
transducer beam search (the recorded final beam) and of the reference's own ctc_prefix_beam_search over the case's CTC
log-probs (with the score() fix of gen_golden_beam.py), with rescoring weights (ctc_weight, attn_weight,
transducer_weight) and a decoder cycling over the lists below.  The attention decoders are seeded
chunkformer_amd.rescore.synthetic_decoder_state_dict weights for an AEDConfig with the model's vocabulary and d_model
32 (= the fixture's enc_dim), 2 heads, ff 64, `transformer` (1 block) and `bitransformer` (1 + 1 blocks).

Where the reference can run (a full beam: it asserts len(hyps) == beam_size; reverse_weight 0: its
transducer_attention_rescoring reverses the padded hypotheses with the lengths it has already incremented for <sos>,
unlike ASRModel.forward_attention_decoder), Transducer.transducer_attention_rescoring runs unmodified on a small object
that carries what it reads: `bs` pre-initialised (the shipped method asserts it before init_bs()) over the adapters of
gen_golden_rnnt_beam.py, the reference's predictor, joint and decoder modules, and `_ctc_prefix_beam_search` (which
the reference does not define) supplied from the reference's ctc_prefix_beam_search.  torchaudio is not installed:
torchaudio.functional.rnnt_loss is a stand-in that applies chunkformer_amd.transducer_rescore.td_score_host (f64) to
the log-softmax of the joint tensor the reference hands it -- so the reference pins the predictor / joint inputs, the
attention scores, the combination and the choice, not the loss recursion, which is pinned by enumeration in the
tests.  Nothing of the reference's text is copied.

Stored per case: the source case of rnnt_beam.npz, the mode, the weights, the n-best (tokens, search scores), the
restatement's (rescore_host, f64) td and attn per hypothesis, its totals, chosen index and margin (best minus second
total), and the reference's chosen index and score where it ran.

Conditions asserted here:
  - at least 100 cases;
  - where the reference ran, its score is within (T + U_max + 1) * 1e-5 * (transducer_weight + attn_weight) of the
    restatement's (the reference's joint and decoder are f32);
  - every case with margin >= 2 (T + U_max + 1) * 1e-5 * (transducer_weight + attn_weight) is an equality case -- the
    reference, where it ran, chose the restatement's index -- and these are at least 90% of all cases;
  - in at least a third of the equality cases the chosen index is not 0.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import gen_golden_rnnt_beam as GB  # noqa: E402  (the shim, the adapters, ref_modules)
import gen_golden_rescore as GR  # noqa: E402  (RefModel: the reference decoder under our weights)
from chunkformer.modules import search as ref_search  # noqa: E402
from chunkformer.transducer.search.prefix_beam_search import PrefixBeamSearch  # noqa: E402
from chunkformer.transducer.transducer import Transducer  # noqa: E402
from chunkformer.utils.common import log_add  # noqa: E402

import rnnt_beam_fixture as F  # noqa: E402
from chunkformer_amd import rescore as R  # noqa: E402
from chunkformer_amd import transducer_rescore as TR  # noqa: E402
from chunkformer_amd.search import DecodeResult  # noqa: E402

ref_search.PrefixScore.score = lambda self: log_add([self.s, self.ns])   # (gen_golden_beam.py's one deviation)

torch.set_num_threads(4)
OUT = os.path.join(HERE, "td_rescore.npz")
DEV = 1e-5
MAX_ROWS = 70
WEIGHTS = ((0.5, 0.5, 0.5), (0.3, 0.0, 0.7), (0.0, 0.5, 0.5), (1.0, 0.3, 0.3), (0.5, 0.0, 0.5))   # (ctc, attn, td)
DECODERS = (("uni", 0.0), ("bi", 0.0), ("bi", 0.3))   # (kind, reverse_weight)
DECODER_SEED = {"uni": 41, "bi": 42}


def aed_config(kind: str, vocab: int) -> R.AEDConfig:
    return R.AEDConfig(vocab=vocab, d_model=32, heads=2, ff=64, num_blocks=1, r_num_blocks=1 if kind == "bi" else 0,
                       bidirectional=kind == "bi")


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


class RefTransducer:
    """What Transducer.transducer_attention_rescoring reads of a Transducer."""
    ignore_id = -1
    reverse_weight = 0.0
    transducer_attention_rescoring = Transducer.transducer_attention_rescoring
    _cal_transducer_score = Transducer._cal_transducer_score
    _cal_attn_score = Transducer._cal_attn_score
    init_bs = Transducer.init_bs

    def __init__(self, cfg, pred, joint, dec: GR.RefModel, ctc_logp: torch.Tensor):
        self.blank, self.predictor, self.joint = cfg.blank, pred, joint
        self.decoder, self.sos, self.eos = dec.decoder, dec.sos, dec.eos
        self.ctc_logp = ctc_logp
        self.bs = PrefixBeamSearch(GB.EncoderStub(), GB.PredictorAdapter(pred), joint, GB.CtcStub(ctc_logp), cfg.blank)

    def _ctc_prefix_beam_search(self, speech, speech_lengths, beam_size, decoding_chunk_size=-1,
                                num_decoding_left_chunks=-1, simulate_streaming=False):
        r = ref_search.ctc_prefix_beam_search(self.ctc_logp[None], speech_lengths, beam_size, None, self.blank)[0]
        return list(zip(r.nbest, r.nbest_scores)), speech


def main():
    _, meta_src = F.archive()
    modules, decoders = {}, {}
    arrays, meta = {}, {"dev": DEV, "decoder_seed": DECODER_SEED, "cases": []}
    n_ref = 0
    for src, mc in enumerate(meta_src["cases"]):
        if not 1 <= mc["rows"] <= MAX_ROWS:
            continue
        i = len(meta["cases"])
        c = F.case(src)
        name, recipe, T, beam = mc["model"], mc["recipe"], mc["rows"], mc["beam"]
        cfg, sd = F.model(name, recipe)
        host = F.host_model(name, recipe)
        if (name, recipe) not in modules:
            modules[(name, recipe)] = GB.ref_modules(cfg, sd)
        pred, joint = modules[(name, recipe)]
        kind, rw = DECODERS[i % len(DECODERS)]
        cw, aw, tw = WEIGHTS[i % len(WEIGHTS)]
        if (kind, cfg.vocab) not in decoders:
            ac = aed_config(kind, cfg.vocab)
            dsd = R.synthetic_decoder_state_dict(ac, DECODER_SEED[kind])
            decoders[(kind, cfg.vocab)] = (ac, dsd, GR.RefModel(ac, dsd))
        ac, dsd, ref_dec = decoders[(kind, cfg.vocab)]
        mode = "transducer" if i % 2 == 0 else "ctc"
        if mode == "transducer":
            nbest, scores = c["tokens"], c["scores"]
        else:
            r = ref_search.ctc_prefix_beam_search(c["ctc"][None], torch.tensor([T]), beam, None, cfg.blank)[0]
            nbest, scores = [list(h) for h in r.nbest], [float(s) for s in r.nbest_scores]
        res = DecodeResult(list(nbest[0]), scores[0], nbest=[list(h) for h in nbest], nbest_scores=list(scores))
        got = TR.rescore_host(host, (ac, dsd), c["enc"], [0], [T], [res], cw, aw, tw, rw)[0]
        totals = got.nbest_scores
        srt = sorted(totals, reverse=True)
        margin = srt[0] - srt[1] if len(srt) > 1 else 1e30
        u_max = max(len(h) for h in nbest)
        bar = (T + u_max + 1) * DEV * (tw + aw)
        ref_index, ref_score = -1, 0.0
        if len(nbest) == beam and rw == 0.0:
            m = RefTransducer(cfg, pred, joint, ref_dec, c["ctc"])
            with torch.no_grad():
                hyp, sc = m.transducer_attention_rescoring(
                    c["enc"].unsqueeze(0), torch.tensor([T]), beam, reverse_weight=0.0, ctc_weight=cw, attn_weight=aw,
                    transducer_weight=tw, search_ctc_weight=mc["cw"], search_transducer_weight=mc["tw"],
                    beam_search_type=mode)
            ref_score = float(sc)
            ref_index = [list(h) for h in nbest].index([int(t) for t in hyp])
            assert abs(ref_score - (totals[ref_index])) <= bar, (src, mode, ref_score, totals[ref_index], bar)
            n_ref += 1
        equality = bool(margin >= 2 * bar)
        if equality and ref_index >= 0:
            assert ref_index == got.best_index, (src, mode, ref_index, got.best_index, margin)
        meta["cases"].append({"src": src, "model": name, "recipe": recipe, "rows": T, "beam": beam, "mode": mode,
                              "decoder": kind, "reverse_weight": rw, "ctc_weight": cw, "attn_weight": aw,
                              "transducer_weight": tw, "search_ctc_weight": mc["cw"],
                              "search_transducer_weight": mc["tw"], "equality": equality, "margin": float(min(margin, 1e30)),
                              "best_index": int(got.best_index), "score": float(got.score), "ref_index": ref_index,
                              "ref_score": ref_score})
        p = f"c{i:03d}/"
        arrays[p + "lens"] = np.array([len(h) for h in nbest], np.int32)
        arrays[p + "tokens"] = np.array([t for h in nbest for t in h], np.int16)
        arrays[p + "search"] = np.array(scores, np.float64)
        arrays[p + "td"] = np.array(got.td_scores, np.float64)
        arrays[p + "attn"] = np.array(got.decoder_scores, np.float64)
        arrays[p + "totals"] = np.array(totals, np.float64)
    cases = meta["cases"]
    eq = [c for c in cases if c["equality"]]
    moved = [c for c in eq if c["best_index"] != 0]
    print(len(cases), "cases,", n_ref, "reference runs,", len(eq), "equality,", len(moved), "choose another than 0")
    assert len(cases) >= 100
    assert len(eq) >= 0.9 * len(cases), (len(eq), len(cases))
    assert 3 * len(moved) >= len(eq), (len(moved), len(eq))
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
