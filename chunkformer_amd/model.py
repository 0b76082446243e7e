"""Host-side mirror of the reference `ChunkFormerModel` callers of the encoder hot path
(chunkformer/chunkformer_model.py), on top of `ChunkFormerEncoder` (libcfm.so):

  encode           chunkformer_model.py:256-274   padded batch -> (xs, xs_lens)
  endless_decode   chunkformer_model.py:321-459   segment loop with att/cnn caches carried
  batch_decode     chunkformer_model.py:462-552   duration-budget grouping -> masked batch -> CTC
  from_pretrained  chunkformer_model.py:107-200   LOCAL directory only (no hub access)

Audio (`_load_audio_and_extract_features`, 276-318): wherever the reference takes an
`audio_path`, this mirror takes a 16-bit PCM `.wav` path (decoded with the standard library,
features by the GPU Kaldi fbank of fbank.py with the reference's parameters, config
`fbank_conf` / `resample_conf`), or 80-dim fbank features directly -- a `[T, 80]` tensor, or a
path to a `.npy` (loaded with allow_pickle=False) / `.pt` (torch.load weights_only=True) file.

CTC post-processing (remove_duplicates_and_blank and get_output_with_timestamps' sentence
split, chunkformer/utils/model_utils.py:23-221) runs on the device (cfm_ctc_collapse); only
the id -> text mapping (class2str) and the hh:mm:ss:ms formatting stay on the host, so
`char_dict` models return strings like the reference.

Hybrid CTC / attention checkpoints (`decoder: transformer` / `bitransformer` with decoder.* tensors) also
decode with `decoding_method="attention_rescoring"` (asr_model.py:326-343): the prefix beam search's n-best
rescored by the attention decoder on the device (rescore.py, cfm_aed_score).

`model: transducer` checkpoints (config.yaml, init_model.py:118-135) decode with the RNN-T greedy
search on the device (transducer.py, cfm_rnnt_greedy) exactly where the reference calls
optimized_search / batch_greedy_search (chunkformer_model.py:439-448, 533-543); their per-frame
decisions [T, n_steps] go through get_output_with_timestamps' transducer branch (no collapse).
With `decoding_method="rnnt_beam_search"` they run the reference's transducer prefix beam search instead
(transducer_beam.py, cfm_rnnt_beam_search): frame-synchronous, shallow-fused with the CTC head's posterior
(`ctc_weight` 0.3, `transducer_weight` 0.7), with n-best and token frames.
`decoding_method="rnnt_beam_attn_rescoring"` / `"ctc_beam_td_attn_rescoring"` re-rank the n-best of that search / of
the CTC prefix beam search by the full-sum transducer score of every hypothesis and, when the checkpoint carries
decoder.* tensors, the attention decoder's score (transducer_rescore.py, cfm_rnnt_td_score + cfm_aed_score).
`model: classification` checkpoints (config.yaml `model_conf.tasks`, init_model.py:106-116, with an
optional label_mapping.json) run the reference's classification path on the device (classifier.py,
cfm_cls_classify): masked mean pool of the encoder output over time + one linear head per task,

  classify         classification_model.py:232-281   padded batch -> {task}_prediction / _probability
  classify_audio   chunkformer_model.py:555-640      one input -> {task: {label, label_id, prob}}
  batch_classify   (bin/classify.py's use case)      duration-budget grouping -> masked batch -> heads

They have no CTC head; the ASR decoding methods raise ValueError on them and classify* raises
ValueError on the other model types.
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from .config import EncoderConfig
from .encoder import ChunkFormerEncoder
from .streaming import EndlessGraphPipeline, EndlessGraphRunner, EndlessPipeline
from .classifier import ClassifierConfig, ClassifierHeads
from .rescore import AEDConfig, AttentionRescorer
from .transducer import RNNTConfig, RNNTGreedy

Features = Union[torch.Tensor, np.ndarray, str]


# ----------------------------------------------------------------------------- text helpers
def remove_duplicates_and_blank(hyp: Sequence[int], blank_id: int = 0) -> List[int]:
    """model_utils.py:23-32: collapse repeats, then drop blanks."""
    out: List[int] = []
    prev = None
    for t in hyp:
        t = int(t)
        if t != prev and t != blank_id:
            out.append(t)
        prev = t
    return out


def class2str(target: Sequence[int], char_dict: Dict[int, str]) -> str:
    """model_utils.py:135-139."""
    return "".join(char_dict[int(w)] for w in target).replace("▁", " ")


def get_output(hyps, char_dict: Dict[int, str]) -> List[str]:
    """model_utils.py:164-171 (asr_model branch)."""
    return [class2str(remove_duplicates_and_blank([int(t) for t in h]), char_dict).strip() for h in hyps]


def milliseconds_to_hhmmssms(ms: int) -> str:
    """model_utils.py:142-161."""
    h, rem = divmod(int(ms), 3600 * 1000)
    m, rem = divmod(rem, 60 * 1000)
    s, rem = divmod(rem, 1000)
    return f"{h:02}:{m:02}:{s:02}:{rem:03}"


def max_silence_frames(max_silence_duration: float) -> int:
    """model_utils.py:176: max_silence = max_silence_duration // 0.08 (80 ms frames); a negative
    value never closes a sentence, i.e. one segment per utterance."""
    ms = max_silence_duration // 0.08
    return int(ms) if ms >= 0 else 1 << 30


def format_segments(segs, char_dict: Dict[int, str]) -> List[dict]:
    """Device segments (tokens, start frame, end frame) -> the reference's items
    {"decode", "start", "end"} (model_utils.py:203-218: class2str(...).strip(), 80 ms frames)."""
    return [{"decode": class2str(toks, char_dict).strip(), "start": milliseconds_to_hhmmssms(st * 80),
             "end": milliseconds_to_hhmmssms(en * 80)} for toks, st, en in segs]


def transducer_segments(dense, max_silence: int):
    """get_output_with_timestamps (model_utils.py:174-221) for model_type "transducer": dense
    per-frame decisions [T, n_steps] (0 = blank; a frame is silent when all are blank, its tokens
    are the non-blank decisions in step order, no duplicate removal) -> [(tokens, start, end)] in
    80 ms frames.  Walks the non-blank frames only (a blank run closes the sentence when it
    reaches max_silence frames)."""
    d = np.asarray(dense)
    T = d.shape[0]
    nbf = np.nonzero((d != 0).any(1))[0].tolist()
    segs, toks, start, prev_end = [], [], -1, -1
    for i, t in enumerate(nbf):
        if start == -1:
            start = max(math.ceil((t + prev_end) / 2), t - 2) if prev_end != -1 else max(t - 2, 0)
        row = d[t]
        toks.extend(int(v) for v in row[row != 0])
        gap = (nbf[i + 1] if i + 1 < len(nbf) else T) - t - 1   # blank frames after t
        end = t if max_silence == 0 else (t + max_silence if 0 < max_silence <= gap else -1)
        if end != -1:
            segs.append((toks, start, end))
            prev_end, toks, start = end, [], -1
    if start != -1 and toks:
        segs.append((toks, start, T - 1))
    return segs


# ----------------------------------------------------------------------------- segment math
def endless_segments(xs_len: int, C: int, L: int, R: int, total_batch_duration: float, num_blocks: int,
                     kernel_size: int = 15, subsampling: int = 8):
    """The segment schedule of endless_decode (chunkformer_model.py:355-435) as plain
    integers: returns (truncated_context_size, [(start, stop, keep_trunc, last), ...]) where
    frames [start, stop) feed one forward_parallel_chunk call and `keep_trunc` says whether
    only the first `truncated_context_size` output frames are kept."""
    lorder = kernel_size // 2
    max_len = int(total_batch_duration // 0.01) // 2
    mult = max_len // C // subsampling
    trunc = C * mult
    if trunc <= 0:
        raise ValueError("total_batch_duration too small for one chunk")
    r = max(R, lorder)
    rel_right = (r + max(C, r) * (num_blocks - 1)) * subsampling
    step = trunc * subsampling
    segs = []
    for idx in range((xs_len + step - 1) // step if xs_len > 0 else 0):
        start = step * idx
        end = min(step * (idx + 1) + 7, xs_len)
        stop = min(end + rel_right, xs_len)
        last = step * idx + rel_right >= xs_len
        segs.append((start, stop, not last, last))
        if last:
            break
    return trunc, segs


def budget_groups(lens: Sequence[int], total_batch_duration: float) -> List[List[int]]:
    """batch_decode's grouping (chunkformer_model.py:481-529): utterances are appended
    until the frame budget int(tbd // 0.01) // 2 is used up (the utterance that crosses
    it is included), then the group is flushed; the tail is flushed at the end."""
    budget = int(total_batch_duration // 0.01) // 2
    groups, cur, left = [], [], budget
    for i, t in enumerate(lens):
        cur.append(i)
        left -= int(t)
        if left <= 0 or i == len(lens) - 1:
            groups.append(cur)
            cur, left = [], budget
    return groups


def _load_features(x: Features, featurize=None) -> torch.Tensor:
    if isinstance(x, str) and x.lower().endswith(".wav"):
        from .fbank import load_wav
        samples, sr = load_wav(x)
        return featurize(samples, sr)
    if isinstance(x, torch.Tensor):
        t = x
    elif isinstance(x, np.ndarray):
        t = torch.from_numpy(x)
    elif isinstance(x, str):
        if x.endswith(".npy"):
            t = torch.from_numpy(np.load(x, allow_pickle=False))
        elif x.endswith(".pt"):
            t = torch.load(x, map_location="cpu", weights_only=True)
        else:
            raise ValueError(f"{x}: only 16-bit PCM .wav audio is decoded here (no pydub/ffmpeg); or pass "
                             "80-dim fbank features ([T, 80] tensor, .npy or .pt)")
    else:
        raise TypeError(f"unsupported feature input {type(x)}")
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2:
        raise ValueError(f"features must be [T, F], got {tuple(t.shape)}")
    return t.float()


# ----------------------------------------------------------------------------- model
@dataclasses.dataclass(frozen=True)
class _Decoding:
    """A decoding_method other than the greedy default, resolved once per call."""
    method: str        # "ctc_prefix_beam_search", "attention_rescoring", "attention", "rnnt_beam_search",
                       # "rnnt_beam_attn_rescoring" or "ctc_beam_td_attn_rescoring"
    searcher: object   # the encoder (CTC prefix beam search), the AttentionDecoder, the RNNTBeamSearch or the
                       # TransducerRescorer
    lens: str          # the row lengths the search runs over: "ctc" (el_ctc) or "rnnt" (el_rnnt)
    timed: bool        # its hypotheses carry frame times (endless_decode's sentence split)


class ChunkFormerModel:
    """encoder + CTC head, RNN-T search or classification heads; the inference API of
    chunkformer_model.py on libcfm."""

    def __init__(self, cfg: EncoderConfig, state_dict: Dict[str, torch.Tensor], dtype: str = "bf16", device=None,
                 char_dict: Optional[Dict[int, str]] = None, fbank_conf: Optional[dict] = None,
                 resample_conf: Optional[dict] = None, model_type: str = "asr_model",
                 rnnt_config: Optional[RNNTConfig] = None, tasks: Optional[Dict[str, int]] = None,
                 classifier_config: Optional[ClassifierConfig] = None,
                 label_mapping: Optional[Dict[str, Dict[str, str]]] = None, aed_config: Optional[AEDConfig] = None,
                 aed_unsupported: Optional[str] = None):
        if model_type not in ("asr_model", "transducer", "classification"):
            raise AssertionError(f"model: {model_type} is not one of asr_model / transducer / classification")
        self.is_classification = model_type == "classification"
        if self.is_classification:
            if classifier_config is None:
                if not tasks:
                    raise ValueError("Classification model requires 'tasks' in model_conf")
                classifier_config = ClassifierConfig(tasks=dict(tasks), enc_dim=cfg.d_model)
            if cfg.vocab != 0:   # init_model.py:77: a classification model has no CTC head
                cfg = dataclasses.replace(cfg, vocab=0)
        self.config = cfg
        self.model_type = model_type
        self.encoder = ChunkFormerEncoder(cfg, state_dict, device=device, dtype=dtype)
        self.device = self.encoder.device
        self.rnnt = None
        if model_type == "transducer":
            rc = rnnt_config or RNNTConfig(vocab=cfg.vocab, enc_dim=cfg.d_model)
            self.rnnt = RNNTGreedy(rc, state_dict, self.device)
        self.classifier = None
        if self.is_classification:
            self.classifier = ClassifierHeads(classifier_config, state_dict, self.device)
        # the attention decoder of a hybrid CTC / attention checkpoint (decoding_method "attention_rescoring")
        self.rescorer = None
        if aed_config is not None and model_type in ("asr_model", "transducer"):
            self.rescorer = AttentionRescorer(aed_config, state_dict, self.device, dtype)
        # why a transducer checkpoint's decoder.* tensors gave no rescorer (raised when a rescoring mode asks for it)
        self._aed_unsupported = aed_unsupported
        self._dtype = dtype
        self._td_rescorer = None         # the transducer rescoring modes: built on first use over self.rnnt's handle
        self._attention_decoder = None   # decoding_method "attention": built on first use over the rescorer's handle
        self._rnnt_beam = None           # decoding_method "rnnt_beam_search": built on first use over self.rnnt's handle
        self.label_mapping = label_mapping
        self.char_dict = char_dict
        self.fbank_conf = dict(fbank_conf or {})
        self.resample_conf = dict(resample_conf or {})
        self._fbank = None
        self._endless_runners: Dict[tuple, EndlessGraphRunner] = {}
        # endless_decode: truncated segments compute only the rows their kept rows depend on (native
        # "trim_right"; the kept rows, ids and caches are unchanged -- test_endless_trim_equals_full)
        self.endless_trim = True
        # endless_decode's graph pipeline: a segment's first front-end windows (the previous segment's last
        # complete ones, the same frames) are carried over instead of recomputed (streaming.py; exact)
        self.endless_fe_reuse = True

    def extract_features(self, samples, sample_rate: Optional[int] = None) -> torch.Tensor:
        """_load_audio_and_extract_features (chunkformer_model.py:276-318) after decoding:
        kaldi.fbank with the config's num_mel_bins / frame_length / frame_shift, dither 0,
        energy_floor 0, at resample_conf.resample_rate (16 kHz), on int16-scale samples; on the GPU."""
        rate = int(self.resample_conf.get("resample_rate", 16000))
        if sample_rate is not None and int(sample_rate) != rate:
            raise ValueError(f"audio at {sample_rate} Hz: resampling is not part of this build, expected {rate} Hz")
        if self._fbank is None:
            from .fbank import KaldiFbank
            self._fbank = KaldiFbank(self.device, num_mel_bins=int(self.fbank_conf.get("num_mel_bins", 80)),
                                     frame_length=float(self.fbank_conf.get("frame_length", 25)),
                                     frame_shift=float(self.fbank_conf.get("frame_shift", 10)), dither=0.0,
                                     energy_floor=0.0, sample_frequency=float(rate))
        return self._fbank(torch.as_tensor(samples, dtype=torch.float32))

    # ---------------------------------------------------------------- loading
    @classmethod
    def from_pretrained(cls, path: str, dtype: str = "bf16", device=None) -> "ChunkFormerModel":
        """Local checkpoint directory in the reference layout (chunkformer_model.py:107-200):

        * config.yaml (yaml.safe_load): encoder_conf, input_dim, output_dim, cmvn / cmvn_conf;
        * global_cmvn: JSON {mean_stat, var_stat, frame_num} or kaldi text stats
          (cmvn_conf.is_json_cmvn, utils/cmvn.py:23-98), used when config `cmvn: global_cmvn`
          (init_model.py:63-69);
        * pytorch_model.{bin,pt,ckpt} (torch.load weights_only=True: plain tensors only), loaded
          like load_checkpoint(strict=False) (checkpoint.py:26-41): keys present in the
          checkpoint win, so its `encoder.global_cmvn.{mean,istd}` buffers override the stats file
          exactly as load_state_dict does in the reference; model.safetensors is also accepted;
        * vocab.txt ("token id" per line, file_utils.py:62-69) -> char_dict for text output;
        * `model: classification`: the heads come from model_conf.tasks (in their order), and
          label_mapping.json ({task: {"id": label}}, chunkformer_model.py:200-205), when present,
          names the predicted ids in classify_audio / batch_classify.
        There is no hub access: `path` must be a local directory."""
        import yaml
        if not os.path.isdir(path):
            raise FileNotFoundError(f"{path}: only local checkpoint directories are supported (no hub access)")
        cfg_path = os.path.join(path, "config.yaml")
        if not os.path.exists(cfg_path):
            raise ValueError(f"No config found in {path}")
        with open(cfg_path) as f:
            conf = yaml.safe_load(f)
        st = os.path.join(path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd: Dict[str, torch.Tensor] = dict(load_file(st))
        else:
            cands = ["pytorch_model.bin", "pytorch_model.pt", "pytorch_model.ckpt"]
            for nm in cands:
                p = os.path.join(path, nm)
                if os.path.exists(p):
                    sd = torch.load(p, map_location="cpu", weights_only=True)
                    break
            else:
                raise ValueError(f"No checkpoint found in {path}. Expected one of: {cands}")
        # chunkformer_model.py:153-160, 91-100: GlobalCMVN exists exactly when the directory holds a
        # global_cmvn file (whatever config.yaml's `cmvn` key says), JSON unless the config's top-level
        # is_json_cmvn is false
        cmvn_path = os.path.join(path, "global_cmvn")
        has_cmvn = os.path.exists(cmvn_path)
        if has_cmvn:
            is_json = bool(conf.get("is_json_cmvn", True))
            mean, istd = load_json_cmvn(cmvn_path) if is_json else load_kaldi_cmvn(cmvn_path)
            sd.setdefault("encoder.global_cmvn.mean", torch.tensor(mean, dtype=torch.float64).float())
            sd.setdefault("encoder.global_cmvn.istd", torch.tensor(istd, dtype=torch.float64).float())
        else:   # no GlobalCMVN module: checkpoint buffers would be unexpected keys (ignored)
            sd.pop("encoder.global_cmvn.mean", None)
            sd.pop("encoder.global_cmvn.istd", None)
        model_type = conf.get("model", "asr_model")   # ChunkFormerConfig default (chunkformer_model.py:47-48)
        vocab = int(conf.get("output_dim", sd["ctc.ctc_lo.weight"].shape[0] if "ctc.ctc_lo.weight" in sd else 0))
        if model_type == "classification":
            vocab = 0   # init_model.py:77
        cfg = EncoderConfig.from_encoder_conf(conf.get("encoder_conf", {}), input_dim=int(conf.get("input_dim", 80)),
                                              output_dim=vocab, cmvn=has_cmvn)
        rnnt_cfg = RNNTConfig.from_conf(conf, vocab, cfg.d_model) if model_type == "transducer" else None
        cls_cfg = ClassifierConfig.from_conf(conf, cfg.d_model) if model_type == "classification" else None
        # init_model.py:81-98: an asr_model checkpoint with decoder.* tensors carries the attention decoder that
        # attention_rescoring runs; unsupported decoder settings raise AssertionError here
        aed_cfg = None
        if (model_type == "asr_model" and any(k.startswith("decoder.") for k in sd)
                and conf.get("decoder", "transformer") in ("transformer", "bitransformer")):
            aed_cfg = AEDConfig.from_conf(conf, vocab, cfg.d_model)
        # init_model.py:118-135 passes the decoder into the Transducer too (its attention rescoring modes); a decoder
        # those modes cannot run must not keep the checkpoint from loading: the reason is kept for them
        aed_reason = None
        if model_type == "transducer":
            aed_cfg, aed_reason = transducer_decoder_config(conf, sd, vocab, cfg.d_model)
        label_mapping = None
        lp = os.path.join(path, "label_mapping.json")
        if os.path.exists(lp):
            with open(lp) as f:
                label_mapping = json.load(f)
        char_dict = None
        vp = os.path.join(path, "vocab.txt")
        if os.path.exists(vp):
            char_dict = {}
            with open(vp, encoding="utf8") as f:
                for line in f:
                    arr = line.strip().split()
                    if len(arr) != 2:
                        raise AssertionError(f"bad vocab line {line!r}")
                    char_dict[int(arr[1])] = arr[0]
        return cls(cfg, sd, dtype=dtype, device=device, char_dict=char_dict, fbank_conf=conf.get("fbank_conf"),
                   resample_conf=conf.get("resample_conf"), model_type=model_type, rnnt_config=rnnt_cfg,
                   classifier_config=cls_cfg, label_mapping=label_mapping, aed_config=aed_cfg,
                   aed_unsupported=aed_reason)

    def get_tasks(self) -> Optional[Dict[str, int]]:
        """chunkformer_model.py:250-254: {task: classes} of a classification model, else None."""
        return dict(self.classifier.cfg.tasks) if self.is_classification else None

    def get_classification_heads(self) -> Optional[ClassifierHeads]:
        """chunkformer_model.py:244-248: the heads of a classification model, else None."""
        return self.classifier if self.is_classification else None

    def _require_classification(self) -> None:
        if not self.is_classification:   # chunkformer_model.py:595-598
            raise ValueError("This model is not a classification model. Use ASR decoding methods instead.")

    def _require_asr(self, what: str) -> None:
        if self.is_classification:
            raise ValueError(f"This model is a classification model: {what} needs an asr_model or transducer "
                             "checkpoint. Use classify / classify_audio / batch_classify instead.")

    def _attention_search(self):
        """The AttentionDecoder of decoding_method "attention" (attention_decode.py), over the rescorer's handle: the
        decoder weights are on the device once.  ValueError for a transducer model or a checkpoint without decoder."""
        if self.model_type == "transducer":
            raise ValueError("This model is a transducer model: attention needs an asr_model checkpoint with an "
                             "attention decoder. Its decoding is the RNN-T greedy search.")
        if getattr(self, "rescorer", None) is None:
            raise ValueError("This model has no attention decoder (the checkpoint holds no decoder.* tensors): "
                             "attention needs a hybrid CTC / attention checkpoint. Use ctc_prefix_beam_search or "
                             "ctc_greedy_search.")
        if getattr(self, "_attention_decoder", None) is None:
            from .attention_decode import AttentionDecoder
            self._attention_decoder = AttentionDecoder(self.rescorer)
        return self._attention_decoder

    def _rnnt_beam_search(self):
        """The RNNTBeamSearch of decoding_method "rnnt_beam_search" (transducer_beam.py), over the greedy search's
        handle.  ValueError for a model that is not a transducer."""
        if self.model_type != "transducer" or getattr(self, "rnnt", None) is None:
            raise ValueError(f"This model is a {self.model_type} model: rnnt_beam_search needs a transducer checkpoint "
                             "(model: transducer).")
        if getattr(self, "_rnnt_beam", None) is None:
            from .transducer_beam import RNNTBeamSearch
            self._rnnt_beam = RNNTBeamSearch(self.rnnt)
        return self._rnnt_beam

    def _transducer_rescoring(self, decoding_method: str):
        """The TransducerRescorer of the modes "rnnt_beam_attn_rescoring" / "ctc_beam_td_attn_rescoring"
        (transducer_rescore.py), over the greedy search's handle and the attention rescorer's, if the checkpoint has
        one.  ValueError naming the mode for a model that is not a transducer."""
        if self.model_type != "transducer" or getattr(self, "rnnt", None) is None:
            raise ValueError(f"This model is a {self.model_type} model: {decoding_method} needs a transducer checkpoint "
                             "(model: transducer).")
        if getattr(self, "_td_rescorer", None) is None:
            from .transducer_rescore import TransducerRescorer
            self._td_rescorer = TransducerRescorer(self.rnnt, getattr(self, "rescorer", None),
                                                   getattr(self, "_dtype", "fp32"))
        return self._td_rescorer

    def _beam_method(self, decoding_method: str) -> bool:
        """True for "ctc_prefix_beam_search" and "attention_rescoring" (CTC checkpoints only; the latter needs the
        checkpoint's attention decoder), False for the greedy default."""
        if decoding_method == "ctc_greedy_search":
            return False
        if decoding_method not in ("ctc_prefix_beam_search", "attention_rescoring"):
            raise ValueError(f"unknown decoding_method {decoding_method!r}: ctc_greedy_search, "
                             "ctc_prefix_beam_search or attention_rescoring")
        if self.model_type == "transducer":
            raise ValueError(f"This model is a transducer model: {decoding_method} needs an asr_model "
                             "checkpoint. Its decoding is the RNN-T greedy search.")
        if decoding_method == "attention_rescoring" and getattr(self, "rescorer", None) is None:
            raise ValueError("This model has no attention decoder (the checkpoint holds no decoder.* tensors): "
                             "attention_rescoring needs a hybrid CTC / attention checkpoint. Use "
                             "ctc_prefix_beam_search or ctc_greedy_search.")
        return True

    def _resolve_decoding(self, decoding_method: str) -> Optional[_Decoding]:
        """The search of `decoding_method`, None for the greedy default; ValueError for an unknown method or one this
        checkpoint cannot run."""
        if decoding_method == "attention":
            return _Decoding("attention", self._attention_search(), "ctc", timed=False)
        if decoding_method == "rnnt_beam_search":
            return _Decoding("rnnt_beam_search", self._rnnt_beam_search(), "rnnt", timed=True)
        if decoding_method == "rnnt_beam_attn_rescoring":
            return _Decoding(decoding_method, self._transducer_rescoring(decoding_method), "rnnt", timed=True)
        if decoding_method == "ctc_beam_td_attn_rescoring":
            return _Decoding(decoding_method, self._transducer_rescoring(decoding_method), "ctc", timed=True)
        if not self._beam_method(decoding_method):
            return None
        return _Decoding(decoding_method, self.encoder, "ctc", timed=True)

    def _search_rows(self, mode: _Decoding, rows: torch.Tensor, starts, lens, beam_size: int = 10, context_graph=None,
                     return_nbest: bool = False, transducer_weight: Optional[float] = None,
                     ctc_weight: Optional[float] = None, reverse_weight: Optional[float] = None,
                     length_penalty: float = 0.0, max_len: Optional[int] = None, attn_weight: Optional[float] = None,
                     search_ctc_weight: Optional[float] = None, search_transducer_weight: Optional[float] = None):
        """The search `mode` over packed encoder rows, utterance b = rows [starts[b], + lens[b]): one DecodeResult
        per utterance.  The options are those of endless_decode / batch_decode."""
        if mode.method in ("rnnt_beam_attn_rescoring", "ctc_beam_td_attn_rescoring"):
            rescorer = mode.searcher
            aw = (0.5 if rescorer.rescorer is not None else 0.0) if attn_weight is None else float(attn_weight)
            if aw > 0 and rescorer.rescorer is None:
                why = getattr(self, "_aed_unsupported", None)
                raise ValueError(f"{mode.method} with attn_weight > 0 needs an attention decoder: "
                                 + (f"this checkpoint's decoder is not supported ({why})." if why else
                                    "the checkpoint holds no decoder.* tensors.") + " Pass attn_weight=0.")
            if mode.method == "rnnt_beam_attn_rescoring":
                scw = 0.3 if search_ctc_weight is None else float(search_ctc_weight)
                stw = 0.7 if search_transducer_weight is None else float(search_transducer_weight)
                logp = None
                if scw > 0:
                    logp, _ = self.encoder.ctc_log_softmax(rows, want_logp=True, want_ids=False)
                results = self._rnnt_beam_search().search_packed(rows, logp, starts, lens, beam_size, scw, stw)
            else:
                results = self.encoder.ctc_prefix_beam_search(rows, starts, lens, beam_size, context_graph)
            return rescorer.rescore(results, rows, starts, lens, 0.5 if ctc_weight is None else float(ctc_weight), aw,
                                    0.5 if transducer_weight is None else float(transducer_weight), reverse_weight,
                                    return_nbest)
        if mode.method == "attention":
            return mode.searcher.search(rows, starts, lens, beam_size, length_penalty, max_len)
        if mode.method == "rnnt_beam_search":
            # one CTC log-softmax call (none at ctc_weight 0) and one search call
            cw = 0.3 if ctc_weight is None else float(ctc_weight)
            tw = 0.7 if transducer_weight is None else float(transducer_weight)
            logp = None
            if cw > 0:
                logp, _ = self.encoder.ctc_log_softmax(rows, want_logp=True, want_ids=False)
            return mode.searcher.search_packed(rows, logp, starts, lens, beam_size, cw, tw)
        results = mode.searcher.ctc_prefix_beam_search(rows, starts, lens, beam_size, context_graph)
        if mode.method == "attention_rescoring":
            results = self.rescorer.rescore(results, rows, starts, lens, ctc_weight, reverse_weight, return_nbest)
        return results

    def _render(self, result, return_nbest: bool):
        """What a search's DecodeResult comes back as: itself without a char_dict, the n-best texts with
        `return_nbest`, else the text of the best hypothesis."""
        if self.char_dict is None:
            return result
        if return_nbest:
            return [class2str(h, self.char_dict).strip() for h in result.nbest]
        return class2str(result.tokens, self.char_dict).strip()

    def _render_segments(self, result, T: int, max_silence_duration: float, return_timestamps: bool):
        """endless_decode's sentence split of a hypothesis with frame times: the reference's split over a dense
        [T, 1] array with the tokens at their `times` frames (at most one token per frame, no duplicate removal: "a a"
        stays two tokens); the sentences joined into one string without `return_timestamps`."""
        dense = np.zeros((T, 1), dtype=np.int64)
        dense[np.asarray(result.times, dtype=np.int64), 0] = np.asarray(result.tokens, dtype=np.int64)
        res = format_segments(transducer_segments(dense, max_silence_frames(max_silence_duration)), self.char_dict)
        if not return_timestamps:
            res = " ".join(item["decode"] for item in res).strip()
        return res

    # ---------------------------------------------------------------- API
    def encode(self, xs: torch.Tensor, xs_lens: torch.Tensor, chunk_size: Optional[int] = None,
               left_context_size: Optional[int] = None, right_context_size: Optional[int] = None, **kwargs):
        """chunkformer_model.py:256-274."""
        out, masks = self.encoder.forward_encoder(xs, xs_lens, chunk_size or 0, left_context_size or 0,
                                                  right_context_size or 0)
        return out, masks.squeeze(1).sum(-1)

    @torch.no_grad()
    def endless_decode(self, audio_path: Features, chunk_size: Optional[int] = 64,
                       left_context_size: Optional[int] = 128, right_context_size: Optional[int] = 128,
                       total_batch_duration: int = 1800, return_timestamps: bool = True,
                       max_silence_duration: float = 0.5, return_encoder_out: bool = False,
                       cuda_graph: bool = True, pipeline: Optional[bool] = None,
                       pipeline_depth: Optional[int] = None, decoding_method: str = "ctc_greedy_search",
                       beam_size: int = 10, context_graph=None, return_nbest: bool = False,
                       attn_weight: Optional[float] = None, search_ctc_weight: Optional[float] = None,
                       search_transducer_weight: Optional[float] = None,
                       transducer_weight: Optional[float] = None, ctc_weight: Optional[float] = None,
                       reverse_weight: Optional[float] = None,
                       length_penalty: float = 0.0, max_len: Optional[int] = None):
        """chunkformer_model.py:321-459.  Segments of `total_batch_duration` seconds (halved,
        like the reference) go through forward_parallel_chunk with the attention/conv caches
        and `offset` carried; the CTC argmax runs per segment on the kept rows (row-wise, so
        identical to the reference's argmax over the concatenation).
        Returns text (with char_dict) or ids [1, T', 1] like the reference; with
        `return_encoder_out` also the concatenated encoder output [1, T', d] (fp32).
        `pipeline` (default: on from 3 segments up): `pipeline_depth` (default 4 with graphs, 3 eager:
        the measured best of each at tbd 1800) segments in flight on as many
        streams, segment k + 1's layer l waiting only for segment k's layer l; with `cuda_graph` all
        segments (up to 128 per graph) replay one captured HIP graph of that whole multi-stream pipeline
        (EndlessGraphPipeline), without it every call is launched eagerly (EndlessPipeline).  pipeline=False: one segment at a time, the full-size
        middle segments replaying one captured graph (EndlessGraphRunner) when `cuda_graph`.  Every
        mode gives the same result as the eager loop (same kernels, same plans); see streaming.py.
        decoding_method "ctc_prefix_beam_search": the runner returns the encoder rows, and the top-k and
        beam kernels run over their concatenation as one utterance (`beam_size`, `context_graph`); the
        sentence split then places the best hypothesis' tokens at their `times` frames.
        `return_nbest`: the n-best texts (or the DecodeResult without a char_dict).
        decoding_method "attention_rescoring": that n-best rescored by the attention decoder over the same
        concatenated rows (rescore.py; `ctc_weight` / `reverse_weight` default to the checkpoint's model_conf);
        with `return_nbest` the n-best comes back re-ranked by the rescored totals.
        decoding_method "attention": the attention decoder's own beam search (attention_decode.py; `beam_size`,
        `length_penalty`, `max_len`) over the concatenated rows as one utterance; more than 5,000 rows need
        `max_len`.  The hypothesis carries no frame times: the text comes back as one string (the DecodeResult
        without a char_dict; `return_nbest`: the N final hypotheses in final-score order).
        decoding_method "rnnt_beam_search" (transducer checkpoints): the transducer prefix beam search
        (transducer_beam.py; `beam_size` 1 .. 16, `ctc_weight` default 0.3, `transducer_weight` default 0.7) over the
        concatenated rows as one utterance; the sentence split places the best hypothesis' tokens at the frames
        that appended them, `return_nbest` gives the final beam.
        decoding_method "rnnt_beam_attn_rescoring" / "ctc_beam_td_attn_rescoring": as in batch_decode, over the
        concatenated rows as one utterance; `attn_weight`, `search_ctc_weight` and `search_transducer_weight` must be
        passed by keyword (see batch_decode)."""
        self._require_asr("endless_decode")
        mode = self._resolve_decoding(decoding_method)
        opts = dict(beam_size=beam_size, context_graph=context_graph, return_nbest=return_nbest,
                    transducer_weight=transducer_weight, ctc_weight=ctc_weight, reverse_weight=reverse_weight,
                    length_penalty=length_penalty, max_len=max_len, attn_weight=attn_weight,
                    search_ctc_weight=search_ctc_weight, search_transducer_weight=search_transducer_weight)
        C = chunk_size if chunk_size is not None else 64
        L = left_context_size if left_context_size is not None else 128
        R = right_context_size if right_context_size is not None else 128
        cfg, enc, dev = self.config, self.encoder, self.device
        xs = _load_features(audio_path, self.extract_features)
        trunc, segs = endless_segments(xs.shape[0], C, L, R, total_batch_duration, cfg.num_blocks, cfg.kernel_size)
        xs_dev = xs.to(dev, torch.float32)
        ids, outs = [], []
        seg_len = max(stop - start for start, stop, _, _ in segs) if segs else 0
        transducer = self.model_type == "transducer"
        want_eo = bool(return_encoder_out) or transducer or mode is not None   # the searches consume the encoder rows
        if pipeline is None:
            pipeline = len(segs) >= 3
        if pipeline_depth is None:
            pipeline_depth = 4 if cuda_graph else 3
        trim = bool(self.endless_trim)
        fe_reuse = bool(self.endless_fe_reuse)
        key = (C, L, R, trunc, seg_len, want_eo, bool(cuda_graph), bool(pipeline), int(pipeline_depth), trim, fe_reuse)
        runner = self._endless_runners.get(key)
        if runner is None:   # graphs are captured once per segment geometry and reused across calls
            for old in self._endless_runners.values():   # the replaced runner's graphs are destroyed
                old.close()
            self._endless_runners = {}
            if pipeline:
                runner = (EndlessGraphPipeline(enc, C, L, R, trunc, seg_len, want_eo, pipeline_depth, trim=trim,
                                               fe_reuse=fe_reuse)
                          if cuda_graph else EndlessPipeline(enc, C, L, R, trunc, want_eo, pipeline_depth, trim=trim))
            else:
                runner = EndlessGraphRunner(enc, C, L, R, trunc, seg_len, want_eo, use_graph=cuda_graph, trim=trim)
            self._endless_runners = {key: runner}
        if pipeline:
            tids, teos, cur = runner.run(xs_dev, segs)
            ids = [t for t in tids if t is not None]
            outs = [e for e in teos if e is not None]
            self.last_endless_caches = (runner.att[cur], runner.cnn[cur])
        else:
            runner.reset()
            offset = 0
            try:
                for start, stop, keep_trunc, _ in segs:
                    # forward_parallel_chunk with att/cnn caches carried; offset += len, then -= dropped rows
                    tok, eo, kept = runner.step(xs_dev[start:stop], offset, keep_trunc)
                    offset += kept
                    if tok is not None:
                        ids.append(tok)
                    if eo is not None:
                        outs.append(eo)
            finally:
                enc._set_trim(False)
            # the caches carried out of the last segment (r_att_cache / r_cnn_cache of its
            # forward_parallel_chunk call, chunkformer_model.py:407-417)
            self.last_endless_caches = (runner.att[runner.cur], runner.cnn[runner.cur])
        if mode is not None:
            # the concatenated rows as one utterance
            enc_all = torch.cat(outs) if outs else torch.zeros(0, cfg.d_model, device=dev)
            T = enc_all.shape[0]
            best = self._search_rows(mode, enc_all, [0], [T], **opts)[0]
            if self.char_dict is None or return_nbest or not mode.timed:
                res = self._render(best, return_nbest)
            else:
                res = self._render_segments(best, T, max_silence_duration, return_timestamps)
            if return_encoder_out:
                return res, enc_all.unsqueeze(0)
            return res
        if transducer:
            # optimized_search over the concatenated encoder output (chunkformer_model.py:439-448):
            # decisions [1, T, n_steps], text by get_output_with_timestamps' transducer branch
            enc_all = torch.cat(outs) if outs else torch.zeros(0, cfg.d_model, device=dev)
            T = enc_all.shape[0]
            dense = self.rnnt.greedy_packed(enc_all, [0], [T])
            tokens = dense.long().reshape(1, T, -1)
            if self.char_dict is not None:
                segs_t = transducer_segments(dense.cpu().numpy(), max_silence_frames(max_silence_duration))
                res = format_segments(segs_t, self.char_dict)
                if not return_timestamps:
                    res = " ".join(item["decode"] for item in res).strip()
            else:
                res = tokens
            if return_encoder_out:
                return res, enc_all.unsqueeze(0)
            return res
        tokens = torch.cat(ids).long().reshape(1, -1, 1) if ids else None
        if self.char_dict is not None and tokens is not None:
            # get_output_with_timestamps (model_utils.py:174-221) on the device: sentence split at
            # max_silence blank frames, de-duplicated tokens per sentence
            segs = enc.ctc_collapse(tokens, [0], [tokens.shape[1]],
                                    max_silence=max_silence_frames(max_silence_duration))[0]
            res = format_segments(segs, self.char_dict)
            if not return_timestamps:
                res = " ".join(item["decode"] for item in res).strip()
        else:
            res = tokens
        if return_encoder_out:
            return res, torch.cat(outs).unsqueeze(0)
        return res

    @torch.no_grad()
    def batch_decode(self, audio_paths: List[Features], chunk_size: Optional[int] = 64,
                     left_context_size: Optional[int] = 128, right_context_size: Optional[int] = 128,
                     total_batch_duration: int = 1800, decoding_method: str = "ctc_greedy_search",
                     beam_size: int = 10, context_graph=None, return_nbest: bool = False,
                     attn_weight: Optional[float] = None, search_ctc_weight: Optional[float] = None,
                     search_transducer_weight: Optional[float] = None,
                     transducer_weight: Optional[float] = None, ctc_weight: Optional[float] = None,
                     reverse_weight: Optional[float] = None,
                     length_penalty: float = 0.0, max_len: Optional[int] = None):
        """chunkformer_model.py:462-552 (asr_model branch): budget grouping, one masked-batch
        encoder call per group, CTC argmax, per-utterance split to its subsampled length.
        decoding_method "ctc_prefix_beam_search": one top-k and one beam-search call per masked batch over
        the same per-utterance row ranges (`beam_size`, `context_graph`: search.ContextGraph); text of the
        best hypothesis (`return_nbest`: of every hypothesis), or DecodeResults without a char_dict.
        decoding_method "attention_rescoring" (asr_model.py:326-343): the same top-k and beam search, then one
        attention decoder call per masked batch over the packed encoder rows it already holds, scoring every
        hypothesis of every utterance (rescore.py); `ctc_weight` / `reverse_weight` default to the checkpoint's
        model_conf; with `return_nbest` the n-best comes back re-ranked by the rescored totals.
        decoding_method "attention" (asr_model.py's `attention` mode): the attention decoder's own beam search
        (attention_decode.py), one device search per masked batch over the same packed rows, every utterance
        stopping at its own row count (or `max_len`); `beam_size` (1 .. 16), `length_penalty`.
        decoding_method "rnnt_beam_search" (transducer checkpoints): per masked batch one CTC log-softmax call
        (none at `ctc_weight` 0) and one transducer prefix beam search over the packed rows (transducer_beam.py;
        `ctc_weight` default 0.3, `transducer_weight` default 0.7, `return_nbest` as for the CTC beam search).
        decoding_method "rnnt_beam_attn_rescoring" (transducer checkpoints; transducer.py:257-391): the n-best of that
        transducer beam search (`search_ctc_weight` default 0.3, `search_transducer_weight` default 0.7) re-ranked by
        total = attn * `attn_weight` + search score * `ctc_weight` + td * `transducer_weight`, td the full-sum
        transducer log-likelihood of the hypothesis (transducer_rescore.py, one device call per masked batch) and attn
        the attention decoder's score (`reverse_weight` as in attention_rescoring).  `ctc_weight`, `transducer_weight`
        and `attn_weight` default to 0.5 each, `attn_weight` to 0 when the checkpoint has no decoder: this project's
        defaults -- the reference's CLI defaults are all 0, which always returns hypothesis 0.  `attn_weight` > 0
        without a decoder is a ValueError.  With `return_nbest` the n-best comes back re-ranked by the totals.
        decoding_method "ctc_beam_td_attn_rescoring": the same rescoring of the CTC prefix beam search's n-best
        (`context_graph` honoured; the search score is the CTC prefix score).
        `attn_weight`, `search_ctc_weight` and `search_transducer_weight` must be passed by keyword: they stand before
        `transducer_weight` in the signature (its tail is kept as earlier callers know it), so positional arguments
        past `return_nbest` are not a supported way to call this method."""
        self._require_asr("batch_decode")
        mode = self._resolve_decoding(decoding_method)
        opts = dict(beam_size=beam_size, context_graph=context_graph, return_nbest=return_nbest,
                    transducer_weight=transducer_weight, ctc_weight=ctc_weight, reverse_weight=reverse_weight,
                    length_penalty=length_penalty, max_len=max_len, attn_weight=attn_weight,
                    search_ctc_weight=search_ctc_weight, search_transducer_weight=search_transducer_weight)
        C = chunk_size if chunk_size is not None else 64
        L = left_context_size if left_context_size is not None else 128
        R = right_context_size if right_context_size is not None else 128
        feats = [_load_features(a, self.extract_features) for a in audio_paths]
        decodes = []
        for grp in budget_groups([f.shape[0] for f in feats], total_batch_duration):
            xs = [feats[i] for i in grp]
            lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int)
            offset = torch.zeros(len(xs), dtype=torch.int)
            eo, el, n_chunks, _, _, _ = self.encoder.forward_parallel_chunk(xs, lens, C, L, R, offset=offset)
            # per-utterance rows as the reference slices them: hyp.flatten()[:x_len] (Python slice: an
            # utterance under 7 frames has calc_length -1 and keeps all but the last row of its padded
            # chunk) and, for the transducer, frames t < encoder_out_lens (none at <= 0)
            el_ctc = [len(range(int(nc) * C)[: int(n)]) for nc, n in zip(n_chunks, el.tolist())]
            el_rnnt = [max(0, int(n)) for n in el.tolist()]
            if mode is not None:
                starts = (np.cumsum([0] + list(n_chunks[:-1])) * C).tolist()
                results = self._search_rows(mode, eo.reshape(-1, eo.shape[-1]), starts,
                                            el_rnnt if mode.lens == "rnnt" else el_ctc, **opts)
                decodes.extend(self._render(r, return_nbest) for r in results)
                continue
            if self.model_type == "transducer":
                # batch_greedy_search over each utterance's rows (chunkformer_model.py:533-543): the
                # packed rows go straight in (no pad_sequence), one workgroup per utterance
                starts = (np.cumsum([0] + list(n_chunks[:-1])) * C).tolist()
                dense = self.rnnt.greedy_packed(eo.reshape(-1, eo.shape[-1]), starts, el_rnnt).cpu()
                hyps = [dense[s0: s0 + n].reshape(-1) for s0, n in zip(starts, el_rnnt)]
                hyps = [h[h != self.rnnt.cfg.blank].tolist() for h in hyps]
                if self.char_dict is not None:
                    decodes.extend(class2str(h, self.char_dict).strip() for h in hyps)
                else:
                    decodes.extend(hyps)
                continue
            _, hyp = self.encoder.ctc_log_softmax(eo, want_logp=False)   # fused argmax head
            if self.char_dict is not None:
                # remove_duplicates_and_blank on the device, per utterance rows [64 * chunk0, +len)
                starts = np.cumsum([0] + list(n_chunks[:-1])) * C
                toks = self.encoder.ctc_collapse(hyp, starts.tolist(), el_ctc)
                decodes.extend(class2str(t, self.char_dict).strip() for t, _ in toks)
            else:
                decodes.extend(h.flatten()[:n].long() for h, n in zip(hyp.split(n_chunks, dim=0), el_ctc))
        return decodes

    # ---------------------------------------------------------------- forced alignment
    def _require_ctc_align(self, what: str) -> None:
        self._require_asr(what)
        if self.model_type == "transducer":
            raise ValueError(f"This model is a transducer model: {what} needs an asr_model checkpoint "
                             "(CTC forced alignment runs on the CTC head's log-probs).")

    @torch.no_grad()
    def batch_align(self, audio_paths: List[Features], targets, chunk_size: Optional[int] = 64,
                    left_context_size: Optional[int] = 128, right_context_size: Optional[int] = 128,
                    total_batch_duration: int = 1800, max_workspace_bytes: Optional[int] = None):
        """CTC forced alignment of many inputs (the reference: bin/alignment.py, one utterance at a time
        through torchaudio on the CPU): batch_decode's budget groups and per-utterance row ranges, one
        masked-batch encoder call, one ctc_log_softmax call and one align call per group.  `targets`:
        one token-id list per input.  Returns one align.AlignResult per input, in input order (frames,
        spans, token_times(), words(char_dict)); ValueError names the inputs that cannot be aligned, after
        the others have been computed.  `max_workspace_bytes` bounds the trellis."""
        self._require_ctc_align("batch_align")
        if len(targets) != len(audio_paths):
            raise ValueError("batch_align needs one target per input")
        C = chunk_size if chunk_size is not None else 64
        L = left_context_size if left_context_size is not None else 128
        R = right_context_size if right_context_size is not None else 128
        from .align import raise_failed
        feats = [_load_features(a, self.extract_features) for a in audio_paths]
        results, status = [None] * len(feats), [0] * len(feats)
        for grp in budget_groups([f.shape[0] for f in feats], total_batch_duration):
            xs = [feats[i] for i in grp]
            lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int)
            offset = torch.zeros(len(xs), dtype=torch.int)
            eo, el, n_chunks, _, _, _ = self.encoder.forward_parallel_chunk(xs, lens, C, L, R, offset=offset)
            el_ctc = [len(range(int(nc) * C)[: int(n)]) for nc, n in zip(n_chunks, el.tolist())]
            starts = (np.cumsum([0] + list(n_chunks[:-1])) * C).tolist()
            res, st = self.encoder.ctc_align(eo.reshape(-1, eo.shape[-1]), starts, el_ctc, [targets[i] for i in grp],
                                             max_workspace_bytes=max_workspace_bytes, return_status=True)
            for i, r, code in zip(grp, res, st):
                results[i], status[i] = r, code
        raise_failed(status)
        return results

    @torch.no_grad()
    def endless_align(self, audio_path: Features, target, chunk_size: Optional[int] = 64,
                      left_context_size: Optional[int] = 128, right_context_size: Optional[int] = 128,
                      total_batch_duration: int = 1800, max_workspace_bytes: Optional[int] = None, **endless_kwargs):
        """CTC forced alignment of one long recording: the encoder rows of
        endless_decode(..., return_encoder_out=True) aligned to the token ids `target` as one utterance
        -> align.AlignResult.  The trellis takes 4 bytes per frame and 16 states (`max_workspace_bytes`
        raises before anything is launched when it would be larger)."""
        self._require_ctc_align("endless_align")
        _, eo = self.endless_decode(audio_path, chunk_size, left_context_size, right_context_size,
                                    total_batch_duration=total_batch_duration, return_encoder_out=True,
                                    **endless_kwargs)
        rows = eo[0]
        return self.encoder.ctc_align(rows, [0], [rows.shape[0]], [target], max_workspace_bytes=max_workspace_bytes)[0]

    # ---------------------------------------------------------------- classification
    def _classify_rows(self, enc_rows: torch.Tensor, row_start, row_len):
        """One cfm_cls_classify call over packed encoder rows -> (pred [B, n_tasks], prob [B, n_tasks])."""
        pooled, logits, pred, prob = self.classifier.classify(enc_rows, row_start, row_len)
        self.last_classification = (pooled, logits)   # embeddings and logits of the last call, on the device
        return pred, prob

    def _label_dicts(self, pred: torch.Tensor, prob: torch.Tensor) -> List[dict]:
        """chunkformer_model.py:616-640 per utterance: {task: {"label", "label_id", "prob"}}, the label
        looked up in label_mapping[task] by str(label_id), falling back to the id string."""
        pred_h, prob_h = pred.cpu().tolist(), prob.cpu().tolist()
        out = []
        for ids, ps in zip(pred_h, prob_h):
            item = {}
            for task, label_id, p in zip(self.classifier.cfg.task_names, ids, ps):
                label = str(label_id)
                if self.label_mapping and task in self.label_mapping:
                    label = self.label_mapping[task].get(str(label_id), str(label_id))
                item[task] = {"label": label, "label_id": int(label_id), "prob": float(p)}
            out.append(item)
        return out

    @torch.no_grad()
    def classify(self, xs: torch.Tensor, xs_lens: torch.Tensor, chunk_size: int = -1, left_context_size: int = -1,
                 right_context_size: int = -1) -> Dict[str, torch.Tensor]:
        """SpeechClassificationModel.classify (classification_model.py:232-281) on a padded batch
        xs [B, T, 80]: encoder (any negative context argument = full attention, encoder.py:490-493),
        mean over each utterance's calc_length(len) valid frames, heads.  Returns
        {task}_prediction (int64 [B]) and {task}_probability (f32 [B]) on the device.  Pooling and
        heads run in f32 whatever the encoder dtype (the reference: under its autocast)."""
        self._require_classification()
        C, L, R = int(chunk_size), int(left_context_size), int(right_context_size)
        if C < 0 or L < 0 or R < 0:
            C = L = R = 0
        out, masks = self.encoder.forward_encoder(xs, xs_lens, C, L, R)
        B, Tp, d = out.shape
        lens = masks.squeeze(1).sum(-1).tolist()
        pred, prob = self._classify_rows(out.reshape(B * Tp, d), [b * Tp for b in range(B)], lens)
        res = {}
        for t, task in enumerate(self.classifier.cfg.task_names):
            res[f"{task}_prediction"] = pred[:, t].long()
            res[f"{task}_probability"] = prob[:, t].contiguous()
        return res

    @torch.no_grad()
    def classify_audio(self, audio_path: Features, chunk_size: Optional[int] = -1,
                       left_context_size: Optional[int] = -1, right_context_size: Optional[int] = -1) -> dict:
        """chunkformer_model.py:555-640: one input (a .wav path or fbank features, as _load_features
        takes them) -> {task: {"label", "label_id", "prob"}}."""
        self._require_classification()
        xs = _load_features(audio_path, self.extract_features)
        C = -1 if chunk_size is None else chunk_size
        L = -1 if left_context_size is None else left_context_size
        R = -1 if right_context_size is None else right_context_size
        res = self.classify(xs.unsqueeze(0), torch.tensor([xs.shape[0]]), C, L, R)
        names = self.classifier.cfg.task_names
        pred = torch.stack([res[f"{t}_prediction"] for t in names], dim=1)
        prob = torch.stack([res[f"{t}_probability"] for t in names], dim=1)
        return self._label_dicts(pred, prob)[0]

    @torch.no_grad()
    def batch_classify(self, audio_paths: List[Features], chunk_size: Optional[int] = 64,
                       left_context_size: Optional[int] = 128, right_context_size: Optional[int] = 128,
                       total_batch_duration: int = 1800) -> List[dict]:
        """Many inputs of uneven length on the masked batch (the bin/classify.py use case): the
        duration-budget grouping of batch_decode, one forward_parallel_chunk call and one
        cfm_cls_classify call per group -- utterance b is rows [cumsum(n_chunks)[b] * chunk_size,
        + calc_length(len_b)) of the packed encoder output, pooled and classified on the device
        without unpacking.  Returns one {task: {"label", "label_id", "prob"}} dict per input, in
        input order."""
        self._require_classification()
        C = chunk_size if chunk_size is not None else 64
        L = left_context_size if left_context_size is not None else 128
        R = right_context_size if right_context_size is not None else 128
        feats = [_load_features(a, self.extract_features) for a in audio_paths]
        results: List[dict] = []
        for grp in budget_groups([f.shape[0] for f in feats], total_batch_duration):
            xs = [feats[i] for i in grp]
            lens = torch.tensor([x.shape[0] for x in xs], dtype=torch.int)
            offset = torch.zeros(len(xs), dtype=torch.int)
            eo, el, n_chunks, _, _, _ = self.encoder.forward_parallel_chunk(xs, lens, C, L, R, offset=offset)
            el = [int(n) for n in el.tolist()]
            for i, n in zip(grp, el):
                if n <= 0:
                    what = audio_paths[i] if isinstance(audio_paths[i], str) else f"input {i}"
                    raise ValueError(f"{what}: {feats[i].shape[0]} frames are too few to classify "
                                     "(no encoder frame after subsampling)")
            starts = (np.cumsum([0] + list(n_chunks[:-1])) * C).tolist()
            pred, prob = self._classify_rows(eo.reshape(-1, eo.shape[-1]), starts, el)
            results.extend(self._label_dicts(pred, prob))
        return results


def transducer_decoder_config(conf: dict, sd: Dict[str, torch.Tensor], vocab: int, d_model: int):
    """The attention decoder of a `model: transducer` checkpoint for its rescoring modes: (AEDConfig, None) when the
    checkpoint carries decoder.* tensors the rescorer can run, (None, reason) when it carries some it cannot (settings
    AEDConfig.from_conf rejects, missing or mis-shaped tensors): the checkpoint then loads as it did without them and
    the reason is raised when a rescoring mode asks for attn_weight > 0; (None, None) without decoder.* tensors."""
    if not any(k.startswith("decoder.") for k in sd):
        return None, None
    try:
        if conf.get("decoder", "transformer") not in ("transformer", "bitransformer"):
            raise AssertionError(f"decoder: {conf.get('decoder')} is not transformer / bitransformer")
        aed_cfg = AEDConfig.from_conf(conf, vocab, d_model)
        from .rescore import native_names
        native_names(aed_cfg, sd)
        return aed_cfg, None
    except (AssertionError, KeyError, ValueError) as e:
        return None, str(e) or type(e).__name__


def _cmvn_from_stats(mean_stat, var_stat, count):
    mean = [m / count for m in mean_stat]
    istd = []
    for m, v in zip(mean, var_stat):
        var = v / count - m * m
        if var < 1.0e-20:
            var = 1.0e-20
        istd.append(1.0 / math.sqrt(var))
    return mean, istd


def load_json_cmvn(path: str):
    """utils/cmvn.py:23-45: JSON {mean_stat, var_stat, frame_num} -> (mean, istd)."""
    with open(path) as f:
        st = json.load(f)
    return _cmvn_from_stats(st["mean_stat"], st["var_stat"], st["frame_num"])


def load_kaldi_cmvn(path: str):
    """utils/cmvn.py:48-90: kaldi text stats `[ m_1 .. m_F count v_1 .. v_F 0 ]` -> (mean, istd);
    the binary kaldi form is rejected like the reference."""
    with open(path, "r") as f:
        if f.read(2) == "\0B":
            raise ValueError("kaldi cmvn binary file is not supported; recompute it with "
                             "compute-cmvn-stats --binary=false")
        f.seek(0)
        arr = f.read().split()
    if not (arr[0] == "[" and arr[-2] == "0" and arr[-1] == "]"):
        raise AssertionError(f"{path}: not a kaldi text cmvn file")
    F = (len(arr) - 4) // 2
    means = [float(a) for a in arr[1: F + 1]]
    count = float(arr[F + 1])
    var = [float(a) for a in arr[F + 2: 2 * F + 2]]
    return _cmvn_from_stats(means, var, count)
