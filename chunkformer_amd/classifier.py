"""Classification consumer of the encoder: what the reference runs for `model: classification`
checkpoints (SpeechClassificationModel, modules/classification_model.py) on top of the encoder hot
path, as HIP kernels (csrc/classify.hip, cfm_cls_* in include/cfm.h).

  _average_pooling   classification_model.py:174-200   -> ClassifierHeads.pool
  classify (heads)   classification_model.py:263-281   -> ClassifierHeads.classify

Utterances are row ranges of a packed [rows, d] encoder output, so a padded batch ([B, T', d], rows
b * T' ...) and a masked batch (rows cumsum(n_chunks) * chunk_size ...) go through the same call; the
padded tails and chunk tails between the ranges are never read.

Pooling and heads always compute in f32, whatever the encoder's compute dtype.  The reference runs
its heads under the caller's fp16 autocast; f32 is the more exact of the two, so 16-bit results can
differ from the reference's in the last bits of a probability, never by more than its own rounding.
The summation order is fixed: two calls on the same input are bit-identical.
"""
from __future__ import annotations

import ctypes
import weakref
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import torch

from . import _lib

MAX_TASKS = _lib.CLS_MAX_TASKS


@dataclass
class ClassifierConfig:
    tasks: "Dict[str, int]" = field(default_factory=OrderedDict)   # task name -> classes, in model_conf order
    enc_dim: int = 512

    @classmethod
    def from_conf(cls, conf: dict, enc_dim: int = 512) -> "ClassifierConfig":
        """From a reference config.yaml: model_conf.tasks (init_model.py:106-111)."""
        tasks = dict((conf.get("model_conf") or {}).get("tasks") or {})
        if not tasks:
            raise ValueError("Classification model requires 'tasks' in model_conf")
        return cls(tasks=OrderedDict((str(k), int(v)) for k, v in tasks.items()), enc_dim=int(enc_dim))

    @property
    def task_names(self) -> List[str]:
        return list(self.tasks.keys())

    @property
    def sum_classes(self) -> int:
        return sum(self.tasks.values())


def schema(c: ClassifierConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of every head tensor, keys as in the reference SpeechClassificationModel."""
    out: List[Tuple[str, Tuple[int, ...]]] = []
    for name, n in c.tasks.items():
        out += [(f"classification_heads.{name}.linear.weight", (n, c.enc_dim)),
                (f"classification_heads.{name}.linear.bias", (n,))]
    return out


def _row_arrays(row_start, row_len, rows: int, device):
    rs, rl = _lib.packed_ranges(row_start, row_len, rows, "encoder rows")
    return rs.to(device), rl.to(device)


def masked_mean_pool(enc: torch.Tensor, row_start, row_len) -> torch.Tensor:
    """cfm_cls_pool: pooled[b] = sum of rows [row_start[b], +row_len[b]) of enc [rows, d] / (row_len[b] +
    1e-10), f32 [B, d] on enc's device (zeros for an empty range).  Needs no model."""
    d = enc.shape[-1]
    enc = enc.reshape(-1, d).to(torch.float32).contiguous()
    rows, dev = enc.shape[0], enc.device
    rs, rl = _row_arrays(row_start, row_len, rows, dev)
    B = rs.numel()
    pooled = torch.empty(B, d, dtype=torch.float32, device=dev)
    if B == 0:
        return pooled
    nbytes = int(_lib.cfm_cls_pool_workspace_bytes(rows, d, B))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.cfm_cls_pool(enc.data_ptr(), rows, d, rs.data_ptr(), rl.data_ptr(), B, pooled.data_ptr(),
                                     ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream))
    return pooled


class ClassifierHeads:
    """Masked mean pool + every task's Linear head, argmax and softmax probability on libcfm
    (cfm_cls_*), in f32 (see the module docstring)."""

    def __init__(self, cfg: ClassifierConfig, state_dict: Dict[str, torch.Tensor], device):
        if not cfg.tasks:
            raise ValueError("At least one classification task must be defined")
        if len(cfg.tasks) > MAX_TASKS:
            raise ValueError(f"{len(cfg.tasks)} classification tasks: at most {MAX_TASKS} are supported")
        self.cfg = cfg
        self.device = torch.device(device)
        for name, shape in schema(cfg):
            if name not in state_dict:
                raise ValueError(f"missing weight {name}")
            if tuple(state_dict[name].shape) != tuple(shape):
                raise ValueError(f"weight {name}: shape {tuple(state_dict[name].shape)} != {shape}")
        c = _lib.CfmClsConfig()
        c.enc_dim, c.n_tasks = int(cfg.enc_dim), len(cfg.tasks)
        for i, n in enumerate(cfg.tasks.values()):
            c.num_classes[i] = int(n)
        names = [n for n, _ in schema(cfg)]    # {weight, bias} per task, in task order
        keep = []
        views = (_lib.CfmTensorView * len(names))()
        for i, k in enumerate(names):
            t = state_dict[k].detach().to("cpu", torch.float32).contiguous()
            keep.append(t)
            views[i] = _lib.CfmTensorView(k.encode(), t.data_ptr(), t.numel())
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.cfm_cls_create(ctypes.byref(c), views, len(names), self.device.index or 0,
                                           ctypes.byref(h)))
        self._h = h
        self._finalizer = weakref.finalize(self, _lib.cfm_cls_destroy, ctypes.c_void_p(h.value))

    @torch.no_grad()
    def pool(self, enc: torch.Tensor, row_start, row_len) -> torch.Tensor:
        """_average_pooling over utterances b = rows [row_start[b], row_start[b] + row_len[b]) of
        enc [rows, d]: f32 [B, d]."""
        return masked_mean_pool(enc.to(self.device), row_start, row_len)

    @torch.no_grad()
    def classify(self, enc: torch.Tensor, row_start, row_len):
        """One cfm_cls_classify call: (pooled [B, d] f32, logits [B, sum_classes] f32 with the tasks'
        logits side by side in task order, pred [B, n_tasks] int32, prob [B, n_tasks] f32), all on
        the device; prob = softmax(logits_task)[pred]."""
        d, dev = self.cfg.enc_dim, self.device
        if enc.shape[-1] != d:
            raise ValueError(f"encoder width {enc.shape[-1]} != enc_dim {d}")
        enc = enc.reshape(-1, d).to(dev, torch.float32).contiguous()
        rows = enc.shape[0]
        rs, rl = _row_arrays(row_start, row_len, rows, dev)
        B, T, S = rs.numel(), len(self.cfg.tasks), self.cfg.sum_classes
        pooled = torch.empty(B, d, dtype=torch.float32, device=dev)
        logits = torch.empty(B, S, dtype=torch.float32, device=dev)
        pred = torch.empty(B, T, dtype=torch.int32, device=dev)
        prob = torch.empty(B, T, dtype=torch.float32, device=dev)
        if B == 0:
            return pooled, logits, pred, prob
        nbytes = int(_lib.cfm_cls_workspace_bytes(self._h, rows, B))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        _lib.check(_lib.cfm_cls_classify(self._h, enc.data_ptr(), rows, rs.data_ptr(), rl.data_ptr(), B,
                                         pooled.data_ptr(), logits.data_ptr(), pred.data_ptr(), prob.data_ptr(),
                                         ws.data_ptr(), nbytes, stream.cuda_stream))
        return pooled, logits, pred, prob

    def split_logits(self, logits: torch.Tensor) -> Dict[str, torch.Tensor]:
        """[B, sum_classes] -> {task: [B, classes]} (views)."""
        return dict(zip(self.cfg.task_names, logits.split(list(self.cfg.tasks.values()), dim=-1)))
