"""CPU-side checks of the classification consumer: config parsing, the C-ABI exports and the
self-consistency of the reference-generated fixture (tests/golden/gen_golden_classification.py)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLS_SYMBOLS = ["cfm_cls_create", "cfm_cls_destroy", "cfm_cls_pool_workspace_bytes", "cfm_cls_workspace_bytes",
               "cfm_cls_pool", "cfm_cls_classify"]


@pytest.fixture(scope="module")
def lib():
    from chunkformer_amd import build
    build.build()
    from chunkformer_amd import _lib
    return _lib


def test_config_from_conf_keeps_task_order(lib):
    from chunkformer_amd.classifier import ClassifierConfig, schema
    conf = {"model": "classification", "model_conf": {"tasks": {"region": 5, "gender": 2, "emotion": 7}}}
    c = ClassifierConfig.from_conf(conf, enc_dim=128)
    assert list(c.tasks.items()) == [("region", 5), ("gender", 2), ("emotion", 7)]
    assert c.task_names == ["region", "gender", "emotion"] and c.sum_classes == 14 and c.enc_dim == 128
    assert schema(c)[:2] == [("classification_heads.region.linear.weight", (5, 128)),
                             ("classification_heads.region.linear.bias", (5,))]


@pytest.mark.parametrize("conf", [{"model_conf": {"tasks": {}}}, {"model_conf": {}}, {}])
def test_config_empty_tasks_raises(lib, conf):
    from chunkformer_amd.classifier import ClassifierConfig
    with pytest.raises(ValueError):
        ClassifierConfig.from_conf(conf)


def test_classification_symbols_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "cfm.h")).read()
    declared = set(re.findall(r"\b(cfm_[a-z_]+)\s*\(", hdr))
    for name in CLS_SYMBOLS:
        assert name in declared, f"include/cfm.h does not declare {name}"
        assert hasattr(lib.lib, name), f"libcfm.so does not export {name}"
        assert name in lib.EXPORTED
    assert set(lib.EXPORTED) == declared


def test_pool_workspace_layout(lib):
    """slab offsets [B + 1] int32 padded to 256 bytes + (ceil(rows / 64) + B) partial rows of d floats."""
    assert lib.cfm_cls_pool_workspace_bytes(1000, 128, 3) == 256 + (16 + 3) * 128 * 4
    assert lib.cfm_cls_pool_workspace_bytes(64, 512, 1) == 256 + 2 * 512 * 4


def test_synthetic_classifier_state_dict(lib):
    from chunkformer_amd.config import SMALL
    from chunkformer_amd.weights import synthetic_classifier_state_dict, synthetic_state_dict
    import dataclasses
    sd = synthetic_classifier_state_dict(SMALL, {"a": 3, "b": 1}, seed=4)
    assert "ctc.ctc_lo.weight" not in sd
    assert tuple(sd["classification_heads.a.linear.weight"].shape) == (3, SMALL.d_model)
    assert tuple(sd["classification_heads.b.linear.bias"].shape) == (1,)
    enc = synthetic_state_dict(dataclasses.replace(SMALL, vocab=0), 4)
    assert all((sd[k] == v).all() for k, v in enc.items())


def test_fixture_self_consistent(golden_dir):
    g = np.load(os.path.join(golden_dir, "classification.npz"))
    names = [str(n) for n in g["task_names"]]
    assert names == ["gender", "emotion", "region"] and g["task_classes"].tolist() == [2, 7, 5]
    B = len(g["lens"])
    for geo in ("full", "chunk", "packed"):
        pooled = g[f"{geo}_pooled"].astype(np.float64)
        assert pooled.shape == (B, 128)
        for n in names:
            logits = g[f"{geo}_logits_{n}"]
            pred = g[f"{geo}_prediction_{n}"]
            np.testing.assert_array_equal(pred, logits.argmax(-1))
            l64 = logits.astype(np.float64)
            sm = np.exp(l64 - l64.max(-1, keepdims=True))
            sm /= sm.sum(-1, keepdims=True)
            np.testing.assert_allclose(g[f"{geo}_probability_{n}"], sm[np.arange(B), pred], rtol=1e-5, atol=0)
            # the stored logits are the stored heads applied to the stored pooled vectors
            ref = pooled @ g[f"w_{n}"].astype(np.float64).T + g[f"b_{n}"]
            np.testing.assert_allclose(l64, ref, rtol=0, atol=1e-4)
            assert len(set(pred.tolist())) >= 2, f"{geo}/{n}: every utterance has the same class"
            # the generator's guarantee: every top-2 margin is at least twice the fp32 logit bar
            bar = 1e-4 * np.abs(g[f"w_{n}"]).sum(1).max() + 1e-6
            top = np.sort(l64, -1)
            assert (top[:, -1] - top[:, -2]).min() >= 2 * bar
