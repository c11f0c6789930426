"""The train_attention keyword of DinoV2ClassifierSlice (memory-efficient attention in the mixed-precision training step): default, keyword,
environment default, and the combinations that raise -- at construction and again in the step.  No GPU needed."""
import warnings

import pytest
import torch


def _model(**kw):
    from mst.models import DinoV2ClassifierSlice
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, **kw)


def test_default_keeps_the_probabilities(monkeypatch):
    monkeypatch.delenv("MST_TRAIN_ATTENTION", raising=False)
    assert _model().train_attention == "stored"
    assert _model(train_precision="bf16").train_attention == "stored"


def test_keyword_and_environment_are_read(monkeypatch):
    monkeypatch.delenv("MST_TRAIN_ATTENTION", raising=False)
    assert _model(train_precision="fp16", train_attention="flash").train_attention == "flash"
    assert _model(train_precision="bf16", train_attention="FLASH").train_attention == "flash"
    monkeypatch.setenv("MST_TRAIN_ATTENTION", "flash")
    assert _model(train_precision="bf16").train_attention == "flash"
    assert _model(train_precision="bf16", train_attention="stored").train_attention == "stored"   # the keyword wins
    with pytest.raises(ValueError):
        _model()                                                                  # environment flash with the fp32 step


@pytest.mark.parametrize("kw", [dict(train_attention="flash"), dict(train_attention="flash", train_precision="fp32"),
                                dict(train_attention="tiled", train_precision="bf16"), dict(train_attention="")])
def test_bad_combinations_raise(monkeypatch, kw):
    monkeypatch.delenv("MST_TRAIN_ATTENTION", raising=False)
    with pytest.raises(ValueError):
        _model(**kw)


def test_the_step_rechecks_attributes_changed_after_construction(monkeypatch):
    from mst.train_mode import resolve
    monkeypatch.delenv("MST_TRAIN_ATTENTION", raising=False)
    m = _model(train_precision="fp16", train_attention="flash")
    assert resolve(m).flash is True
    m.train_precision = "fp32"
    with pytest.raises(ValueError, match="train_precision"):
        resolve(m)
    m.train_precision, m.train_attention = "bf16", "paged"
    with pytest.raises(ValueError):
        resolve(m)
    m.train_attention = "stored"
    assert resolve(m).flash is False


def test_wrappers_refuse_host_tensors():
    from mst import hip
    qkv = torch.zeros(4, 3 * 6 * 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.attention_train_fwd(qkv, 1, 4, 6)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.attention_train_bwd(qkv, torch.zeros(4, 384), torch.zeros(4, 384), torch.zeros(1, 6, 4), 1, 4, 6)
