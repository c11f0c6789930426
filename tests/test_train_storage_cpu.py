"""train_storage ('fp32' | '16bit', env MST_TRAIN_STORAGE) of DinoV2ClassifierSlice and the autocast bookkeeping of train_precision:
parsing, validation at construction and again at call time.  No GPU."""

import warnings

import pytest
import torch

from mst.models import DinoV2ClassifierSlice

ENV = ("MST_TRAIN_STORAGE", "MST_TRAIN_ATTENTION", "MST_TRAIN_PRECISION")


def _model(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, **kw)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def test_default_is_fp32_storage():
    assert _model().train_storage == "fp32"
    assert _model(train_precision="fp16", train_attention="flash").train_storage == "fp32"


def test_keyword_and_environment_are_read(monkeypatch):
    assert _model(train_precision="fp16", train_attention="flash", train_storage="16bit").train_storage == "16bit"
    assert _model(train_precision="bf16", train_attention="flash", train_storage="16BIT").train_storage == "16bit"
    monkeypatch.setenv("MST_TRAIN_STORAGE", "16bit")
    assert _model(train_precision="bf16", train_attention="flash").train_storage == "16bit"
    assert _model(train_precision="bf16", train_attention="flash", train_storage="fp32").train_storage == "fp32"      # the keyword wins
    assert _model(train_storage="fp32").train_storage == "fp32"
    with pytest.raises(ValueError):
        _model()                                                                   # environment 16bit with the fp32 step


@pytest.mark.parametrize("kw", [dict(train_storage="16bit"), dict(train_storage="16bit", train_precision="fp32", train_attention="stored"),
                                dict(train_storage="16bit", train_precision="fp16"),
                                dict(train_storage="16bit", train_precision="bf16", train_attention="stored"),
                                dict(train_storage="fp16", train_precision="fp16", train_attention="flash"), dict(train_storage="")])
def test_bad_combinations_raise(kw):
    with pytest.raises(ValueError):
        _model(**kw)


def test_the_step_rechecks_attributes_changed_after_construction():
    from mst.train_mode import check, resolve
    m = _model(train_precision="fp16", train_attention="flash", train_storage="16bit")
    assert resolve(m).storage16 is True
    m.train_attention = "stored"
    with pytest.raises(ValueError, match="train_storage"):
        resolve(m)
    m.train_attention, m.train_storage = "flash", "8bit"
    with pytest.raises(ValueError, match="train_storage"):
        resolve(m)
    m.train_storage, m.train_precision = "16bit", "fp32"
    with pytest.raises(ValueError):
        resolve(m)
    with pytest.raises(ValueError, match="train_storage"):
        check(False, "stored", m.train_storage, needs_flash=True)                  # the storage check itself, arguments by hand
    m.train_storage = "fp32"
    assert check(False, "stored", m.train_storage, needs_flash=True) == (False, False)      # (no 16-bit type, not flash: the arguments by hand)


def test_whether_train_precision_was_given_is_recorded(monkeypatch):
    """The autocast rule applies to a defaulted train_precision only; the attribute still reads 'fp32' then.  Outside an autocast region
    every model resolves to its own value."""
    from mst.train_mode import resolve
    m = _model()
    assert m.train_precision == "fp32" and m._train_precision_given is False and resolve(m).mp is None
    assert _model(train_precision="fp32")._train_precision_given is True
    assert _model(train_precision="bf16")._train_precision_given is True
    monkeypatch.setenv("MST_TRAIN_PRECISION", "fp32")
    assert _model()._train_precision_given is True
    monkeypatch.setenv("MST_TRAIN_PRECISION", "fp16")
    m = _model()
    assert m._train_precision_given is True and resolve(m).mp is torch.float16


def test_wrappers_refuse_host_tensors_and_wrong_types():
    from mst import hip
    x = torch.zeros(4, 384)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.residual_layernorm16(x, x.half(), None, None, None, 1e-6)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.act_fwd16(x.half(), 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.transpose16(x.bfloat16())
    with pytest.raises(TypeError):
        hip.act_fwd16(x, 0)                                                        # fp32 where a 16-bit tensor is expected
