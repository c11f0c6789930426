"""train_storage ('fp32' | '16bit', env MST_RESNET_TRAIN_STORAGE) of ResNet / ResNetSliceTrans and the autocast bookkeeping of their
train_precision: parsing, validation at construction and at call time, and the header / binding agreement of the new entry points.  No GPU."""

import re
import warnings
from pathlib import Path

import pytest
import torch

from mst.models import ResNet, ResNetSliceTrans

ROOT = Path(__file__).resolve().parent.parent
ENV = ("MST_RESNET_TRAIN_STORAGE", "MST_TRAIN_STORAGE", "MST_TRAIN_PRECISION")
NEW_SYMBOLS = ("mst_batchnorm_train16_workspace_bytes", "mst_batchnorm_train16", "mst_batchnorm_bwd16_workspace_bytes", "mst_batchnorm_bwd16",
               "mst_maxpool_bwd_nhwc16_workspace_bytes", "mst_maxpool_bwd_nhwc16", "mst_avgpool_nhwc16")


def _slice(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ResNetSliceTrans(in_ch=1, out_ch=2, pretrained=False, model=18, **kw)


def _plain(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ResNet(in_ch=3, out_ch=2, spatial_dims=2, model=18, **kw)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("build", [_slice, _plain])
def test_default_keyword_and_environment(build, monkeypatch):
    assert build().train_storage == "fp32"
    assert build(train_precision="fp16").train_storage == "fp32"
    assert build(train_precision="fp16", train_storage="16bit").train_storage == "16bit"
    assert build(train_precision="bf16", train_storage="16BIT").train_storage == "16bit"
    monkeypatch.setenv("MST_RESNET_TRAIN_STORAGE", "16bit")
    assert build(train_precision="bf16").train_storage == "16bit"
    assert build(train_precision="bf16", train_storage="fp32").train_storage == "fp32"       # the keyword wins
    with pytest.raises(ValueError, match="train_storage"):
        build()                                                                               # environment 16bit with the fp32 step


@pytest.mark.parametrize("build", [_slice, _plain])
def test_the_dinov2_variable_does_not_reach_a_resnet(build, monkeypatch):
    monkeypatch.setenv("MST_TRAIN_STORAGE", "16bit")
    assert build().train_storage == "fp32"
    assert build(train_precision="fp16").train_storage == "fp32"


@pytest.mark.parametrize("build", [_slice, _plain])
@pytest.mark.parametrize("kw", [dict(train_storage="16bit"), dict(train_storage="16bit", train_precision="fp32"),
                                dict(train_storage="fp16", train_precision="fp16"), dict(train_storage="8bit", train_precision="bf16"),
                                dict(train_storage="")])
def test_bad_combinations_raise(build, kw):
    with pytest.raises(ValueError, match="train_storage"):
        build(**kw)


def test_the_step_rechecks_attributes_changed_after_construction():
    from mst.train_mode import check, resolve
    m = _slice(train_precision="fp16", train_storage="16bit")
    assert resolve(m).storage16 is True
    m.train_precision = "fp32"
    with pytest.raises(ValueError, match="train_storage"):
        resolve(m)
    m.train_precision, m.train_storage = "bf16", "8bit"
    with pytest.raises(ValueError, match="train_storage"):
        resolve(m)
    m.train_storage = "fp32"
    assert resolve(m).storage16 is False
    assert check(False, "stored", m.train_storage, needs_flash=False) == (False, False)     # (no 16-bit type: the arguments by hand)


@pytest.mark.parametrize("build", [_slice, _plain])
def test_whether_train_precision_was_given_is_recorded(build, monkeypatch):
    """The autocast rule applies to a defaulted train_precision only; the attribute still reads 'fp32' then, and outside a region every
    model resolves to its own value."""
    from mst.train_mode import resolve
    m = build()
    assert m.train_precision == "fp32" and m._train_precision_given is False and resolve(m).mp is None
    assert build(train_precision="fp32")._train_precision_given is True
    assert build(train_precision="bf16")._train_precision_given is True
    monkeypatch.setenv("MST_TRAIN_PRECISION", "fp32")
    assert build()._train_precision_given is True
    monkeypatch.setenv("MST_TRAIN_PRECISION", "fp16")
    m = build()
    assert m._train_precision_given is True and resolve(m).mp is torch.float16


def test_the_unit_refuses_16_bit_storage_without_a_16_bit_type():
    from mst import train_resnet
    with pytest.raises(ValueError, match="train_storage"):
        train_resnet._conv_bn_fwd(torch.zeros(1, 4, 4, 64), None, None, 3, 1, 1, False, None, True, None, True)


def test_header_declares_every_new_symbol_the_binding_names():
    from mst import hip
    header = (ROOT / "include" / "mst_hip.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t)\s+(mst_[a-z0-9_]+)\s*\(", header, flags=re.M))
    lib = hip.load()
    for sym in NEW_SYMBOLS:
        assert sym in hip.SIGNATURES, sym
        assert sym in declared, f"{sym} is bound but not declared in include/mst_hip.h"
        assert hasattr(lib, sym), f"{sym} is not exported"
        # the binding passes as many arguments as the declaration takes
        decl = re.search(r"^(?:int|size_t)\s+" + sym + r"\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(hip.SIGNATURES[sym][1]), sym
    assert lib.mst_version() == 300


def test_wrappers_refuse_host_tensors_and_wrong_types():
    from mst import hip
    z = torch.zeros(8, 64)
    with pytest.raises(TypeError):
        hip.batchnorm_train16(z, None, None, True)                                         # fp32 where a 16-bit tensor is expected
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.batchnorm_train16(z.half(), None, None, True)
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.batchnorm_bwd16(z.half(), None, z[0], z[0], z[0], z, False)
