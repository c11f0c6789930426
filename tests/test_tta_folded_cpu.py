"""Folded test-time augmentation (mst.saliency.run_pred(tta="folded"), csrc/k_tta.hip), the parts that need no GPU: the C ABI of the
two new entry points, the refusals run_pred makes before anything touches a device, and a check of the GPU test's own teeth -- on
the two order-sensitive models of tests/tta_ref.py the oracle's answer is told apart from two wrong readings of the folding
(the padding mask mirrored together with D; depth-flipped variants fed the slices in their original order) by more than 10x the
fp32 bar, so a folded path that made either mistake could not pass tests/test_tta_folded_gpu.py."""
import re
import types
from pathlib import Path

import pytest
import torch

import tta_ref as R
from conftest import rel_l2
from mst import hip

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("mst_tta_inplane_flips", "mst_saliency_accumulate_tta")


def test_new_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "mst_hip.h").read_text()
    lib = hip.load()
    for sym in NEW_SYMBOLS:
        assert sym in hip.SIGNATURES, sym
        assert hasattr(lib, sym), f"{sym} is not exported"
        decl = re.search(r"^int\s+" + sym + r"\s*\(([^;]*)\);", header, flags=re.M | re.S)
        assert decl, f"{sym} is not declared in include/mst_hip.h"
        assert len(decl.group(1).split(",")) == len(hip.SIGNATURES[sym][1]), sym
    assert "main_predict.py:147-158" in header          # the entries cite the lines of the script they fold


def test_entry_points_refuse_bad_arguments_before_a_launch():
    """Calls that fail an entry point's argument checks: the addresses are made up and never dereferenced."""
    lib = hip.load()
    a, b, c, d = 0x1000, 0x2000, 0x3000, 0x4000
    assert lib.mst_tta_inplane_flips(None, hip.F32, 1, 4, 4, b, None) != 0
    assert lib.mst_tta_inplane_flips(a, hip.F32, 1, 4, 4, a, None) != 0               # not in place
    assert lib.mst_tta_inplane_flips(a, 7, 1, 4, 4, b, None) != 0 and "dtype" in hip.last_error()
    assert lib.mst_tta_inplane_flips(a, hip.BF16, 1, 4, 0, b, None) != 0
    assert lib.mst_tta_inplane_flips(a, hip.F32, 1, 4, 16385, b, None) != 0 and "LDS" in hip.last_error()
    assert lib.mst_saliency_accumulate_tta(None, b, 5, 6, 4, 4, 16, c, d, None) != 0
    assert lib.mst_saliency_accumulate_tta(a, None, 5, 6, 4, 4, 16, c, d, None) != 0   # the sum itself needs the slice attention
    assert lib.mst_saliency_accumulate_tta(a, b, 5, 6, 4, 4, 16, None, d, None) != 0
    assert lib.mst_saliency_accumulate_tta(a, b, 5, 6, 5, 4, 16, c, d, None) != 0 and "does not fit" in hip.last_error()
    assert lib.mst_saliency_accumulate_tta(a, b, 0, 6, 4, 4, 16, c, None, None) != 0


def test_wrappers_refuse_host_tensors_and_wrong_types():
    with pytest.raises(TypeError):
        hip.tta_inplane_flips(torch.zeros(2, 4, 4, dtype=torch.float64))
    with pytest.raises(TypeError):
        hip.tta_inplane_flips([[1.0]])
    with pytest.raises(ValueError):
        hip.tta_inplane_flips(torch.zeros(2, 4, 4, 4))                                # rank
    with pytest.raises(ValueError):
        hip.tta_inplane_flips(torch.zeros(0, 4, 4))                                   # empty
    with pytest.raises(ValueError):
        hip.tta_inplane_flips(torch.zeros(2, 4, 4))                                   # a host tensor
    plane, sa, low, ws = torch.zeros(4, 5, 6, 16), torch.zeros(8, 5), torch.zeros(5, 4, 4), torch.zeros(5)
    with pytest.raises(TypeError):
        hip.saliency_accumulate_tta(plane.half(), sa, 4, 4, low, ws)
    with pytest.raises(ValueError):
        hip.saliency_accumulate_tta(plane[:3], sa, 4, 4, low, ws)
    with pytest.raises(ValueError):
        hip.saliency_accumulate_tta(plane, sa[:7], 4, 4, low, ws)
    with pytest.raises(ValueError):
        hip.saliency_accumulate_tta(plane, sa, 5, 4, low, ws)                         # 20 columns of 16
    with pytest.raises(ValueError):
        hip.saliency_accumulate_tta(plane, sa, 4, 4, low, ws)                         # host tensors


def test_run_pred_validates_tta_before_the_library_is_loaded(monkeypatch):
    from mst import saliency
    from mst.models import DinoV2ClassifierSlice

    def no_library():
        raise AssertionError("run_pred reached the library before refusing its arguments")
    monkeypatch.setattr(hip, "load", no_library)
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False)
    batch = {"source": torch.zeros(1, 1, 2, 28, 28)}
    for kwargs in (dict(), dict(use_tta=True)):                                       # the value is checked whether or not it is used
        with pytest.raises(ValueError, match="'loop' or 'folded'"):
            saliency.run_pred(model, batch, tta="fold", **kwargs)
    model._sharding = types.SimpleNamespace(world_size=2)
    with pytest.raises(NotImplementedError, match="shard"):
        saliency.run_pred(model, batch, use_tta=True, tta="folded")
    with pytest.raises(TypeError):
        saliency.run_pred(torch.nn.Linear(2, 2), batch, use_tta=True, tta="folded")
    with pytest.raises(TypeError):
        saliency.run_pred(torch.nn.Linear(2, 2), batch, tta="neither")               # the model's refusal comes first


@pytest.mark.parametrize("name", list(R.ORDER_CASES))
def test_restatement_is_the_oracle_and_wrong_readings_are_not(name):
    """The folded algorithm restated on the oracle's pieces equals oracle.run_pred (eight whole forwards) far inside the fp32 bars;
    each wrong reading misses pred or weight by more than 10x the fp32 bar."""
    tl, tm = R.TOL["fp32"]
    pred, weight, ws = R.oracle_run_pred(name)
    p, w, s = R.restated_run_pred(name)
    right = (float((p - pred).abs().max()), rel_l2(w, weight), rel_l2(s, ws))
    print(f"{name}: restatement vs oracle: pred {right[0]:.2e} weight {right[1]:.2e} weight_slice {right[2]:.2e}")
    assert right[0] < tl / 10 and right[1] < tm / 10 and right[2] < tm / 10, right
    for wrong in (dict(flip_mask_with_d=True), dict(reverse_embeddings=False)):
        p, w, s = R.restated_run_pred(name, **wrong)
        dp, dw = float((p - pred).abs().max()), rel_l2(w, weight)
        print(f"{name}: {wrong}: pred off by {dp:.2e}, weight by {dw:.2e}")
        assert dp > 10 * tl or dw > 10 * tm, (wrong, dp, dw)
