"""The host side of the ResNet input-volume gradient: the C ABI declares and exports mst_conv_dgrad_stem (additively: the ABI version is
unchanged), and its binding refuses wrong operands before the library is reached."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from mst import hip

ROOT = Path(__file__).resolve().parents[1]


def test_header_declares_and_library_exports_the_stem_data_gradient():
    header = (ROOT / "include" / "mst_hip.h").read_text()
    m = re.search(r"int\s+mst_conv_dgrad_stem\s*\(([^;]*)\)\s*;", header)
    assert m, "include/mst_hip.h does not declare mst_conv_dgrad_stem"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 16 and args[0].startswith("const void*") and args[-2].startswith("float*") and args[-1].startswith("mst_stream_t")
    assert len(hip.SIGNATURES["mst_conv_dgrad_stem"][1]) == 16
    lib = ctypes.CDLL(str(hip.LIB_PATH))
    assert hasattr(lib, "mst_conv_dgrad_stem")
    assert "k_conv_stem_dgrad.hip" in {p.name for p in (ROOT / "new-vit_amd" / "csrc").glob("*.hip")}


def test_abi_version_is_unchanged():
    lib = ctypes.CDLL(str(hip.LIB_PATH))
    lib.mst_version.restype = ctypes.c_int
    assert lib.mst_version() == 300 == hip.ABI_VERSION


def test_binding_rejects_bad_operands_before_the_library():
    dz = torch.zeros(2, 8, 8, 64)
    wg = torch.zeros(64, 49)
    with pytest.raises(ValueError, match="HIP device"):                    # CPU tensors
        hip.conv_dgrad_stem(dz, wg, 7, 2, 3, 16, 16, 1)
    with pytest.raises(ValueError, match="does not match"):                # weight of another channel count
        hip.conv_dgrad_stem(dz, torch.zeros(64, 147), 7, 2, 3, 16, 16, 1)
    with pytest.raises(ValueError, match="does not match"):                # padded GEMM weight
        hip.conv_dgrad_stem(dz, torch.zeros(64, 64), 7, 2, 3, 16, 16, 1)
    with pytest.raises(TypeError, match="wg is"):                          # operand types differ
        hip.conv_dgrad_stem(dz.half(), wg, 7, 2, 3, 16, 16, 1)
    with pytest.raises(TypeError):
        hip.conv_dgrad_stem(dz.double(), wg.double(), 7, 2, 3, 16, 16, 1)
    with pytest.raises(TypeError):
        hip.conv_dgrad_stem(dz.numpy(), wg, 7, 2, 3, 16, 16, 1)
    with pytest.raises(ValueError, match=r"\[n, Ho, Wo, Cout\]"):
        hip.conv_dgrad_stem(dz.view(-1, 64), wg, 7, 2, 3, 16, 16, 1)
