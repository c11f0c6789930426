"""CPU-side checks of the fixed-order (deterministic) entry points: every one the header declares has a ctypes signature, the library
exports it, and the workspace queries (host functions) size the slabs the order contract describes."""
import re
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent

ORDERED = ("mst_colsum_ordered", "mst_layernorm_bwd_ordered", "mst_batchnorm_train_ordered", "mst_batchnorm_bwd_ordered",
           "mst_col2im_nhwc_gather", "mst_maxpool_bwd_nhwc_gather", "mst_pos_embed_interp_bwd_ordered", "mst_znorm_ordered")


def test_every_ordered_entry_point_is_declared_bound_and_exported():
    from mst import hip
    header = (ROOT / "include" / "mst_hip.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t)\s+(mst_[a-z0-9_]+(?:_ordered|_gather)[a-z_]*)\s*\(", header, flags=re.M))
    for name in ORDERED:
        assert name in declared, name
        if name != "mst_col2im_nhwc_gather":                             # the only one without a workspace
            assert name + "_workspace_bytes" in declared, name
    missing = sorted(declared - set(hip.SIGNATURES))
    assert not missing, f"header symbols without a ctypes signature: {missing}"
    lib = hip.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.mst_version() == 300                                      # additions only: the ABI version stays


def test_workspace_queries_follow_the_row_block_plan():
    from mst import hip
    lib = hip.load()
    # the stem's BatchNorm sums of a 2 x 128 x 512^2 step: 16.8 M rows x 64 columns -> 2,048 row blocks of 8,192 rows
    assert lib.mst_colsum_ordered_workspace_bytes(2 * 128 * 256 * 256, 64) == 2048 * 64 * 4
    # ViT-L fc weight-gradient partials: 16 rows x 4,194,304 columns is one row block (added in place, no slab), past 65,535 column blocks
    assert lib.mst_colsum_ordered_workspace_bytes(16, 4194304) == 0
    assert lib.mst_batchnorm_bwd_ordered_workspace_bytes(2 * 128 * 256 * 256, 64) == 2048 * 2 * 64 * 4
    assert lib.mst_batchnorm_train_ordered_workspace_bytes(2 * 128 * 256 * 256, 64) == 256 + 2048 * 64 * 4
    assert lib.mst_layernorm_bwd_ordered_workspace_bytes(4112, 384) == 257 * 2 * 384 * 4
    assert lib.mst_layernorm_bwd_ordered_workspace_bytes(100000, 1024) == 1024 * 2 * 1024 * 4
    assert lib.mst_maxpool_bwd_nhwc_gather_workspace_bytes(2, 256, 256, 64) == 2 * 128 * 128 * 64
    assert lib.mst_pos_embed_interp_bwd_ordered_workspace_bytes(37, 384, 16, 16) == 16 * 37 * 384 * 4
    assert lib.mst_znorm_ordered_workspace_bytes(1 << 26) == 4096 * 8
    assert lib.mst_znorm_ordered_workspace_bytes(1000) == 256                 # 4 workgroups, rounded up to 256 bytes


def test_deterministic_helper_follows_the_torch_flag():
    from mst import hip
    prev, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert not hip.deterministic()
        torch.use_deterministic_algorithms(True)
        assert hip.deterministic()
        torch.use_deterministic_algorithms(True, warn_only=True)          # nothing to warn about: the ordered forms exist
        assert hip.deterministic()
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=warn)
    assert hip.workspace(0, "cpu") is None and hip.workspace(300, "cpu").numel() == 300
