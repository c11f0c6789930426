"""Device-side training augmentation (mst/augment.py, csrc/k_augment.hip), the parts that need no GPU: the new C ABI symbols, the refusal
of host tensors, the distributions and the reproducibility of the host-side draws, the random crop offsets, the restatement's own
generator against Philox's published vectors, and the cap on what the GPU rotation test may leave out.

Bounds of the distribution checks are 5 sigma of the estimator over N = 4000 draws, derived and not measured:
    frequency of a p = 0.5 event      sigma = sqrt(0.25 / N)      = 0.0079   -> 0.5 +- 0.04
    mean of U(0, 90) degrees          sigma = 90 / sqrt(12 N)     = 0.411    -> 45 +- 2.1
    mean of U(0, 0.25)                sigma = 0.25 / sqrt(12 N)   = 0.00114  -> 0.125 +- 0.006"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_ref as R
from mst import hip, preprocess
from mst.augment import TrainAugment

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("mst_augment_volumes", "mst_volume_min", "mst_crop_or_pad_at")
N_DRAWS = 4000


def test_new_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "mst_hip.h").read_text()
    lib = hip.load()
    for sym in NEW_SYMBOLS:
        assert sym in hip.SIGNATURES, sym
        assert hasattr(lib, sym), f"{sym} is not exported"
        decl = re.search(r"^int\s+" + sym + r"\s*\(([^;]*)\);", header, flags=re.M | re.S)
        assert decl, f"{sym} is not declared in include/mst_hip.h"
        assert len(decl.group(1).split(",")) == len(hip.SIGNATURES[sym][1]), sym
    # each entry point cites the reference lines it replaces, and the header says what is not pinned
    assert "dataset_3d_duke.py:44-47" in header and "augmentations_3d.py:166-195" in header
    assert "NOT pinned against torchio" in header
    # the old entry point keeps its signature
    assert len(hip.SIGNATURES["mst_crop_or_pad"][1]) == 13


def test_entry_points_refuse_null_and_empty_arguments():
    """Only calls that fail an entry point's FIRST check (a null pointer, an empty shape, in == out): the addresses are made up and never
    dereferenced.  Checks behind the first one are tested with real device buffers (tests/test_augment_gpu.py)."""
    lib = hip.load()
    a, b, p = 0x1000, 0x2000, 0x3000
    assert lib.mst_augment_volumes(a, hip.F32, a, hip.F32, 1, 2, 4, 4, p, 0, 0, None) != 0 and "not in place" in hip.last_error()
    assert lib.mst_augment_volumes(a, hip.F32, b, hip.F32, 1, 2, 4, 0, p, 0, 0, None) != 0
    assert lib.mst_augment_volumes(a, hip.F32, b, hip.F32, 0, 2, 4, 4, p, 0, 0, None) != 0
    assert lib.mst_augment_volumes(a, hip.F32, b, hip.F32, 1, 2, 4, 4, None, 0, 0, None) != 0
    assert lib.mst_augment_volumes(None, hip.F32, b, hip.F32, 1, 2, 4, 4, p, 0, 0, None) != 0
    assert lib.mst_volume_min(a, hip.F32, 1, 0, b, 1, None) != 0 and lib.mst_volume_min(a, hip.F32, 1, 8, b, 0, None) != 0
    assert lib.mst_volume_min(a, hip.F32, 1, 8, None, 1, None) != 0 and "volume_min" in hip.last_error()
    assert lib.mst_crop_or_pad_at(a, 4, 4, 0, b, 2, 6, 4, 0, 0, 0, 0, 0, 0, 0, 0.0, p, 4 * 96, None) != 0
    assert lib.mst_crop_or_pad_at(None, 4, 4, 4, b, 2, 6, 4, 0, 0, 0, 0, 0, 0, 0, 0.0, p, 4 * 96, None) != 0 and "crop_or_pad_at" in hip.last_error()


def test_host_tensors_are_refused_with_the_no_cpu_path_wording():
    x = torch.zeros(1, 1, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        TrainAugment(flip=True)(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        TrainAugment()(x)                                   # also with every flag off
    with pytest.raises(RuntimeError, match="no CPU path"):
        preprocess.crop_or_pad(x[0], (2, 2, 2), random_center=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        preprocess.crop_or_pad(x[0], (2, 2, 2))
    with pytest.raises(ValueError, match="no CPU path"):
        hip.augment_volumes(x[0], torch.zeros(1, 8))
    with pytest.raises(ValueError, match="no CPU path"):
        hip.volume_min(x[0])
    with pytest.raises(ValueError):
        TrainAugment(flip=True)(torch.zeros(1, 2, 2, 4, 4))  # one channel
    with pytest.raises(TypeError):
        TrainAugment(out_dtype=torch.float64)


def test_draw_distributions_follow_the_reference():
    aug = TrainAugment(flip=True, random_rotate=True, noise=True, generator=torch.Generator().manual_seed(7))
    p = aug.draw(N_DRAWS)
    flips = p["flip"].double().mean(dim=0)
    for axis in range(3):
        assert abs(float(flips[axis]) - 0.5) < 0.04, (axis, float(flips[axis]))
    # the axes are drawn independently: the frequency of "D and H both flipped" is 0.25 +- 5 sqrt(0.1875 / N) = 0.035
    both = float((p["flip"][:, 0] & p["flip"][:, 1]).double().mean())
    assert abs(both - 0.25) < 0.035, both
    neg = float((p["sign"] < 0).double().mean())
    assert abs(neg - 0.5) < 0.04, neg
    assert set(p["sign"].tolist()) == {-1.0, 1.0}
    th = p["theta_deg"]
    assert 0.0 <= float(th.min()) and float(th.max()) <= 90.0
    assert abs(float(th.mean()) - 45.0) < 2.1, float(th.mean())
    sd = p["noise_std"]
    assert 0.0 <= float(sd.min()) and float(sd.max()) <= 0.25
    assert abs(float(sd.mean()) - 0.125) < 0.006, float(sd.mean())


def test_flags_off_draw_neutral_values_and_records_follow_the_draws():
    p = TrainAugment().draw(5)
    assert not p["flip"].any() and bool((p["sign"] == 1).all()) and not p["theta_deg"].any() and not p["noise_std"].any()
    rec = TrainAugment.record(p)
    assert rec.shape == (5, 8) and rec.dtype == torch.float32
    assert torch.equal(rec, R.records(5))                   # cos = 1, sin = 0, sign = 1, everything else 0: the identity record
    aug = TrainAugment(flip=True, random_rotate=True, noise=True, degrees=(10.0, 20.0), noise_std=(0.1, 0.2),
                       generator=torch.Generator().manual_seed(3))
    p = aug.draw(6)
    rec = TrainAugment.record(p)
    assert float(p["theta_deg"].min()) >= 10.0 and float(p["theta_deg"].max()) <= 20.0
    assert float(p["noise_std"].min()) >= 0.1 and float(p["noise_std"].max()) <= 0.2
    assert torch.allclose(rec[:, hip.AUG_COS].double(), torch.cos(torch.deg2rad(p["theta_deg"])), atol=1e-7)
    assert torch.allclose(rec[:, hip.AUG_SIN].double(), torch.sin(torch.deg2rad(p["theta_deg"])), atol=1e-7)
    assert torch.equal(rec[:, hip.AUG_SIGN].double(), p["sign"]) and torch.equal(rec[:, hip.AUG_FLIP_D:] != 0, p["flip"])
    assert torch.equal(rec[:, hip.AUG_STD], p["noise_std"].float()) and not rec[:, hip.AUG_FILL].any()
    assert (hip.AUG_COS, hip.AUG_SIN, hip.AUG_FILL, hip.AUG_SIGN, hip.AUG_STD, hip.AUG_FLIP_D, hip.AUG_FLIP_H, hip.AUG_FLIP_W) == \
           (R.COS, R.SIN, R.FILL, R.SIGN, R.STD, R.FLIP_D, R.FLIP_H, R.FLIP_W)


def test_same_seed_gives_the_same_draws():
    def draws(seed):
        aug = TrainAugment(flip=True, random_rotate=True, noise=True, generator=torch.Generator().manual_seed(seed))
        return [aug.draw(3) for _ in range(2)]
    a, b, c = draws(11), draws(11), draws(12)
    for pa, pb in zip(a, b):
        assert all(torch.equal(pa[k], pb[k]) for k in pa)
    assert not torch.equal(a[0]["theta_deg"], a[1]["theta_deg"])          # successive batches differ
    assert not torch.equal(a[0]["theta_deg"], c[0]["theta_deg"])
    ca, cb = (preprocess.draw_crop_offsets((9, 4, 7), (5, 8, 7), torch.Generator().manual_seed(5)) for _ in range(2))
    assert ca == cb


def test_random_crop_offsets_stay_in_range_and_hit_both_ends():
    g = torch.Generator().manual_seed(0)
    src, tgt = (9, 4, 7), (5, 8, 7)                                       # axis 0 cropped by 4, axis 1 padded by 4, axis 2 untouched
    seen_crop, seen_pad = set(), set()
    for _ in range(200):                                                  # an end is missed with probability (4/5)^200 < 1e-19
        crop, pad = preprocess.draw_crop_offsets(src, tgt, g)
        assert 0 <= crop[0] <= 4 and crop[1] == 0 and crop[2] == 0, crop
        assert pad[0] == 0 and 0 <= pad[1] <= 4 and pad[2] == 0, pad
        seen_crop.add(crop[0])
        seen_pad.add(pad[1])
    assert seen_crop == set(range(5)) and seen_pad == set(range(5))


def test_restatement_generator_is_philox4x32_10():
    """The known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10 rounds): zeros, all ones, digits of pi."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        got = R.philox4x32_10(*(np.array([c]) for c in ctr), *key)
        assert tuple(int(w[0]) for w in got) == want
    z = R.normals(5, 9, 2, 10)                                            # voxels 8, 9 are the first half of group 2; volume v uses counter 9 + v
    assert z.shape == (2, 10) and torch.equal(R.normals(5, 10, 1, 10)[0], z[1]) and not torch.equal(z[0], z[1])


def test_restatement_is_the_identity_and_a_flip_where_it_must_be():
    x = R.volumes((2, 3, 5, 7))
    out, _ = R.augment(x, R.records(2), torch.float32)
    assert torch.equal(out, x)
    out, _ = R.augment(x, R.records(2, flips=[(1, 0, 1), (0, 1, 0)], sign=[-1.0, 1.0]), torch.float32)
    assert torch.equal(out[0], -x[0].flip(0, 2)) and torch.equal(out[1], x[1].flip(1))
    sq = R.volumes(R.SQUARE)
    out, _ = R.augment(sq, R.records(2, 90.0))
    assert float((out - torch.rot90(sq.double(), -1, (2, 3))).abs().max()) < 1e-12     # the sense the definition gives: k = -1


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("degrees", R.ROTATION_DEGREES)
def test_rotation_parity_leaves_out_at_most_two_percent(shape, degrees):
    """The GPU rotation test compares only voxels whose float64 sample position is at least 1e-3 from the inside / outside boundary; for
    its own inputs that band holds at most 2 % of the voxels (the restatement alone decides), and both sides of the boundary are present."""
    x, rec = R.rotation_case(shape, degrees)
    out, band = R.augment(x, rec)
    frac = float((band < R.BAND).double().mean())
    print(f"shape {shape} theta {degrees}: {frac:.4%} of the voxels within {R.BAND} of the boundary")
    assert frac <= 0.02, frac
    n, D, H, W = shape
    for v in range(n):
        _, s_h, s_w = R.source_positions(rec[v], D, H, W)
        inside = (s_h >= -0.5) & (s_h < H - 0.5) & (s_w >= -0.5) & (s_w < W - 0.5)
        assert bool(inside.any()) and bool((~inside).any())
        assert torch.equal(out[v][:, ~inside], rec[v, R.FILL].double().expand(D, int((~inside).sum())))
