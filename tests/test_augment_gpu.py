"""Device-side training augmentation on the GPU: mst_augment_volumes / mst_volume_min / mst_crop_or_pad_at and their host layer
(mst/augment.py, mst/preprocess.py) against the restatement of tests/augment_ref.py.

Exact checks (bit-equal): the identity record, the eight flip combinations, sign -1, the fill, a 16-bit output against the rounded fp32
output, noise_std 0, the same (seed, counter) twice, crop_or_pad against numpy.pad.

Rotation parity (30 and 77.3 degrees, and the TrainAugment batch): against the float64 restatement, outside the 1e-3 boundary band that
tests/test_augment_cpu.py caps at 2 % of the voxels.  The bar is the project's stand-in method (tests/test_slice_stage_gpu.py): the same
restatement run in float32 on the CPU against its float64 run on the same inputs, times ten, computed by the test for its own inputs.
Stand-in errors, bars and what the kernel gave on an MI355X (max abs, unit-variance volumes):

    shape            degrees   stand-in   bar = 10 x   MI355X
    (2, 3, 5, 7)     30        6.72e-07   6.72e-06     4.51e-07
    (2, 3, 5, 7)     77.3      1.18e-06   1.18e-05     1.24e-06
    (1, 2, 14, 28)   30        3.45e-06   3.45e-05     3.08e-06
    (1, 2, 14, 28)   77.3      3.91e-06   3.91e-05     2.41e-06
    (2, 4, 28, 28)   30        7.54e-06   7.54e-05     7.00e-06
    (2, 4, 28, 28)   77.3      6.53e-06   6.53e-05     5.09e-06
    TrainAugment batch (3, 4, 28, 20), two steps: stand-in 5.50e-06 / 5.02e-06, bar 5.67e-05 / 5.18e-05 (with the noise terms), MI355X 5.38e-06 / 4.24e-06

(The error is that of fp32 sample positions: an ulp of a coordinate near 27 is 1.9e-6, times a neighbour difference of a few units.)

Noise (zeros [2, 1, 8, 64, 64], std 0.25, n = 32768 per volume): every bound is 5 sigma of its estimator, derived and not measured --
    |mean| < 7e-3                  sigma = 0.25 / sqrt(n) = 1.38e-3
    variance within 4 % of 0.0625  relative sigma = sqrt(2 / n) = 7.8e-3
    lag-1 autocorrelation along W and the correlation between the two volumes < 0.03      sigma = 1 / sqrt(n) = 5.5e-3
and, beyond the issue's list, every deviate against the restatement's float64 Philox4x32-10 + Box-Muller.  NOISE_Z_BAR is that
comparison's bar on a unit deviate: 8 fp32 ulps at |z| = 5.8, the largest deviate u >= 2^-24 can give -- logf, sqrtf, sincospif and the
product each err by an ulp or two relative to z, the uniforms are exact; the kernel's final fused multiply-add rounds once more
(half an ulp of the result)."""
import itertools

import pytest
import torch

import augment_ref as R
from mst import hip, preprocess
from mst.augment import TrainAugment
from oracle import mst_oracle as O

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
NOISE_Z_BAR = 5.8 * 8 * ULP
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def run(x, rec, seed=0, counter=0, out_dtype=None):
    return hip.augment_volumes(x.cuda(), rec.cuda(), seed, counter, out_dtype)


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_identity_record_returns_the_input_bits(shape, dtype):
    x = R.volumes(shape).to(dtype)
    x.view(-1)[:4] = torch.tensor([0.0, -0.0, float("inf"), -1e-30], dtype=dtype)     # signed zero, an infinity and a tiny value survive a copy
    out = run(x, R.records(shape[0], fill=123.0))
    assert out.dtype == dtype and out.shape == x.shape
    assert torch.equal(bits(out), bits(x))


@pytest.mark.parametrize("shape", R.SHAPES)
def test_each_flip_combination_equals_torch_flip(shape):
    x = R.volumes(shape)
    for fd, fh, fw in itertools.product((0, 1), repeat=3):
        out = run(x, R.records(shape[0], flips=(fd, fh, fw)))
        dims = [a + 1 for a, f in enumerate((fd, fh, fw)) if f]
        assert torch.equal(bits(out), bits(x.flip(dims) if dims else x)), (fd, fh, fw)
    # volumes of one batch flipped differently
    if shape[0] == 2:
        out = run(x, R.records(2, flips=[(1, 0, 1), (0, 1, 0)])).cpu()
        assert torch.equal(out[0], x[0].flip(0, 2)) and torch.equal(out[1], x[1].flip(1))


@pytest.mark.parametrize("shape", R.SHAPES)
def test_sign_minus_one_negates(shape):
    x = R.volumes(shape)
    assert torch.equal(bits(run(x, R.records(shape[0], sign=-1.0))), bits(-x))
    out = run(x, R.records(shape[0], flips=(1, 1, 1), sign=-1.0))
    assert torch.equal(bits(out), bits(-x.flip(1, 2, 3)))


def test_ninety_degrees_on_the_square_shape_is_rot90():
    x = R.volumes(R.SQUARE)
    out = run(x, R.records(2, 90.0, fill=77.0)).cpu()
    want = torch.rot90(x, -1, (2, 3))                        # the sense the definition gives (tests/test_augment_cpu.py checks the restatement's)
    assert float((out - want).abs().max()) <= 1e-6
    assert not bool((out == 77.0).any())                     # a quarter turn of a square leaves nothing outside


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_volume_min_is_exact(dtype):
    # (3, 5, 33, 37): 6105 voxels per volume, three workgroups each, no 16-byte alignment of the later volumes; signs: mixed, all positive, all negative
    x = R.volumes((3, 5, 33, 37), 1)
    x[1] = x[1].abs() + 0.5
    x[2] = -x[2].abs() - 0.5
    x = x.to(dtype)
    got = hip.volume_min(x.cuda())
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), x.float().reshape(3, -1).min(dim=1).values)
    for shape in R.SHAPES + ((2, 8, 64, 64),):              # the last one takes the 16-byte loads
        y = R.volumes(shape, 2).to(dtype)
        rec = torch.full((shape[0], 8), -5.0).cuda()
        assert hip.volume_min(y.cuda(), out=rec, column=R.FILL) is rec
        want = torch.full((shape[0], 8), -5.0)
        want[:, R.FILL] = y.float().reshape(shape[0], -1).min(dim=1).values
        assert torch.equal(rec.cpu(), want)                  # the fill column written, its neighbours untouched


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_volume_min_with_workgroups_whose_minimum_is_negative_zero(dtype):
    """-0.0 has the bit pattern of INT_MIN: a workgroup whose 2048-voxel chunk holds only -0.0 (and zeros or positives) must not displace the
    negative minimum of another workgroup, whichever of them reaches the atomic last.  The case of a sign-inverted volume with a zero
    background: 16 chunks per volume, the -0.0 chunks first, last, in the middle, and everywhere but one."""
    chunk, chunks = 2048, 16
    x = torch.full((4, chunks * chunk), -0.0)
    x[0, 3 * chunk:] = -R.volumes((1, 1, 1, 13 * chunk), 7).abs().view(-1) - 0.25       # -0.0 chunks first
    x[1, :12 * chunk] = -R.volumes((1, 1, 1, 12 * chunk), 8).abs().view(-1) - 0.25      # -0.0 chunks last
    x[2, 7 * chunk:9 * chunk] = 1.5                                                     # positives and -0.0 around one negative voxel
    x[2, 5 * chunk + 77] = -3.0
    x[3, 9 * chunk + 5] = -0.5                                                          # every chunk but one is -0.0 only
    x = x.to(dtype)
    want = x.float().min(dim=1).values
    assert bool((want < 0).all())
    xc = x.view(4, 8, 64, 64).cuda()
    for _ in range(3):                                                                  # three launches: the arrival order is not ours to choose
        got = hip.volume_min(xc).cpu()
        assert torch.equal(got, want), (got, want)
    # all -0.0: the minimum is a zero
    z = torch.full((1, 2, 64, 64), -0.0).to(dtype).cuda()
    assert float(hip.volume_min(z)) == 0.0
    # and through TrainAugment: the fill of the inverted, rotated volume is its minimum, not 0
    aug = TrainAugment(random_rotate=True, generator=torch.Generator().manual_seed(2))
    aug(xc.view(4, 1, 8, 64, 64))
    assert torch.equal(aug.last_params["record"][:, R.FILL].cpu(), want)


def test_znormalize_extrema_with_negative_zero():
    """mst_znorm takes its extrema through the same integer atomics (atomic_min_f32 / atomic_max_f32): with -0.0 as the largest value and as most
    of the volume, the mask (x > min) & (x < max) must still be that of the true extrema."""
    x = torch.full((1, 4, 64, 64), -0.0)
    x[0, 1:3] = -R.volumes((1, 2, 64, 64), 9)[0].abs() - 0.5
    x[0, 0, 0, 0] = -40.0
    mask = (x > x.min()) & (x < x.max())
    got, st = preprocess.znormalize(x.cuda(), (0.5, 99.5), return_stats=True)
    assert st["count"] == int(mask.sum()) == 2 * 64 * 64
    assert float((got.cpu() - O.znormalize(x, (0.5, 99.5))).abs().max()) < 2e-5          # the bar of tests/test_hip_ops.py's znormalize test


@pytest.mark.parametrize("shape", R.SHAPES)
def test_fill_of_a_rotated_batch_is_the_volume_minimum(shape):
    n, D, H, W = shape
    x = R.volumes(shape, 3)
    aug = TrainAugment(random_rotate=True, degrees=(40.0, 50.0), generator=torch.Generator().manual_seed(1))
    out = aug(x.view(n, 1, D, H, W).cuda()).cpu().view(shape)
    rec = aug.last_params["record"].cpu()
    mins = x.reshape(n, -1).min(dim=1).values
    assert torch.equal(rec[:, R.FILL], mins)
    for v in range(n):
        _, s_h, s_w = R.source_positions(rec[v], D, H, W)
        band = R.boundary_distance(s_h, s_w, H, W)
        outside = ~((s_h >= -0.5) & (s_h < H - 0.5) & (s_w >= -0.5) & (s_w < W - 0.5)) & (band >= R.BAND)
        assert bool(outside.any())
        assert bool((out[v][:, outside] == mins[v]).all())   # exactly the minimum, in every slice


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_sixteen_bit_output_is_the_rounded_fp32_output(shape, name):
    x, rec = R.rotation_case(shape, 30.0)
    rec[:, R.STD], rec[:, R.SIGN] = 0.25, -1.0
    out32 = run(x, rec, seed=3, counter=1)
    out16 = run(x, rec, seed=3, counter=1, out_dtype=DT[name])
    assert out16.dtype == DT[name]
    assert torch.equal(bits(out16), bits(out32.to(DT[name])))
    # and from a 16-bit input: the same values as from that input widened to fp32
    x16 = x.to(DT[name])
    assert torch.equal(bits(run(x16, rec, seed=3, counter=1, out_dtype=torch.float32)), bits(run(x16.float(), rec, seed=3, counter=1)))


def _rotation_error(shape, degrees, x, rec, got):
    """(stand-in error, the kernel's error), both max abs against the float64 restatement outside the boundary band."""
    ref, band = R.augment(x, rec)
    ref32, _ = R.augment(x, rec, torch.float32)
    keep = (band >= R.BAND)[:, None].expand(ref.shape)
    assert float((~keep).double().mean()) <= 0.02
    return float((ref32.double() - ref)[keep].abs().max()), float((got.double().cpu() - ref)[keep].abs().max())


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("degrees", R.ROTATION_DEGREES)
def test_rotation_matches_the_float64_restatement(shape, degrees):
    x, rec = R.rotation_case(shape, degrees)
    stand_in, err = _rotation_error(shape, degrees, x, rec, run(x, rec))
    print(f"shape {shape} theta {degrees}: stand-in {stand_in:.3e}, bar {10 * stand_in:.3e}, kernel {err:.3e}")
    assert stand_in > 0.0
    assert err <= 10 * stand_in, (err, stand_in)


def test_bf16_input_is_accepted():
    x, rec = R.rotation_case(R.SHAPES[1], 30.0)
    x16 = x.to(torch.bfloat16)
    rec[:, R.FILL] = x16.float().reshape(x.shape[0], -1).min(dim=1).values
    out = run(x16, rec)
    assert out.dtype == torch.bfloat16
    ref, band = R.augment(x16, rec)
    keep = (band >= R.BAND)[:, None].expand(ref.shape)
    # bf16 (8 significant bits) rounds the fp32 result once: values below 8 are spaced 2^-5 at most, half of that is 8 * 2^-9; on top of it the
    # fp32 rotation error (below 1e-4: the bars of the rotation test)
    assert float(ref.abs().max()) < 8.0
    assert float((out.double().cpu() - ref)[keep].abs().max()) <= 8.0 * 2.0 ** -9 + 1e-4


@pytest.mark.parametrize("mode", ["minimum", 0.5])
@pytest.mark.parametrize("src,tgt", [((9, 4, 7), (5, 8, 7)), ((6, 10, 5), (9, 3, 8)), ((5, 6, 7), (9, 9, 9)), ((8, 9, 10), (3, 4, 5))])
def test_crop_or_pad_random_center(mode, src, tgt):
    x = R.volumes((2, *src), 4)
    for seed in range(3):
        crop, pad = preprocess.draw_crop_offsets(src, tgt, torch.Generator().manual_seed(seed))
        got = preprocess.crop_or_pad(x.cuda(), tgt, mode, random_center=True, generator=torch.Generator().manual_seed(seed))
        assert torch.equal(got.cpu(), R.crop_or_pad_at(x, tgt, crop, pad, mode)), (seed, crop, pad)
    # the flag off: the centre rule as before (the oracle's numpy.pad restatement), also through the new entry point's code path
    old = preprocess.crop_or_pad(x.cuda(), tgt, mode)
    assert torch.equal(old.cpu(), O.crop_or_pad(x, tgt, mode))
    centre = ([(max(s - t, 0) + 1) // 2 for s, t in zip(src, tgt)], [(max(t - s, 0) + 1) // 2 for s, t in zip(src, tgt)])
    assert torch.equal(old.cpu(), R.crop_or_pad_at(x, tgt, *centre, mode))


def test_crop_or_pad_at_refuses_offsets_out_of_range():
    x = torch.zeros(4, 4, 4, device="cuda")
    out = torch.zeros(2, 6, 4, device="cuda")
    ws = torch.zeros(4 * 6 * 4, device="cuda")
    lib = hip.load()
    # 4 -> 2 leaves an excess of 2 on axis 0, 4 -> 6 a pad of 2 on axis 1; an untouched or padded axis takes crop 0 only, and the reverse
    call = lambda crop, pad: lib.mst_crop_or_pad_at(hip.ptr(x), 4, 4, 4, hip.ptr(out), 2, 6, 4, *crop, *pad, 0, 0.0, hip.ptr(ws), ws.numel() * 4,
                                                    hip.stream_of(x))
    assert call((2, 0, 0), (0, 2, 0)) == 0 and call((0, 0, 0), (0, 0, 0)) == 0
    for crop, pad in (((3, 0, 0), (0, 0, 0)), ((-1, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 3, 0)), ((0, 0, 0), (0, -1, 0)), ((0, 1, 0), (0, 0, 0)),
                      ((0, 0, 0), (1, 0, 0)), ((0, 0, 1), (0, 0, 0)), ((0, 0, 0), (0, 0, 1))):
        assert call(crop, pad) != 0 and "crop_or_pad" in hip.last_error(), (crop, pad)
    # the workspace is checked too: a pad beside a crop needs the padded array
    assert lib.mst_crop_or_pad_at(hip.ptr(x), 4, 4, 4, hip.ptr(out), 2, 6, 4, 0, 0, 0, 0, 0, 0, 0, 0.0, hip.ptr(ws), 4 * 95, hip.stream_of(x)) != 0
    assert "workspace" in hip.last_error()


def test_entry_points_refuse_bad_types_and_counts_on_real_buffers():
    """The checks behind the null / shape check, with device buffers that a launch could use safely were a check ever lost."""
    lib = hip.load()
    n = 65536                                                    # one more volume than a grid's second dimension takes
    x = torch.zeros(n, 1, 1, 4, device="cuda")
    out = torch.empty_like(x)
    rec = R.records(1).repeat(n, 1).cuda()
    st = hip.stream_of(x)
    assert lib.mst_augment_volumes(hip.ptr(x), hip.F32, hip.ptr(out), hip.F32, n, 1, 1, 4, hip.ptr(rec), 0, 0, st) != 0 and "65535" in hip.last_error()
    assert lib.mst_augment_volumes(hip.ptr(x), hip.F32, hip.ptr(out), hip.F32, n - 1, 1, 1, 4, hip.ptr(rec), 0, 0, st) == 0
    assert torch.equal(out[:n - 1], x[:n - 1])
    for idt, odt in ((hip.F8E4M3, hip.F32), (hip.F32, hip.F8E4M3), (-1, hip.F32), (hip.F32, 7)):
        assert lib.mst_augment_volumes(hip.ptr(x), idt, hip.ptr(out), odt, 2, 1, 1, 4, hip.ptr(rec), 0, 0, st) != 0 and "dtype" in hip.last_error()
    mins = torch.zeros(n, device="cuda")
    assert lib.mst_volume_min(hip.ptr(x), hip.F32, n, 4, hip.ptr(mins), 1, st) != 0
    assert lib.mst_volume_min(hip.ptr(x), hip.F8E4M3, 2, 4, hip.ptr(mins), 1, st) != 0 and "dtype" in hip.last_error()
    with pytest.raises(TypeError):
        hip.augment_volumes(x.view(n, 1, 1, 4)[:2].double(), rec[:2])
    with pytest.raises(ValueError):
        hip.augment_volumes(x.view(n, 1, 1, 4)[:2], rec[:3])
    with pytest.raises(TypeError):
        hip.augment_volumes(x.view(n, 1, 1, 4)[:2], rec[:2], out_dtype=torch.float64)


def test_train_augment_batch_equals_the_restatement_on_last_params():
    shape = (3, 1, 4, 28, 20)
    x = R.volumes((3, 4, 28, 20), 5)
    aug = TrainAugment(flip=True, random_rotate=True, noise=True, generator=torch.Generator().manual_seed(21))
    for step in range(2):
        out = aug(x.view(shape).cuda())
        assert out.shape == shape and out.dtype == torch.float32
        p = aug.last_params
        rec = p["record"].cpu()
        assert p["counter"] == 3 * step and aug.counter == 3 * (step + 1) and p["seed"] == aug.seed
        assert torch.equal(rec, _with_fill(TrainAugment.record(p), x))
        ref, band = R.augment(x, rec)
        ref32, _ = R.augment(x, rec, torch.float32)
        z = R.normals(p["seed"], p["counter"], 3, x[0].numel()).view(x.shape)
        ref = ref + rec[:, R.STD].double().view(3, 1, 1, 1) * z
        keep = (band >= R.BAND)[:, None].expand(ref.shape)
        assert float(keep.double().mean()) > 0.95
        stand_in = float((ref32.double() + rec[:, R.STD].double().view(3, 1, 1, 1) * z - ref)[keep].abs().max())
        bar = 10 * stand_in + 0.25 * NOISE_Z_BAR + 0.5 * ULP * float(ref.abs().max())
        err = float((out.double().cpu().view(x.shape) - ref)[keep].abs().max())
        print(f"step {step}: stand-in {stand_in:.3e}, bar {bar:.3e}, kernel {err:.3e}")
        assert err <= bar, (err, bar)
        if step:
            assert not torch.equal(out, first)                # new draws and a new noise key
        first = out
    # the same generator seed reproduces the run; all flags off is the identity and returns the batch itself
    again = TrainAugment(flip=True, random_rotate=True, noise=True, generator=torch.Generator().manual_seed(21))
    again(x.view(shape).cuda())
    assert torch.equal(again(x.view(shape).cuda()), first)
    xb = x.view(shape).cuda()
    off = TrainAugment()
    assert off(xb) is xb and off.last_params is None
    half = TrainAugment(out_dtype=torch.float16)(xb)          # a type change alone: the kernel as a converter
    assert torch.equal(half, xb.half())


def _with_fill(rec, x):
    rec = rec.clone()
    rec[:, R.FILL] = x.reshape(x.shape[0], -1).min(dim=1).values
    return rec


def test_noise_statistics_and_keys():
    zeros = torch.zeros(2, 1, 8, 64, 64, device="cuda")
    n = 8 * 64 * 64
    rec = R.records(2, std=0.25).cuda()
    out = hip.augment_volumes(zeros.view(2, 8, 64, 64), rec, 1234, 5)
    v = out.double().cpu()
    for b in range(2):
        assert abs(float(v[b].mean())) < 7e-3
        assert abs(float(v[b].var()) / 0.0625 - 1.0) < 0.04
        c = v[b] - v[b].mean()
        assert abs(float((c[..., 1:] * c[..., :-1]).sum() / (c * c).sum())) < 0.03
    c0, c1 = v[0] - v[0].mean(), v[1] - v[1].mean()
    assert abs(float((c0 * c1).sum() / (c0.norm() * c1.norm()))) < 0.03
    # every deviate against the float64 restatement: the key is (seed, counter + volume, voxel / 4), whatever the launch looked like
    z = R.normals(1234, 5, 2, n).view(2, 8, 64, 64)
    assert float((v - 0.25 * z).abs().max()) <= 0.25 * NOISE_Z_BAR
    assert torch.equal(bits(hip.augment_volumes(zeros.view(2, 8, 64, 64), rec, 1234, 5)), bits(out))
    nxt = hip.augment_volumes(zeros.view(2, 8, 64, 64), rec, 1234, 6)
    assert not torch.equal(nxt[0], out[0])
    assert torch.equal(bits(nxt[0]), bits(out[1]))            # volume 1 at counter 5 is volume 0 at counter 6: no dependence on the batch
    assert not torch.equal(hip.augment_volumes(zeros.view(2, 8, 64, 64), rec, 1235, 5), out)
    # a 64-bit seed and counter are used in full
    big = hip.augment_volumes(zeros.view(2, 8, 64, 64), rec, (1 << 63) + 1234, (1 << 40) + 5).double().cpu()
    assert float((big - 0.25 * R.normals((1 << 63) + 1234, (1 << 40) + 5, 2, n).view(2, 8, 64, 64)).abs().max()) <= 0.25 * NOISE_Z_BAR
    # shapes whose voxel count is no multiple of 4: the last group is cut, the keys do not move
    x = R.volumes(R.SHAPES[0])
    got = run(x, R.records(2, std=0.25), 9, 0).double().cpu()
    assert float((got - x.double() - 0.25 * R.normals(9, 0, 2, 105).view(2, 3, 5, 7)).abs().max()) <= 0.25 * NOISE_Z_BAR + 0.5 * ULP * 8


def test_noise_std_zero_leaves_the_input_bits():
    x = R.volumes((2, 8, 64, 64), 6)
    x[0, 0, 0, :2] = torch.tensor([-0.0, 0.0])
    assert torch.equal(bits(run(x, R.records(2, std=0.0), 77, 3)), bits(x))
    # one volume noised, the other not
    out = run(x, R.records(2, std=[0.0, 0.1]), 77, 3).cpu()
    assert torch.equal(bits(out[0]), bits(x[0])) and not torch.equal(out[1], x[1])
