"""CPU restatement of the training augmentation as include/mst_hip.h defines it (mst_augment_volumes, mst_crop_or_pad_at): plain torch /
numpy, float64 or float32, taking the kernel's parameter records.  A helper module, not a test.

    augment(x, records, dtype)           rotate -> flip -> sign of x [n, D, H, W] per its record, WITHOUT the noise
    source_positions(...)                the float64 sample positions, and how far each lies from the inside / outside boundary
    philox4x32_10, normals(...)          the kernel's counter-based N(0, 1): Philox4x32-10 + Box-Muller, per (seed, counter, voxel)
    crop_or_pad_at(x, target, crop, pad) numpy.pad + slicing with explicit begin offsets

The rotation's sense, centre and edge rule are this build's definition, restated here; nothing here is torchio."""
import math

import numpy as np
import torch

COS, SIN, FILL, SIGN, STD, FLIP_D, FLIP_H, FLIP_W = range(8)

SHAPES = ((2, 3, 5, 7), (1, 2, 14, 28), (2, 4, 28, 28))      # [n, D, H, W]: odd sizes, W % 4 != 0; W % 4 == 0; square, several volumes
SQUARE = (2, 4, 28, 28)
ROTATION_DEGREES = (30.0, 77.3)
BAND = 1e-3                                                  # voxels this close to the inside / outside boundary are left out of rotation parity


def volumes(shape, seed=0):
    """The test volumes: standard normal fp32 [n, D, H, W] from a seeded generator (the same on every machine)."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 + seed))


def records(n, theta_deg=0.0, flips=(0, 0, 0), sign=1.0, std=0.0, fill=0.0):
    """[n, 8] fp32 records; every argument a scalar (all volumes alike) or a sequence of n.  theta 0 is cos = 1, sin = 0 exactly."""
    at = lambda a, v: float(a[v]) if isinstance(a, (list, tuple, torch.Tensor)) else float(a)
    rec = torch.zeros(n, 8, dtype=torch.float32)
    for v in range(n):
        t = at(theta_deg, v)
        rec[v, COS], rec[v, SIN] = (1.0, 0.0) if t == 0.0 else (math.cos(math.radians(t)), math.sin(math.radians(t)))
        f = flips[v] if isinstance(flips[0], (list, tuple)) else flips
        rec[v, FLIP_D], rec[v, FLIP_H], rec[v, FLIP_W] = (float(bool(a)) for a in f)
        rec[v, SIGN], rec[v, STD], rec[v, FILL] = at(sign, v), at(std, v), at(fill, v)
    return rec


def rotation_case(shape, degrees, seed=0):
    """The inputs of the rotation parity test: (x, records) -- every volume rotated by `degrees`, filled with its own minimum, odd volumes
    also flipped along D and H."""
    x = volumes(shape, seed)
    n = shape[0]
    rec = records(n, degrees, [(v % 2, v % 2, 0) for v in range(n)], fill=x.reshape(n, -1).min(dim=1).values)
    return x, rec


def source_positions(rec, D, H, W, dtype=torch.float64):
    """For one record: (d' [D], s_h [H, W], s_w [H, W]) -- where output voxel (d, h, w) samples the input -- in `dtype`, from the record's
    values cast to it, each product and sum rounded on its own in the order of the definition."""
    r = rec.to(dtype)
    d = torch.arange(D)
    h = torch.arange(H, dtype=dtype)[:, None].expand(H, W)
    w = torch.arange(W, dtype=dtype)[None, :].expand(H, W)
    if rec[FLIP_D] != 0:
        d = D - 1 - d
    if rec[FLIP_H] != 0:
        h = H - 1 - h
    if rec[FLIP_W] != 0:
        w = W - 1 - w
    ch, cw = (H - 1) / 2, (W - 1) / 2
    y, x = h - ch, w - cw
    s_h = ch + r[COS] * y - r[SIN] * x
    s_w = cw + r[SIN] * y + r[COS] * x
    return d, s_h, s_w


def boundary_distance(s_h, s_w, H, W):
    """Distance of every sample position from the nearest inside / outside decision boundary (s_h = -0.5, H - 0.5; s_w = -0.5, W - 0.5)."""
    return torch.minimum(torch.minimum((s_h + 0.5).abs(), (s_h - (H - 0.5)).abs()), torch.minimum((s_w + 0.5).abs(), (s_w - (W - 0.5)).abs()))


def augment(x, records, dtype=torch.float64):
    """x [n, D, H, W] (any float type; cast to `dtype`), records [n, 8] -> (out [n, D, H, W] in `dtype`, band [n, H, W] fp64: the float64
    boundary distance of every in-plane position, for the caller's exclusion band).  Noise is not added."""
    n, D, H, W = x.shape
    xs = x.detach().cpu().to(dtype)
    records = records.detach().cpu().float()
    out = torch.empty((n, D, H, W), dtype=dtype)
    band = torch.empty((n, H, W), dtype=torch.float64)
    for v in range(n):
        rec = records[v]
        d, s_h, s_w = source_positions(rec, D, H, W, dtype)
        _, e_h, e_w = source_positions(rec, D, H, W, torch.float64)
        band[v] = boundary_distance(e_h, e_w, H, W)
        inside = (s_h >= -0.5) & (s_h < H - 0.5) & (s_w >= -0.5) & (s_w < W - 0.5)
        fh, fw = torch.floor(s_h), torch.floor(s_w)
        th, tw = s_h - fh, s_w - fw
        h0, w0 = fh.long(), fw.long()
        ha, hb = h0.clamp(0, H - 1), (h0 + 1).clamp(0, H - 1)
        wa, wb = w0.clamp(0, W - 1), (w0 + 1).clamp(0, W - 1)
        vol = xs[v][d]                                                   # [D, H, W], the slice axis flipped
        v00, v01, v10, v11 = vol[:, ha, wa], vol[:, ha, wb], vol[:, hb, wa], vol[:, hb, wb]
        top = v00 + tw * (v01 - v00)
        bot = v10 + tw * (v11 - v10)
        val = top + th * (bot - top)
        val = torch.where(inside, val, rec[FILL].to(dtype))
        out[v] = val * rec[SIGN].to(dtype)
    return out, band


_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) on arrays of 32-bit words held
    in uint64 -> the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LO for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & _LO, np.uint64(k1) & _LO
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                                       # < 2^64: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def normals(seed, counter, n, elems):
    """The kernel's N(0, 1) for n volumes of `elems` voxels: float64 [n, elems].  Voxel i of volume v takes word i % 4 of the block with
    key = seed, counter words (i // 4, 0, c_lo, c_hi), c = counter + v;  u = ((word >> 9) + 0.5) / 2^23;  words (0, 1) and (2, 3) make
    z = sqrt(-2 ln u_a) (cos, sin)(2 pi u_b)."""
    groups = (elems + 3) // 4
    out = np.empty((n, groups * 4), dtype=np.float64)
    g = np.arange(groups, dtype=np.uint64)
    zero = np.zeros(groups, dtype=np.uint64)
    mask = (1 << 64) - 1
    for v in range(n):
        c = (int(counter) + v) & mask
        w = philox4x32_10(g, zero, zero + np.uint64(c & 0xFFFFFFFF), zero + np.uint64(c >> 32), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        u = [((x >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0 for x in w]
        z = out[v].reshape(groups, 4)
        for a in (0, 2):
            r = np.sqrt(-2.0 * np.log(u[a]))
            z[:, a], z[:, a + 1] = r * np.cos(2.0 * np.pi * u[a + 1]), r * np.sin(2.0 * np.pi * u[a + 1])
    return torch.from_numpy(out[:, :elems].copy())


def crop_or_pad_at(x, target_shape, crop_begin, pad_begin, padding_mode=0):
    """CropOrPad with explicit begins (augmentations_3d.py:178-195 with the drawn ini / r): numpy.pad of every channel of x [C, a0, a1, a2]
    by (pad_begin, total - pad_begin) per axis ('minimum' or a constant), then the crop [crop_begin, crop_begin + target)."""
    a = x.detach().cpu().float().numpy()
    src = a.shape[1:]
    widths = [(0, 0)] + [(int(p), max(int(t) - int(s), 0) - int(p)) for s, t, p in zip(src, target_shape, pad_begin)]
    a = np.pad(a, widths, mode="minimum") if padding_mode == "minimum" else np.pad(a, widths, mode="constant", constant_values=float(padding_mode))
    sl = (slice(None),) + tuple(slice(int(c), int(c) + int(t)) for c, t in zip(crop_begin, target_shape))
    return torch.from_numpy(np.ascontiguousarray(a[sl]))
