"""Device-side training augmentation: what the reference's datasets do to a training volume behind CropOrPad and
ZNormalization, on CPU workers and one volume at a time (mst/data/datasets/dataset_3d_duke.py:44-47; the same lines in dataset_3d_lidc.py
and dataset_3d_mrnet.py) --

    tio.RandomAffine(scales=0, degrees=(0, 0, 0, 0, 0, 90), translation=0, default_pad_value='minimum')   if random_rotate
    tio.RandomFlip((0, 1, 2))                                                                            if flip
    tio.Lambda(lambda x: -x if torch.rand((1,))[0] < 0.5 else x)                                         if noise
    tio.RandomNoise(std=(0.0, 0.25))                                                                     if noise

-- for a whole batch already in device memory, as one HIP gather kernel (mst_augment_volumes, csrc/k_augment.hip) behind one small
reduction for the 'minimum' fill (mst_volume_min).  The random parameters are drawn on the host, per volume, from a torch.Generator; the
voxel noise comes from a counter-based generator inside the kernel.

Not pinned against torchio (it and SimpleITK are not installed where this was built): the rotation's sense, its centre ((H-1)/2, (W-1)/2)
and its edge rule (bilinear, inside iff the sample lies within half a voxel of the grid, else the volume's minimum) are the definition in
include/mst_hip.h, tested against a float64 restatement of that definition (tests/augment_ref.py)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from . import hip


class TrainAugment:
    """TrainAugment(flip, random_rotate, noise)(batch): the flags of the reference datasets' constructors.  batch [B, 1, D, H, W] on a HIP
    device (fp32 / fp16 / bf16) -> the same shape in out_dtype (the batch's own by default).  Per volume and call:

        flip            each of the axes D, H, W reversed with p = 0.5, independently
        random_rotate   in-plane rotation by t uniform in `degrees`, the same for every slice; outside voxels take the volume's minimum
        noise           sign inversion with p = 0.5, then + std N(0,1) per voxel with std uniform in `noise_std`

    in the reference's order: rotate, flip, sign, noise.  The draws come from `generator` (a CPU torch.Generator; torch's default one when
    None) and the last call's are kept in `last_params`; the voxel noise is keyed by a 64-bit seed drawn from the generator at the first
    call that needs one and by a volume counter that advances by B per call, so successive batches differ and a run is reproducible from
    the generator's seed.  All flags off is the identity: the batch itself is returned and nothing is launched -- unless out_dtype asks for
    another type than the batch's: then the kernel runs with identity records, as a converter (the batch rounded once to out_dtype)."""

    def __init__(self, flip: bool = False, random_rotate: bool = False, noise: bool = False, noise_std: Tuple[float, float] = (0.0, 0.25),
                 degrees: Tuple[float, float] = (0.0, 90.0), out_dtype: Optional[torch.dtype] = None,
                 generator: Optional[torch.Generator] = None):
        self.flip, self.random_rotate, self.noise = bool(flip), bool(random_rotate), bool(noise)
        self.noise_std = (float(noise_std[0]), float(noise_std[1]))
        self.degrees = (float(degrees[0]), float(degrees[1]))
        if out_dtype is not None and out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"TrainAugment: out_dtype {out_dtype} (float32, float16, bfloat16)")
        self.out_dtype = out_dtype
        self.generator = generator
        self.seed: Optional[int] = None
        self.counter = 0                                    # volumes noised so far: the counter of the next call's volume 0
        self.last_params: Optional[Dict[str, object]] = None

    def _uniform(self, n: int, lo: float, hi: float) -> torch.Tensor:
        return lo + (hi - lo) * torch.rand(n, dtype=torch.float64, generator=self.generator)

    def draw(self, B: int) -> Dict[str, torch.Tensor]:
        """The per-volume parameters of one batch (host tensors): theta_deg [B] fp64, flip [B, 3] bool (axes D, H, W), sign [B] fp64 (+-1),
        noise_std [B] fp64.  A transform whose flag is off draws nothing and gets its neutral value."""
        theta = self._uniform(B, *self.degrees) if self.random_rotate else torch.zeros(B, dtype=torch.float64)
        flips = torch.rand(B, 3, generator=self.generator) < 0.5 if self.flip else torch.zeros(B, 3, dtype=torch.bool)
        if self.noise:
            sign = 1.0 - 2.0 * (torch.rand(B, generator=self.generator) < 0.5).double()           # -x if rand < 0.5 else x
            std = self._uniform(B, *self.noise_std)
        else:
            sign, std = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
        return {"theta_deg": theta, "flip": flips, "sign": sign, "noise_std": std}

    @staticmethod
    def record(p: Dict[str, torch.Tensor]) -> torch.Tensor:
        """The [B, 8] fp32 records of mst_augment_volumes for draw()'s parameters (host tensor; the fill column is left 0).  No rotation
        is cos = 1, sin = 0 exactly: the kernel then copies voxels."""
        B = p["theta_deg"].numel()
        rec = torch.zeros(B, hip.AUG_REC, dtype=torch.float32)
        for b, deg in enumerate(p["theta_deg"].tolist()):
            rec[b, hip.AUG_COS], rec[b, hip.AUG_SIN] = (1.0, 0.0) if deg == 0.0 else (math.cos(math.radians(deg)), math.sin(math.radians(deg)))
        rec[:, hip.AUG_SIGN] = p["sign"].float()
        rec[:, hip.AUG_STD] = p["noise_std"].float()
        rec[:, hip.AUG_FLIP_D:hip.AUG_FLIP_W + 1] = p["flip"].float()
        return rec

    def __call__(self, batch: torch.Tensor) -> torch.Tensor:
        if not isinstance(batch, torch.Tensor) or batch.dim() != 5 or batch.shape[1] != 1:
            raise ValueError("TrainAugment expects [B, 1, D, H, W]")
        if not batch.is_cuda:
            raise RuntimeError("TrainAugment: tensor must live on a HIP device; there is no CPU path")
        out_dtype = self.out_dtype or batch.dtype
        if not (self.flip or self.random_rotate or self.noise) and out_dtype == batch.dtype:
            self.last_params = None
            return batch
        B, _, D, H, W = batch.shape
        x = batch.contiguous().view(B, D, H, W)
        p = self.draw(B)
        rec = self.record(p).to(batch.device, non_blocking=True)
        if self.random_rotate:
            hip.volume_min(x, out=rec, column=hip.AUG_FILL)             # default_pad_value='minimum'
        if self.noise and self.seed is None:
            self.seed = int(torch.randint(0, 2 ** 62, (1,), generator=self.generator))
        seed, counter = self.seed or 0, self.counter
        out = hip.augment_volumes(x, rec, seed, counter, out_dtype)
        if self.noise:
            self.counter += B
        self.last_params = {**p, "record": rec, "seed": seed, "counter": counter}
        return out.view(batch.shape)
