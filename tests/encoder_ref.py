"""CPU restatement of the encoder API -- DinoVisionTransformer.forward / forward_features / get_intermediate_layers
(extern/dinov2/vision_transformer.py:213-329) -- composed from the oracle's own pieces: interpolate_pos_encoding, vit_block (through
swiglu_ref.block, which is vit_block for the GELU MLP and swaps the FFN for SwiGLU blocks), layer_norm.  Its own part is the patch
embedding of a true RGB image, F.conv2d with the full three-channel kernel (patch_embed.py:65,75-81).  A helper module, not a test:
dtype-generic (the GPU tests run it in float64), nothing under oracle/ changes.  tests/test_encoder_api_cpu.py pins it against the
reference's own DinoVisionTransformer (tests/golden/encoder_api.npz)."""
import torch
import torch.nn.functional as F

import swiglu_ref
from oracle import mst_oracle as O

PATCH = O.PATCH


def tokens(sd, x):
    """prepare_tokens_with_masks (vision_transformer.py:213-232, no masks) on x [n, 3, H, W] (or [n, 1, H, W]: the grey image
    repeated over the channels, dino.py:125-127) -> [n, N, E]."""
    if x.shape[1] == 1:
        x = x.repeat(1, 3, 1, 1)
    n, _, H, W = x.shape
    assert H % PATCH == 0, f"Input image height {H} is not a multiple of patch height {PATCH}"
    assert W % PATCH == 0, f"Input image width {W} is not a multiple of patch width: {PATCH}"
    t = F.conv2d(x, sd["encoder.patch_embed.proj.weight"], sd["encoder.patch_embed.proj.bias"], stride=PATCH).flatten(2).transpose(1, 2)
    t = torch.cat((sd["encoder.cls_token"].expand(n, -1, -1), t), dim=1)
    reg = sd.get("encoder.register_tokens")
    # register encoders are the hub's *_reg models: anti-aliased, size-based resampling (see O.prepare_tokens)
    t = t + O.interpolate_pos_encoding(sd["encoder.pos_embed"], t.shape[1] - 1, H, W, offset=0.0 if reg is not None else 0.1,
                                       antialias=reg is not None)
    if reg is not None:
        t = torch.cat((t[:, :1], reg.expand(n, -1, -1), t[:, 1:]), dim=1)
    return t


class Restated:
    """Every block's residual stream of one input, and the three API results read off it."""

    def __init__(self, sd, x, depth, heads, dtype=torch.float64):
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        self.sd, self.shape = sd, tuple(x.shape)
        self.R = sd["encoder.register_tokens"].shape[1] if "encoder.register_tokens" in sd else 0
        t = tokens(sd, x.to(dtype))
        self.streams = []
        for i in range(depth):
            t, _ = swiglu_ref.block(t, sd, O._block_prefix(sd, i), heads)
            self.streams.append(t)

    def norm(self, t):
        return O.layer_norm(t, self.sd["encoder.norm.weight"], self.sd["encoder.norm.bias"], 1e-6)

    def forward_features(self):
        x, R = self.streams[-1], self.R
        xn = self.norm(x)
        return {"x_norm_clstoken": xn[:, 0], "x_norm_regtokens": xn[:, 1:R + 1], "x_norm_patchtokens": xn[:, R + 1:], "x_prenorm": x,
                "masks": None}

    def forward(self):
        return self.forward_features()["x_norm_clstoken"]

    def get_intermediate_layers(self, n=1, reshape=False, return_class_token=False, norm=True):
        total = len(self.streams)
        take = range(total - n, total) if isinstance(n, int) else n
        outs = [self.streams[i] for i in range(total) if i in take]
        assert len(outs) == len(take), f"only {len(outs)} / {len(take)} blocks found"
        if norm:
            outs = [self.norm(o) for o in outs]
        cls = [o[:, 0] for o in outs]
        outs = [o[:, 1 + self.R:] for o in outs]
        if reshape:
            B, _, H, W = self.shape
            outs = [o.reshape(B, H // PATCH, W // PATCH, -1).permute(0, 3, 1, 2).contiguous() for o in outs]
        return tuple(zip(outs, cls)) if return_class_token else tuple(outs)


def rgb_image(shape, seed):
    """[n, 3, H, W] with three different channels: three synthetic volumes' slices, one per channel (z-normalised like the data)."""
    from mst import synth
    n, c, H, W = shape
    return torch.cat([synth.synth_volume((1, 1, n, H, W), seed + 17 * ch)[0, 0][:, None] for ch in range(c)], dim=1).contiguous()


def worst_row(got, ref):
    """Worst per-token-row rel-L2 over the last dim: a whole-tensor norm hides one misplaced or stale row."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(((got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)).max())
