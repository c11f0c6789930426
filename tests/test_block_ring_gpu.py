"""Weight-ring schedule of the single-role block kernel (``mst_block_fused_s``) on a real MI355X (``-m gpu``).

The kernel streams its weights through a six-slot LDS ring whose slots, LDS addresses and LDS-DMA destinations are constants
of the position inside a tile (a tile consumes 108 = 18 x 6 elements, so every tile starts at slot 0), with the MLP part rolled
over one ring period.  What such a schedule can get wrong is a function of the ring position at which a tile starts and of how
many tiles a workgroup owns: a slot read before it has landed, or overwritten before every wave has left it, shows in the second
or a later tile of a workgroup, or in its last one.  So the input rows and the attention rows are periodic with period 128: every
tile sees the same operands and must return the same bits as tile 0, and tile 0 must meet the fp64 bars of
``tests/test_hip_ops.py::test_block_fused_single_role`` (1.5e-2 (bf16) / 2.5e-3 (fp16) of max(|proj|, |mlp|) for ``x``, four times
that, absolute, for the normalised rows).  A stale ring slot cannot pass both by luck; the reference alone passes trivially.

Row counts for the 256-workgroup persistent grid of MI355X: one tile; 257 tiles (two on one workgroup); 4 x 256 + 3 tiles (four
and five per workgroup).
"""
import math

import pytest
import torch

from mst import synth

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TOL = {"bf16": 1.5e-2, "fp16": 2.5e-3}
E, HID, TILE = 384, 1536, 128
ROWS = [TILE, TILE * 257, TILE * (4 * 256 + 3)]


@pytest.fixture(scope="module")
def hip():
    from mst import hip as h
    h.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return h


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(synth.hash_normal(tuple(shape), seed, 77)) * scale


@pytest.fixture(scope="module")
def weights():
    wp, bp = rnd((E, E), 62) / math.sqrt(E), rnd((E,), 63) * 0.1
    w1, b1 = rnd((HID, E), 51) / math.sqrt(E), rnd((HID,), 52) * 0.1
    w2, b2 = rnd((E, HID), 53) / math.sqrt(HID), rnd((E,), 54) * 0.1
    g, be = rnd((E,), 55) * 0.2 + 1, rnd((E,), 56) * 0.2
    return wp, bp, w1, b1, w2, b2, g, be


_ref = {}                                   # per dtype: one tile of operands, its fp64 reference, the packed weights


def tile_case(hip, dt, weights):
    """One tile of x and attention rows, the fp64 block arithmetic on them (attention.py:67-68; block.py:89-94,112-113;
    mlp.py:34-40) and the packed weight stream; computed once per dtype and left unchanged."""
    if dt not in _ref:
        x = rnd((TILE, E), 60, 1.5) + 0.3
        att = rnd((TILE, E), 61, 1.0).to(DT[dt])
        wp, bp, w1, b1, w2, b2, g, be = (w.double() for w in weights)
        proj = att.double() @ wp.t() + bp
        xmid = x.double() + proj
        h = torch.nn.functional.layer_norm(xmid, (E,), g, be, 1e-6)
        h = h @ w1.t() + b1
        h = 0.5 * h * (1 + torch.erf(h / math.sqrt(2)))
        y = h @ w2.t() + b2
        ref = xmid + y
        refn = torch.nn.functional.layer_norm(ref, (E,))
        scale = max(float(y.abs().max()), float(proj.abs().max()))
        packed = hip.pack_block_seq(*(w.cuda() for w in weights[:2]), None, *(w.cuda() for w in weights[2:]), None, DT[dt])
        _ref[dt] = (x.cuda(), att.cuda(), ref, refn, scale, packed)
    return _ref[dt]


@pytest.mark.parametrize("with_xn", [False, True])
@pytest.mark.parametrize("layout", [0, 7])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_block_ring(hip, weights, dt, M, layout, with_xn):
    x1, a1, ref, refn, scale, (seq, b1f, pbf, b2f) = tile_case(hip, dt, weights)
    ntiles = M // TILE
    if layout:                               # a 32-row group is one block of either layout: permute the tile, then repeat it
        xb, ab = hip.to_image32(x1).repeat(ntiles, 1), hip.to_blocked16(a1).repeat(ntiles, 1)
    else:
        xb, ab = x1.repeat(ntiles, 1), a1.repeat(ntiles, 1)
    xn = torch.zeros(M, E, dtype=DT[dt], device="cuda") if with_xn else None

    hip.block_fused_s(xb, ab, seq, b1f, pbf, b2f, xn, layout=layout)
    torch.cuda.synchronize()

    # every tile against tile 0, bit for bit (whole tiles, so the comparison needs no change of layout)
    tiles = xb.view(ntiles, TILE * E)
    bad = (tiles != tiles[0]).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"x: tiles {bad[:8]} (of {len(bad)}) differ from tile 0"
    if with_xn:
        ntile = xn.view(ntiles, TILE * E)
        bad = (ntile != ntile[0]).any(dim=1).nonzero().flatten().tolist()
        assert not bad, f"xn: tiles {bad[:8]} (of {len(bad)}) differ from tile 0"

    # tile 0 against fp64
    got_x = hip.from_image32(xb[:TILE]) if layout else xb[:TILE]
    err_x = float((got_x.double().cpu() - ref).abs().max() / scale)
    print(f"{dt} M={M} layout={layout} xn={with_xn}: x error {err_x:.3e} of scale (bar {TOL[dt]:g})")
    assert err_x < TOL[dt]
    if with_xn:
        got_n = hip.from_blocked16(xn[:TILE]) if layout else xn[:TILE]
        err_n = float((got_n.double().cpu() - refn).abs().max())
        print(f"{dt} M={M} layout={layout} xn={with_xn}: xn error {err_n:.3e} (bar {4 * TOL[dt]:g})")
        assert err_n < 4 * TOL[dt]
