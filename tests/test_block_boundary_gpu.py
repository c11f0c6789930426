"""Tile boundaries of the single-role block kernel (``mst_block_fused_s``) on a real MI355X (``-m gpu``).

The kernel stores a finished tile's rows, and fetches the next tile's, from inside the next tile's out-projection phases; only
one accumulator pair and the attention rows move between two tiles, and the last tile of a workgroup drains behind the loop.
What that schedule can get wrong is a function of how many tiles a workgroup owns and of where the rows end, so the row counts
below are written for the 256-workgroup persistent grid of MI355X: a single partial group; fewer tiles than workgroups; exactly
one tile per workgroup; uneven tile counts (some workgroups drain one tile earlier); a ragged last 32-row group.

Reference and bars are those of ``tests/test_hip_ops.py::test_block_fused_single_role``: the block arithmetic in fp64 on the same
(already rounded) operands, 1.5e-2 (bf16) / 2.5e-3 (fp16) of max(|proj|, |mlp|) for ``x`` and four times that, absolute, for the
normalised rows.  The kernel is given the true row count M; in the blocked layouts the buffers hold whole 32-row groups, which it
may write whole.  Behind them lie guard rows: they must come back untouched, and so must every buffer the call has no business
in (``xn`` when none is asked for, the attention rows when ``xn`` goes elsewhere).
"""
import math

import pytest
import torch

from mst import synth
from seam_ref import block_reference

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TOL = {"bf16": 1.5e-2, "fp16": 2.5e-3}
E, HID = 384, 1536
GUARD = 64                                  # sentinel rows behind the buffers
SENTINEL = 12288.0                          # exact in bf16 and fp16
ROWS = [1, 31, 33, 127, 129, 128 * 255 + 1, 128 * 256, 128 * 256 + 97, 128 * 513 + 5]


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


_case = {}                                  # the operands and the reference of the last (dt, M): six cases share them


def operands_and_reference(dt, M, weights):
    """x, attention rows and the fp64 block arithmetic on them (attention.py:67-68; block.py:89-94,112-113; mlp.py:34-40)."""
    if _case.get("key") != (dt, M):
        x = rnd((M, E), 60, 1.5) + 0.3
        att = rnd((M, E), 61, 1.0).to(DT[dt])
        _case.update(key=(dt, M), val=(x, att, *block_reference(x, att, weights)))   # the arithmetic: tests/seam_ref.py (the chain replay of test_encoder_seam_gpu.py shares it)
    return _case["val"]


@pytest.mark.parametrize("xn_mode", ["none", "own", "alias"])
@pytest.mark.parametrize("layout", [0, 7])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_block_boundary(hip, weights, dt, M, layout, xn_mode):
    tdt = DT[dt]
    wp, bp, w1, b1, w2, b2, g, be = weights
    x, att, ref, refn, scale = operands_and_reference(dt, M, weights)
    seq, b1f, pbf, b2f = hip.pack_block_seq(wp.cuda(), bp.cuda(), None, w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda(), g.cuda(), be.cuda(),
                                            None, tdt)
    # buffers: the rows the layout defines (whole 32-row groups when blocked), then guard rows nobody may touch
    Mp = (M + 31) // 32 * 32 if layout else M
    guarded = lambda body: torch.cat([body, torch.full((GUARD, E), SENTINEL, dtype=body.dtype, device="cuda")])
    xb = torch.cat([x.cuda(), torch.zeros(Mp - M, E, device="cuda")])
    ab = torch.cat([att.cuda(), torch.zeros(Mp - M, E, dtype=tdt, device="cuda")])
    if layout:
        xb, ab = hip.to_image32(xb), hip.to_blocked16(ab)
    x_full, a_full = guarded(xb), guarded(ab)
    n_full = torch.full((Mp + GUARD, E), SENTINEL, dtype=tdt, device="cuda")
    xn_full = {"none": None, "own": n_full, "alias": a_full}[xn_mode]

    # the kernel sees M rows of each buffer (one launch per case)
    hip.block_fused_s(x_full[:M], a_full[:M], seq, b1f, pbf, b2f, None if xn_full is None else xn_full[:M], layout=layout)
    torch.cuda.synchronize()

    got_x = (hip.from_image32(x_full[:Mp]) if layout else x_full)[:M]
    err_x = float((got_x.double().cpu() - ref).abs().max() / scale)
    print(f"{dt} M={M} layout={layout} xn={xn_mode}: x error {err_x:.3e} of scale (bar {TOL[dt]:g})")
    assert err_x < TOL[dt]
    if xn_full is not None:
        got_n = (hip.from_blocked16(xn_full[:Mp]) if layout else xn_full)[:M]
        err_n = float((got_n.double().cpu() - refn).abs().max())
        print(f"{dt} M={M} layout={layout} xn={xn_mode}: xn error {err_n:.3e} (bar {4 * TOL[dt]:g})")
        assert err_n < 4 * TOL[dt]
    # nothing behind the rows the layout defines was written, and no buffer the call did not name for writing
    sent = lambda t: bool((t.float() == SENTINEL).all())
    assert sent(x_full[Mp:]), "x: guard rows written"
    assert sent(a_full[Mp:]), "attention rows / aliased xn: guard rows written"
    assert sent(n_full[Mp:]), "xn: guard rows written"
    if xn_mode != "own":
        assert sent(n_full), "a buffer that was not passed was written"
    if xn_mode != "alias":
        assert torch.equal(a_full[:Mp], ab), "attention rows changed although xn_out is another buffer"


@pytest.mark.parametrize("layout", [1, 2, 4, 7])
def test_blocked_layouts_refuse_buffers_short_of_whole_groups(hip, weights, layout):
    """in the image / blocked layouts the kernel reads and writes whole 32-row groups (include/mst_hip.h, mst_layout_flags), so
    M = 300 needs 320 rows behind every operand a flag names.  The wrapper looks at the STORAGE behind each tensor: exactly sized
    tensors are refused before any launch (nothing is written), `buf[:M]` views of padded buffers -- what test_block_boundary passes --
    are taken, and the result is the block arithmetic like the row-major call's."""
    M, Mp, tdt = 300, 320, torch.bfloat16
    wp, bp, w1, b1, w2, b2, g, be = weights
    seq, b1f, pbf, b2f = hip.pack_block_seq(wp.cuda(), bp.cuda(), None, w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda(), g.cuda(), be.cuda(),
                                            None, tdt)
    x0, att0, ref, refn, scale = operands_and_reference("bf16", M, weights)
    x = torch.cat([x0.cuda(), torch.zeros(Mp - M, E, device="cuda")])
    att = torch.cat([att0.cuda(), torch.zeros(Mp - M, E, dtype=tdt, device="cuda")])
    short = dict(x=x[:M].clone(), attn_out=att[:M].clone(), xn_out=torch.full((M, E), SENTINEL, dtype=tdt, device="cuda"))
    named = [n for n, flags in (("x", 3), ("attn_out", 4), ("xn_out", 4)) if layout & flags]
    for name in named:                                   # one short operand at a time, the others padded
        ops = dict(x=x.clone()[:M], attn_out=att.clone()[:M], xn_out=torch.full((Mp, E), SENTINEL, dtype=tdt, device="cuda")[:M])
        ops[name] = short[name]
        before = {k: v.clone() for k, v in ops.items()}
        with pytest.raises(ValueError, match=f"block_fused_s: {name} is backed by 300 rows.*320 rows for M = 300"):
            hip.block_fused_s(ops["x"], ops["attn_out"], seq, b1f, pbf, b2f, ops["xn_out"], layout=layout)
        torch.cuda.synchronize()
        assert all(torch.equal(ops[k], before[k]) for k in ops), "a refused call launched"
    # an offset view counts from its own first element: the last 300 rows of a 320-row buffer have 300 rows behind them
    if layout & 3:
        with pytest.raises(ValueError, match="x is backed by 300 rows"):
            hip.block_fused_s(x.clone()[Mp - M:], att.clone()[:M], seq, b1f, pbf, b2f, None, layout=layout)
    if layout != 7:
        return
    # padded buffers: runs, and is the block arithmetic at the bars of test_block_boundary, like the row-major call on the same operands
    xr, nr = x[:M].clone(), torch.empty((M, E), dtype=tdt, device="cuda")
    hip.block_fused_s(xr, att[:M].clone(), seq, b1f, pbf, b2f, nr, layout=0)
    xb, ab, nb = hip.to_image32(x), hip.to_blocked16(att), torch.empty((Mp, E), dtype=tdt, device="cuda")
    hip.block_fused_s(xb[:M], ab[:M], seq, b1f, pbf, b2f, nb[:M], layout=7)
    for what, gx, gn in (("row-major", xr, nr), ("blocked", hip.from_image32(xb)[:M], hip.from_blocked16(nb)[:M])):
        assert float((gx.double().cpu() - ref).abs().max() / scale) < TOL["bf16"], what
        assert float((gn.double().cpu() - refn).abs().max()) < 4 * TOL["bf16"], what
