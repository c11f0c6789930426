"""Folded test-time augmentation on an MI355X: mst.saliency.run_pred(use_tta=True, tta="folded") -- one encoder pass over the four
in-plane flips instead of eight forwards -- against the reference's fixture, the CPU oracle and the loop it replaces, and the two
kernels of csrc/k_tta.hip at the op level.

Bars (tests/tta_ref.py restates the project's TOL table of tests/test_model_gpu.py): fp32 pred 1e-4 abs, volumes 1e-3 rel-L2; fp16
5e-3 and 1e-2.  Op level: mst_tta_inplane_flips copies bits (exact); mst_saliency_accumulate_tta is a sum of eight fp32 products of
positive terms, so eight roundings of 2^-24 relative each bound its error by ~5e-7 per element: rel-L2 < 1e-6.
"""
import numpy as np
import pytest
import torch

import tta_ref as R
from conftest import load_golden, rel_l2
from mst import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mst import hip as h
    h.load()
    return h


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_folded_run_pred_matches_reference_fixture(mode):
    """The three assertions and bars of test_run_pred_saliency_volume_matches_reference_fixture, on the folded path."""
    from mst.saliency import run_pred
    g = load_golden("saliency_tta_1x4x56x84")
    tl, tm = R.TOL[mode]
    model = R.build({}, int(g["seed"]), mode)
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    pred, weight, ws = run_pred(model, {"source": src, "uid": "x"}, save_attn=True, use_softmax=True, use_tta=True, tta="folded")
    assert np.abs(pred.cpu().numpy() - g["pred"]).max() < tl
    assert tuple(weight.shape) == g["weight"].shape and tuple(ws.shape) == g["weight"].shape
    assert weight.dtype == torch.float32 and ws.dtype == torch.float32
    assert rel_l2(weight.cpu(), g["weight"]) < tm
    assert rel_l2(ws[0, 0, :, 0, 0].cpu(), g["weight_slice_per_slice"]) < tm
    pred2, none_w, none_ws = run_pred(model, {"source": src}, save_attn=False, use_softmax=True, use_tta=True, tta="folded")
    assert none_w is None and none_ws is None and torch.allclose(pred2, pred, atol=1e-6)
    again = run_pred(model, {"source": src}, save_attn=True, use_softmax=True, use_tta=True, tta="folded")
    assert all(torch.equal(a, b) for a, b in zip(again, (pred, weight, ws)))          # fixed summation order: the same bits
    assert model.attention_maps == [] and model.attention_maps_slice == [] and model._cls_last is None   # no model state written
    with pytest.raises(RuntimeError):
        run_pred(model, {"source": torch.cat([src, src])}, save_attn=True, use_tta=True, tta="folded")


@pytest.mark.parametrize("name", list(R.ORDER_CASES))
def test_folded_run_pred_order_sensitive_cases_match_oracle_and_loop(name):
    """Slice positions (learned / rotary), odd D, a padding mask that the depth flip does not mirror: against the CPU oracle's eight
    forwards and against the loop on the same model, at the fp32 bars."""
    from mst.saliency import run_pred
    tl, tm = R.TOL["fp32"]
    model = R.build(R.ORDER_CASES[name], R.ORDER_SEED, "fp32")
    src, mask = R.order_inputs()
    batch = {"source": src, "src_key_padding_mask": mask}
    pred, weight, ws = run_pred(model, batch, save_attn=True, use_tta=True, tta="folded")
    refs = {"oracle": R.oracle_run_pred(name),
            "loop": tuple(t.cpu() for t in run_pred(model, batch, save_attn=True, use_tta=True, tta="loop"))}
    for what, (rp, rw, rs) in refs.items():
        errs = (float((pred.cpu() - rp).abs().max()), rel_l2(weight.cpu(), rw), rel_l2(ws.cpu(), rs))
        print(f"{name} folded vs {what}: pred {errs[0]:.2e} weight {errs[1]:.2e} weight_slice {errs[2]:.2e}")
        assert tuple(weight.shape) == tuple(rw.shape) == tuple(ws.shape)
        assert errs[0] < tl and errs[1] < tm and errs[2] < tm, (what, errs)


@pytest.mark.parametrize("fusion", ["transformer", "average"])
def test_folded_batches_and_raw_logits(fusion):
    """B = 2 without save_attn, softmax and raw logits: folded == loop at the fp32 logits bar; without use_tta the keyword is inert."""
    from mst.saliency import run_pred
    tl, _ = R.TOL["fp32"]
    model = R.build(dict(slice_fusion=fusion), 5, "fp32")
    src = synth.synth_volume((2, 1, 4, 28, 42), 105)
    mask = torch.tensor([[False, False, False, True], [False, True, False, False]])
    batch = {"source": src, "src_key_padding_mask": mask}
    for use_softmax in (True, False):
        folded = run_pred(model, batch, use_softmax=use_softmax, use_tta=True, tta="folded")
        loop = run_pred(model, batch, use_softmax=use_softmax, use_tta=True, tta="loop")
        assert folded[1] is None and folded[2] is None and folded[0].shape == loop[0].shape == (2, 2)
        err = float((folded[0] - loop[0]).abs().max())
        print(f"{fusion} softmax={use_softmax}: folded vs loop {err:.2e}")
        assert err < tl, err
    plain = run_pred(model, batch, save_attn=False, use_tta=False)
    assert torch.equal(run_pred(model, batch, save_attn=False, use_tta=False, tta="folded")[0], plain[0])
    one = {"source": src[:1], "src_key_padding_mask": mask[:1]}
    if fusion == "transformer":
        a, b = run_pred(model, one, save_attn=True, use_tta=False), run_pred(model, one, save_attn=True, use_tta=False, tta="folded")
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    else:                                                   # no slice attention to read: refused before the encoder runs
        with pytest.raises(RuntimeError, match="slice_fusion"):
            run_pred(model, one, save_attn=True, use_tta=True, tta="folded")


def test_folded_makes_one_encoder_call_on_four_flips():
    """Half the encoder work: ONE encode_slices call on 4*B*D rows and ONE fuse_slices call on 8*B volumes; the loop makes eight
    encoder calls of B*D rows."""
    from mst.saliency import run_pred
    model = R.build({}, 5, "fp32", use_graph="0")
    B, D = 2, 4
    batch = {"source": synth.synth_volume((B, 1, D, 28, 42), 105)}
    calls = {"encode": [], "fuse": []}
    encode, fuse = model.encode_slices, model.fuse_slices

    def counted_encode(slices, *a, **k):
        calls["encode"].append((int(slices.shape[0]), a, k))
        return encode(slices, *a, **k)

    def counted_fuse(emb, Bv, Dv, *a, **k):
        calls["fuse"].append((int(Bv), int(Dv)))
        return fuse(emb, Bv, Dv, *a, **k)
    model.encode_slices, model.fuse_slices = counted_encode, counted_fuse
    run_pred(model, batch, use_tta=True, tta="folded")
    assert [c[0] for c in calls["encode"]] == [4 * B * D] and calls["fuse"] == [(8 * B, D)], calls
    for v in calls.values():
        v.clear()
    run_pred(model, {"source": batch["source"][:1]}, save_attn=True, use_tta=True, tta="folded")
    (rows, a, k), = calls["encode"]
    assert rows == 4 * D and calls["fuse"] == [(8, D)]
    assert (list(a) + [k.get("n_layers_probs"), k.get("full")])[:2] == [model.encoder.depth, False], (a, k)   # last-block rows, never `full`
    for v in calls.values():
        v.clear()
    run_pred(model, batch, use_tta=True, tta="loop")
    assert [c[0] for c in calls["encode"]] == [B * D] * 8 and calls["fuse"] == [(B, D)] * 8, calls


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 28, 42), (2, 5, 30), (1, 14, 1), (3, 7, 33)])
def test_tta_inplane_flips_bit_equal_to_torch_flip(hip, shape, dtype):
    """x, flip H, flip W, flip both, bit for bit.  [2, 5, 30]: a width with a vector tail (30 = 7 x 4 + 2 fp32, 3 x 8 + 6 bf16);
    [3, 7, 33]: an odd width, so rows start off the 16-byte grid and the kernel's head elements are used too; [1, 14, 1]: one column."""
    gen = torch.Generator().manual_seed(shape[1] * 100 + shape[2])
    x = torch.randn(shape, generator=gen).to(dtype).cuda()
    out = hip.tta_inplane_flips(x)
    ref = torch.stack([x, torch.flip(x, (1,)), torch.flip(x, (2,)), torch.flip(x, (1, 2))])
    assert out.shape == ref.shape and out.dtype == dtype
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(out.view(bits), ref.view(bits))


def test_tta_inplane_flips_refusals(hip):
    x = torch.zeros(2, 4, 4, device="cuda")
    with pytest.raises(TypeError):
        hip.tta_inplane_flips(x.double())
    with pytest.raises(TypeError):
        hip.tta_inplane_flips(x.to(torch.int32))
    with pytest.raises(ValueError):
        hip.tta_inplane_flips(x[0])                                                   # rank
    with pytest.raises(ValueError):
        hip.tta_inplane_flips(x.cpu())
    with pytest.raises(ValueError):
        hip.tta_inplane_flips(x[:0])                                                  # empty
    with pytest.raises(ValueError):
        hip.tta_inplane_flips(x[:, :, ::2])                                           # not contiguous


def _tta_sum_fp64(plane, sa, g):
    """low[d,y,x] = sum_v headmean(plane[f_v][d])[y_f, x_f] * sa[v][r_v ? D-1-d : d] and ws[d] = sum_v sa[v][...], in float64."""
    plane, sa = plane.double(), sa.double()
    D = plane.shape[1]
    low, ws = torch.zeros(D, g, g, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
    for v, m in enumerate(R.TTA_MASKS):
        f, r = m >> 1, m & 1
        hm = plane[f].mean(dim=1)[:, :g * g].reshape(D, g, g)
        hm = torch.flip(hm, tuple(a for a, bit in ((1, 1), (2, 2)) if f & bit)) if f else hm
        w = sa[v].flip(0) if r else sa[v]
        low += hm * w[:, None, None]
        ws += w
    return low, ws


@pytest.mark.parametrize("Np", [24, 16])                    # 24: g = 4 with eight truncated columns
def test_saliency_accumulate_tta(hip, Np):
    D, heads, g = 5, 6, 4
    gen = torch.Generator().manual_seed(Np)
    plane = torch.rand(4, D, heads, Np, generator=gen) + 0.05
    sa = torch.rand(8, D, generator=gen) + 0.05
    low = torch.full((D, g, g), float("nan"), device="cuda")
    ws = torch.full((D,), float("nan"), device="cuda")
    hip.saliency_accumulate_tta(plane.cuda(), sa.cuda(), g, g, low, ws)
    ref_low, ref_ws = _tta_sum_fp64(plane, sa, g)
    errs = (rel_l2(low.cpu(), ref_low), rel_l2(ws.cpu(), ref_ws))
    print(f"saliency_accumulate_tta Np={Np}: rel-L2 low {errs[0]:.2e} slice {errs[1]:.2e}")
    assert max(errs) < 1e-6, errs
    # eight calls of the per-variant kernel on explicitly gathered inputs: variant v's maps as ITS forward would have produced them
    # (slice d' of a depth-flipped variant is slice D-1-d' of the volume), mirrored back by the kernel's flip mask
    low8, ws8 = torch.empty_like(low), torch.empty_like(ws)
    for v, m in enumerate(R.TTA_MASKS):
        pv = plane[m >> 1].flip(0) if m & 1 else plane[m >> 1]
        maps = (pv * sa[v][:, None, None]).contiguous()
        hip.saliency_accumulate(maps.cuda(), sa[v].contiguous().cuda(), g, g, m, low8, ws8, accumulate=v > 0)
    assert rel_l2(low.cpu(), low8.cpu()) < 1e-6 and rel_l2(ws.cpu(), ws8.cpu()) < 1e-6
    low2, ws2 = torch.empty_like(low), torch.empty_like(ws)
    hip.saliency_accumulate_tta(plane.cuda(), sa.cuda(), g, g, low2, ws2)
    assert torch.equal(low2, low) and torch.equal(ws2, ws)
    hip.saliency_accumulate_tta(plane.cuda(), sa.cuda(), g, g, low2, None)            # slice_acc is optional
    assert torch.equal(low2, low)
