"""End-to-end parity of the drop-in DinoV2ClassifierSlice on an MI355X against the fixtures the
REFERENCE produced (tests/golden, tools/gen_golden.py) and against the CPU oracle.

Tolerances (floating point; north_star: logits / attention maps within 1e-3 in fp32):
  fp32 mode  (exact fp32 MFMA)            logits 1e-4 abs, embeddings 2e-4 rel-L2, maps 1e-3 rel-L2
  fp16 mode  (TF32-class operands)        logits 5e-3 abs, embeddings 3e-3 rel-L2, maps 1e-2 rel-L2
  bf16 mode  (bench dtype, 8-bit mantissa) logits 3e-2 abs, embeddings 3e-2 rel-L2, maps 7e-2 rel-L2
Attention maps are compared relatively (entries are ~1/(D*Np): an absolute 1e-3 would be vacuous).
The 16-bit bars are <= 2x the worst error measured over all fixtures (tools/fixture_errors.py, profiles/r02a_fixture_errors.txt:
fp16 logits 3.2e-3 / emb 1.9e-3 / maps 4.7e-3; bf16 logits 2.1e-2 / emb 1.45e-2 / maps 3.5e-2).
"""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_l2
from mst import synth

pytestmark = pytest.mark.gpu

TOL = {  # mode -> (logits abs, emb rel, maps rel)
    "fp32": (1e-4, 2e-4, 1e-3),
    "fp16": (5e-3, 3e-3, 1e-2),
    "bf16": (3e-2, 3e-2, 7e-2),
}
CASES = {
    "c1_1x16x224": dict(),
    "b2_mask": dict(),
    "bottleneck_pos": dict(use_bottleneck=True, use_slice_pos_emb=True),
    "rope": dict(rotary_positional_encoding="RoPE"),
    "liere": dict(rotary_positional_encoding="LiRE"),
    "average": dict(slice_fusion="average"),
    "linear32": dict(slice_fusion="linear"),
    "size_b": dict(model_size="b"),
}


# The across-slice stage (bottleneck .. head) runs in fp32 in every mode, so whatever the logits deviate by is the encoder's
# embedding error carried through it.  Every case therefore checks the stage in isolation -- the HIP logits against the
# oracle's fusion of the HIP embeddings, at the fp32 bar -- and the fixture comparison of the two cases whose fusion amplifies
# that error (LieRE's 33 re-partitioned tokens; 'linear' summing 12,288 features into the head) is bounded by the error the
# oracle itself propagates from those embeddings instead of by a widened constant.
PROPAGATED = ("liere", "linear32")
STAGE_TOL = 2e-4


def build(name_kwargs, seed, mode, **extra):
    from mst.models import DinoV2ClassifierSlice
    kw = dict(name_kwargs)
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=mode, **kw, **extra)
    sd = synth.synth_state_dict(kw.get("model_size", "s"), seed,
                                use_bottleneck=kw.get("use_bottleneck", False),
                                use_slice_pos_emb=kw.get("use_slice_pos_emb", False),
                                slice_fusion=kw.get("slice_fusion", "transformer"),
                                rotary=kw.get("rotary_positional_encoding"))
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval()


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_reference_fixture(name, mode):
    g = load_golden(name)
    tl, te, tm = TOL[mode]
    model = build(CASES[name], int(g["seed"]), mode)
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    mask = torch.from_numpy(g["src_key_padding_mask"]) if "src_key_padding_mask" in g else None
    with torch.no_grad():
        logits = model(src, src_key_padding_mask=mask)                 # CPU input: forward moves it (dino.py:121)
        feats = model(src.cuda(), src_key_padding_mask=mask, without_linear=True)
    assert logits.shape == g["logits"].shape and logits.is_cuda
    B, _, D, H, W = src.shape
    with torch.no_grad():
        emb, _, _ = model.encode_slices(src.cuda().reshape(B * D, H, W))
    assert rel_l2(emb.cpu(), g["emb"]) < te
    # the fp32 across-slice stage alone: HIP logits vs the oracle's fusion of the HIP embeddings
    from oracle import mst_oracle as O
    kw = CASES[name]
    sd = synth.synth_state_dict(kw.get("model_size", "s"), int(g["seed"]), use_bottleneck=kw.get("use_bottleneck", False),
                                use_slice_pos_emb=kw.get("use_slice_pos_emb", False),
                                slice_fusion=kw.get("slice_fusion", "transformer"), rotary=kw.get("rotary_positional_encoding"))
    with torch.no_grad():
        staged = O.fuse(sd, emb.cpu(), B, D, slice_fusion_type=kw.get("slice_fusion", "transformer"),
                        src_key_padding_mask=mask, rotary=kw.get("rotary_positional_encoding"))
    stage_err = float((logits.cpu() - staged["logits"]).abs().max())
    assert stage_err < STAGE_TOL, stage_err
    err = np.abs(logits.cpu().numpy() - g["logits"]).max()
    if name in PROPAGATED and mode != "fp32":
        propagated = float((staged["logits"] - torch.from_numpy(g["logits"])).abs().max())   # embedding error through the exact stage
        assert err <= propagated + STAGE_TOL, (err, propagated)
    else:
        assert err < tl, err
    assert rel_l2(feats.cpu(), g["features"]) < te * 2
    if "attention_maps" not in g:
        return
    with torch.no_grad():
        logits2 = model(src, save_attn=True, src_key_padding_mask=mask)
    assert torch.equal(logits2, logits)                               # save_attn must not change the logits
    assert len(model.attention_maps) == 12 and model.attention_maps[-1].shape[2] == 1
    rows = torch.stack([m[:, :, 0] for m in model.attention_maps]).cpu()
    assert rel_l2(rows, g["vit_cls_rows"]) < tm
    assert rel_l2(model.attention_maps_slice[-1].cpu(), g["slice_map"]) < tm
    for _ in range(2):                                                # getters are idempotent
        assert rel_l2(model.get_plane_attention().cpu(), g["plane_attention"]) < tm
        sa = model.get_slice_attention()
        assert sa.shape == (B * D, 1, 1)
        assert rel_l2(sa.cpu(), g["slice_attention"]) < tm
        am = model.get_attention_maps()
        assert am.shape == g["attention_maps"].shape
        assert rel_l2(am.cpu(), g["attention_maps"]) < tm
    assert abs(float(model.get_attention_maps().sum()) - B * model.encoder.num_heads) < 1e-2


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_c3_full_size_volume_matches_reference_fixture(mode):
    """BASELINE config 3 shape: 1 x 64 x 518 x 518 (the legal realisation of '512^2') with attention."""
    g = load_golden("c3_1x64x518")
    tl, te, tm = TOL[mode]
    model = build({}, int(g["seed"]), mode)
    src = synth.synth_volume((1, 1, 64, 518, 518), int(g["seed"]) + 100)
    with torch.no_grad():
        logits = model(src.cuda(), save_attn=True)
        emb, _, _ = model.encode_slices(src.cuda().reshape(64, 518, 518))
    assert rel_l2(emb.cpu(), g["emb"]) < te
    assert np.abs(logits.cpu().numpy() - g["logits"]).max() < tl
    sub = g["plane_subset"].tolist()
    assert rel_l2(model.get_slice_attention().cpu(), g["slice_attention"]) < tm
    assert rel_l2(model.get_plane_attention().cpu()[sub], g["plane_attention"]) < tm
    assert rel_l2(model.get_attention_maps().cpu()[sub], g["attention_maps"]) < tm


def test_504_grid_and_chunking_are_consistent():
    """504^2 (36x36 grid, interpolated pos-embed) vs the reference fixture; chunked == unchunked bit-for-bit."""
    g = load_golden("s504_1x4x504")
    src = synth.synth_volume((1, 1, 4, 504, 504), int(g["seed"]) + 100).cuda()
    m1 = build({}, int(g["seed"]), "fp32")
    m2 = build({}, int(g["seed"]), "fp32", chunk_slices=3)
    with torch.no_grad():
        l1, l2 = m1(src), m2(src)
    assert np.abs(l1.cpu().numpy() - g["logits"]).max() < 1e-4
    assert torch.equal(l1, l2)


def test_properties_slice_permutation_and_batch_independence():
    """Size-independent properties at a shape the oracle does not cover: volumes of a batch are
    independent, and without slice position information the logits are invariant to slice order."""
    model = build({}, 5, "fp16")
    a = synth.synth_volume((1, 1, 6, 112, 154), 11).cuda()
    b = synth.synth_volume((1, 1, 6, 112, 154), 12).cuda()
    with torch.no_grad():
        la, lb = model(a), model(b)
        lab = model(torch.cat([a, b], 0))
        perm = torch.tensor([3, 1, 5, 0, 2, 4], device="cuda")
        lp = model(a[:, :, perm])
    assert torch.allclose(lab, torch.cat([la, lb], 0), atol=1e-5)
    assert torch.allclose(lp, la, atol=2e-5)


def test_error_behaviour_matches_reference():
    ref = json.loads((GOLDEN / "errors.json").read_text())
    model = build({}, 0, "bf16")
    with pytest.raises(AssertionError) as e:
        model(torch.zeros(1, 1, 2, 512, 512))
    assert str(e.value) == ref["512x512"]["message"]
    with pytest.raises(AssertionError) as e:
        model(torch.zeros(1, 1, 2, 224, 230))
    assert str(e.value) == ref["224x230"]["message"]
    from mst.models import DinoV2ClassifierSlice
    with pytest.raises(AssertionError) as e:
        DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, model_size="l")
    assert str(e.value) == ref["model_size_l"]["message"]
    # 'linear' fusion: the head is nn.Linear(32 * emb, out) (dino.py:245), so any D != 32 is nn.Linear's shape error
    lin = build(dict(slice_fusion="linear"), 5, "fp32")
    for D in (16, 48):
        with pytest.raises(RuntimeError, match="shapes cannot be multiplied"), torch.no_grad():
            lin(torch.zeros(1, 1, D, 28, 28))
    with torch.no_grad():
        assert lin(torch.zeros(1, 1, D, 28, 28), without_linear=True).shape == (1, D * 384)   # features alone have no such limit


def test_hub_layout_layerscale_registers_against_oracle():
    """Hub key layout (blocks.<i>, ls gammas, 518 pos-embed) + 4 register tokens: checked against the
    CPU oracle (the reference cannot build this configuration offline: it needs torch.hub)."""
    from oracle import mst_oracle as O
    from mst.models.dino import _ViT
    from mst.models import DinoV2ClassifierSlice
    sd = synth.synth_state_dict("s", 9, img_size=518, layerscale=True, chunked=False, num_register_tokens=4)
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", use_registers=True)
    model.encoder = _ViT(384, 12, 6, img_size=518, num_register_tokens=4, layerscale=1.0, chunked=False)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    src = synth.synth_volume((1, 1, 3, 70, 98), 21)
    with torch.no_grad():
        logits = model(src, save_attn=True)
        ref = O.forward(sd, src, keep="cls")
    assert np.abs(logits.cpu().numpy() - ref["logits"].numpy()).max() < 1e-4
    assert rel_l2(model.get_plane_attention().cpu(), O.plane_attention(ref["vit_maps"][-1], 4)) < 1e-3
    assert rel_l2(model.get_attention_maps().cpu(), O.attention_maps(ref["vit_maps"][-1], ref["slice_map"], 4)) < 1e-3


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_attention_rollout_matches_reference_fixture(mode):
    """get_attention_cls (dino.py:204-212): full [n,h,N,N] maps of all 12 layers, chained on the device."""
    g = load_golden("rollout_1x3x84")
    model = build({}, int(g["seed"]), mode, full_attention_maps=True)
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    with torch.no_grad():
        logits = model(src, save_attn=True)
        roll = model.get_attention_cls()
    tl, _, tm = TOL[mode]
    assert np.abs(logits.cpu().numpy() - g["logits"]).max() < tl
    assert len(model.attention_maps) == 12 and tuple(model.attention_maps[0].shape) == g["vit_full_first"].shape
    assert rel_l2(model.attention_maps[0].cpu(), g["vit_full_first"]) < tm
    assert rel_l2(model.attention_maps[-1].cpu(), g["vit_full_last"]) < tm
    assert tuple(roll.shape) == g["attention_cls"].shape
    assert rel_l2(roll.cpu(), g["attention_cls"]) < tm
    # without the full maps the rollout must refuse, not approximate
    plain = build({}, int(g["seed"]), mode)
    with torch.no_grad():
        plain(src, save_attn=True)
    with pytest.raises(RuntimeError):
        plain.get_attention_cls()


def test_liere_restrictions_raise_like_the_reference():
    """LieRE in the reference only runs for B == 1, D == 32 (errors.json: RuntimeError from its views)."""
    err = json.loads((GOLDEN / "errors.json").read_text())
    model = build(dict(rotary_positional_encoding="LiRE"), 9, "fp32")
    for tag, shape in (("liere_batch2", (2, 1, 32, 28, 28)), ("liere_d16", (1, 1, 16, 28, 28))):
        assert err[tag]["type"] == "RuntimeError"
        with pytest.raises(RuntimeError), torch.no_grad():
            model(torch.zeros(*shape))


def _shard_worker(rank, world, port, ret):
    import os
    import sys
    import torch.distributed as dist
    from conftest import ROOT
    sys.path.insert(0, str(ROOT / "tools"))
    from rehearsal import HostStagedSharding              # both ranks share cuda:0: RCCL refuses duplicate devices
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    g = load_golden("b2_mask")
    model = build(CASES["b2_mask"], int(g["seed"]), "fp16")
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    mask = torch.from_numpy(g["src_key_padding_mask"])
    res = {}
    with torch.no_grad():
        ref = model(src, src_key_padding_mask=mask, save_attn=True)
        ref_maps, ref_plane = model.get_attention_maps(), model.get_plane_attention()
        ref_rows = torch.stack([m[:, :, 0] for m in model.attention_maps])
        model.enable_slice_sharding(sharding=HostStagedSharding())
        out = model(src, src_key_padding_mask=mask, save_attn=True)      # D = 6 over 2 ranks
        res["logits"] = bool(torch.equal(out, ref))
        res["maps"] = bool(torch.equal(model.get_attention_maps(), ref_maps) and torch.equal(model.get_plane_attention(), ref_plane))
        # only the LAST block's rows travel; the earlier list entries are this rank's own slices
        B, D = 2, 6
        d0, d1, _ = model._sharding.shard_range(D)
        own = ref_rows.view(12, B, D, *ref_rows.shape[2:])[:, :, d0:d1].reshape(12, B * (d1 - d0), *ref_rows.shape[2:])
        res["own_rows"] = bool(torch.equal(torch.stack([m[:, :, 0] for m in model.attention_maps]), own))
        model.enable_slice_sharding(sharding=HostStagedSharding(), gather_all_layers=True)
        model(src, src_key_padding_mask=mask, save_attn=True)
        res["all_rows"] = bool(torch.equal(torch.stack([m[:, :, 0] for m in model.attention_maps]), ref_rows))
    res["err"] = float((out.cpu() - torch.from_numpy(g["logits"])).abs().max())

    # rollout (get_attention_cls, dino.py:204-212) under sharding: D = 3 over 2 ranks is an UNEVEN split (2 + 1 slices)
    g = load_golden("rollout_1x3x84")
    model = build({}, int(g["seed"]), "fp32", full_attention_maps=True)
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    with torch.no_grad():
        ref = model(src, save_attn=True)
        ref_roll = model.get_attention_cls()
        model.enable_slice_sharding(sharding=HostStagedSharding())
        out = model(src, save_attn=True)
        roll = model.get_attention_cls()
        local = model.get_attention_cls(gather=False)
    d0, d1, _ = model._sharding.shard_range(3)
    res["roll_logits"] = bool(torch.equal(out, ref))
    res["roll"] = bool(torch.equal(roll, ref_roll))
    res["roll_local"] = bool(torch.equal(local, ref_roll[d0:d1]))
    res["roll_err"] = rel_l2(roll.cpu(), g["attention_cls"])
    ret[rank] = res
    dist.destroy_process_group()


def test_slice_sharded_forward_equals_unsharded_two_ranks_one_gpu():
    """slices sharded over ranks + all-gather of embeddings / CLS rows must reproduce the single-rank
    forward bit-for-bit (slices are independent in the encoder; the fusion stage is replicated) -- logits, attention
    read-outs and the sharded rollout (BASELINE configs[2]: `--get_attention` rollout with slices sharded)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, 29533, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    for r in range(2):
        res = ret[r]
        for key in ("logits", "maps", "own_rows", "all_rows", "roll_logits", "roll", "roll_local"):
            assert res[key], (r, key, res)
        assert res["err"] < TOL["fp16"][0]
        assert res["roll_err"] < TOL["fp32"][2]


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_graph_replay_equals_eager(mode):
    """hipGraph replay of the inference forward (small fixed shapes): logits, the attention read-outs and the
    stored maps are the eager ones bit for bit, for new inputs and after a weight update (the captured graph points into the
    prepared weight images, so it is dropped with them)."""
    g = load_golden("b2_mask")
    mg = build(CASES["b2_mask"], int(g["seed"]), mode, use_graph="1")
    me = build(CASES["b2_mask"], int(g["seed"]), mode, use_graph="0")
    mask = torch.from_numpy(g["src_key_padding_mask"])
    shape = tuple(int(v) for v in g["shape"])
    with torch.no_grad():
        for it in range(6):                              # calls 1-2 eager, 3 captures, 4+ replay
            src = synth.synth_volume(shape, int(g["seed"]) + 100 + it)
            a = mg(src, src_key_padding_mask=mask, save_attn=True)
            b = me(src, src_key_padding_mask=mask, save_attn=True)
            assert torch.equal(a, b), it
            assert torch.equal(mg.get_attention_maps(), me.get_attention_maps()), it
            assert torch.equal(mg.get_slice_attention(), me.get_slice_attention()), it
            assert torch.equal(torch.stack(mg.attention_maps), torch.stack(me.attention_maps)), it
        assert any(e["graph"] is not None for e in mg._graphs.values())
        # plain call (other key), then a weight update: both models follow
        for it in range(4):
            assert torch.equal(mg(src), me(src))
        for m in (mg, me):
            m.linear.weight.mul_(1.25)
            dict(m.named_parameters())["encoder.blocks.0.5.mlp.fc1.weight" if "encoder.blocks.0.5.mlp.fc1.weight" in dict(m.named_parameters())
                                       else "encoder.blocks.5.mlp.fc1.weight"].mul_(0.9)
        for it in range(4):
            assert torch.equal(mg(src, src_key_padding_mask=mask), me(src, src_key_padding_mask=mask)), it


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_graph_replay_after_the_workspace_has_grown(mode):
    """a captured graph holds raw pointers into the encoder's and the fusion's workspaces, and a volume with more slices
    replaces both tensors.  The graph's entry owns the workspaces of its capture (mst/models/prepared.py, pin_workspaces), so a replay
    of the earlier shape writes its scratch into memory nobody else can have been given: victim tensors of exactly the replaced sizes,
    allocated after the growth (where the caching allocator would hand out a freed workspace first), keep every byte -- the replay's own
    results cannot show this, its scratch is written before it is read -- and both shapes stay the eager model's bit for bit."""
    g = load_golden("b2_mask")
    mg = build(CASES["b2_mask"], int(g["seed"]), mode, use_graph="1")
    me = build(CASES["b2_mask"], int(g["seed"]), mode, use_graph="0")
    mask_a = torch.from_numpy(g["src_key_padding_mask"])
    shape_a = tuple(int(v) for v in g["shape"])
    shape_b = shape_a[:2] + (2 * shape_a[2],) + shape_a[3:]
    mask_b = torch.cat([mask_a, torch.zeros_like(mask_a)], dim=1)
    seed = int(g["seed"]) + 300

    def both(shape, mask, it):
        src = synth.synth_volume(shape, seed + it)
        a = mg(src, src_key_padding_mask=mask, save_attn=True)
        b = me(src, src_key_padding_mask=mask, save_attn=True)
        assert torch.equal(a, b), (shape, it)
        assert torch.equal(mg.get_attention_maps(), me.get_attention_maps()), (shape, it)
        assert torch.equal(mg.get_slice_attention(), me.get_slice_attention()), (shape, it)
        assert torch.equal(torch.stack(mg.attention_maps), torch.stack(me.attention_maps)), (shape, it)

    with torch.no_grad():
        for it in range(4):                              # calls 1-2 eager, 3 captures and replays, 4 replays
            both(shape_a, mask_a, it)
        ent = next(e for e in mg._graphs.values() if e["graph"] is not None)
        old = dict(mg._ws)
        assert set(old) == {"vit", "fusion"}
        sizes = {k: t.numel() * t.element_size() for k, t in old.items()}
        both(shape_b, mask_b, 4)                         # twice the slices: both workspaces are replaced
        assert mg._ws["vit"] is not old["vit"] and mg._ws["fusion"] is not old["fusion"]
        assert mg._ws["vit"].numel() > old["vit"].numel()
        old = {k: t.data_ptr() for k, t in old.items()}  # (no reference of the test's own keeps the replaced tensors alive)
        victims = [torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda") for n in sizes.values() for _ in range(4)]
        for it in (5, 6):                                # replays of A: new inputs
            both(shape_a, mask_a, it)
        torch.cuda.synchronize()
        assert all(bool((v == 0xA5).all()) for v in victims), "a replay wrote into memory the model no longer owns"
        both(shape_b, mask_b, 7)
        assert all(bool((v == 0xA5).all()) for v in victims)
        assert {k: t.data_ptr() for k, t in ent["ws"].items()} == old     # why: the entry still owns the workspaces of its capture


def _rccl_worker(port, ret):
    import os
    import torch.distributed as dist
    # dmabuf IPC is the only mode the host driver supports; without it RCCL fails with hipIpcGetMemHandle: invalid argument
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)                 # backend "nccl" IS RCCL on ROCm
    g = load_golden("b2_mask")
    model = build(CASES["b2_mask"], int(g["seed"]), "fp16")
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    mask = torch.from_numpy(g["src_key_padding_mask"])
    res = {}
    with torch.no_grad():
        ref = model(src, src_key_padding_mask=mask, save_attn=True)
        ref_maps = model.get_attention_maps()
        model.enable_slice_sharding()                                      # the product class: SliceSharding over the default (RCCL) group
        res["backend"] = dist.get_backend()
        out = model(src, src_key_padding_mask=mask, save_attn=True)
        res["logits"] = bool(torch.equal(out, ref))
        res["maps"] = bool(torch.equal(model.get_attention_maps(), ref_maps))
        t = torch.tensor([1.0, 5.0, 3.0], device="cuda")
        res["max"] = bool(torch.equal(model._sharding.all_reduce_max(t.clone()), t))
    torch.cuda.synchronize()
    ret[0] = res
    dist.destroy_process_group()


def test_slice_sharding_over_rccl_world_size_one():
    """every other multi-rank test uses gloo or the host-staged rehearsal transport, so
    SliceSharding._all_gather on DEVICE tensors over backend "nccl" (= RCCL) had never executed.  A one-GPU box cannot hold two
    RCCL ranks (duplicate devices are refused), but world_size 1 runs the real all_gather_into_tensor path end to end."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    p = ctx.Process(target=_rccl_worker, args=(29541, ret))
    p.start()
    p.join(300)
    assert p.exitcode == 0
    res = ret[0]
    assert res["backend"] == "nccl"
    assert res["logits"] and res["maps"] and res["max"], res


def test_full_bench_batch_matches_single_volume_and_reference_fixture():
    """BASELINE configs[1] at full size: 4 x 64 x 518^2 in bf16, one launch sequence over 350,720 tokens.  Volume 0 is the
    input of the reference fixture c3_1x64x518: its logits / embeddings inside the batch must be bit-equal to the
    single-volume run (slices are independent rows of every kernel) and within the bf16 bar of what the reference produced."""
    g = load_golden("c3_1x64x518")
    tl, te, _ = TOL["bf16"]
    model = build({}, int(g["seed"]), "bf16")
    gen = torch.Generator().manual_seed(7)
    vols = torch.randn((4, 1, 64, 518, 518), generator=gen)
    vols[0] = synth.synth_volume((1, 1, 64, 518, 518), int(g["seed"]) + 100)[0]
    vols = vols.to(torch.bfloat16).cuda()
    with torch.no_grad():
        batch = model(vols)
        single = model(vols[:1])
        emb_b, _, _ = model.encode_slices(vols.reshape(256, 518, 518))
        emb_s, _, _ = model.encode_slices(vols[0].reshape(64, 518, 518))
        last = model(vols[3:])
    assert torch.equal(batch[:1], single) and torch.equal(batch[3:], last)
    assert torch.equal(emb_b[:64], emb_s)
    assert np.abs(batch[:1].cpu().numpy() - g["logits"]).max() < tl
    assert rel_l2(emb_b[:64].cpu(), g["emb"]) < te


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["saliency_1x5x84", "saliency_tta_1x4x56x84"])
def test_run_pred_saliency_volume_matches_reference_fixture(name, mode):
    """mst.saliency.run_pred == scripts/main_predict.py run_pred(save_attn=True[, use_tta]) on the reference model."""
    from mst.saliency import run_pred
    g = load_golden(name)
    tl, _, tm = TOL[mode]
    model = build({}, int(g["seed"]), mode)
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    pred, weight, ws = run_pred(model, {"source": src, "uid": "x"}, save_attn=True, use_softmax=True, use_tta=bool(g["use_tta"]))
    assert np.abs(pred.cpu().numpy() - g["pred"]).max() < tl
    assert tuple(weight.shape) == g["weight"].shape and tuple(ws.shape) == g["weight"].shape
    assert rel_l2(weight.cpu(), g["weight"]) < tm
    assert rel_l2(ws[0, 0, :, 0, 0].cpu(), g["weight_slice_per_slice"]) < tm
    pred2, none_w, none_ws = run_pred(model, {"source": src}, save_attn=False, use_softmax=True, use_tta=bool(g["use_tta"]))
    assert none_w is None and none_ws is None and torch.allclose(pred2, pred, atol=1e-6)
    with pytest.raises(RuntimeError):
        run_pred(model, {"source": torch.cat([src, src])}, save_attn=True)


def test_forward_is_hipgraph_capturable():
    """Nothing in the C ABI allocates or synchronises, so a forward (workspaces warmed) can be captured into a hipGraph
    and replayed: same bits as the eager call."""
    g = load_golden("c1_1x16x224")
    model = build(CASES["c1_1x16x224"], int(g["seed"]), "fp16")
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100).cuda()
    with torch.no_grad():
        eager = model(src)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model(src)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(src)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert np.abs(out.cpu().numpy() - g["logits"]).max() < TOL["fp16"][0]


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_hub_register_encoder_matches_reference_class_fixture(mode):
    """Encoder in the hub's dinov2_vits14_reg configuration (registers, LayerScale, 518 grid, anti-aliased size-based
    position resampling) vs the vendored reference class built with those arguments (tests/golden/hub_reg.npz)."""
    from mst.models.dino import _ViT
    from mst.models import DinoV2ClassifierSlice
    g = load_golden("hub_reg")
    sd = synth.synth_state_dict("s", int(g["seed"]), img_size=518, layerscale=True, chunked=False, num_register_tokens=4)
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=mode, use_registers=True)
    model.encoder = _ViT(384, 12, 6, img_size=518, num_register_tokens=4, layerscale=1.0, chunked=False)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    te = TOL[mode][1]
    for tag in ("224", "112x140", "518"):
        shape = tuple(int(v) for v in g[f"shape_{tag}"])
        x = synth.synth_volume((1, 1) + shape, int(g["seed"]) + 100)[0, 0].cuda()
        with torch.no_grad():
            emb, _, _ = model.encode_slices(x)
        assert rel_l2(emb.cpu(), g[f"emb_{tag}"]) < te, tag


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_multichannel_input_matches_reference_fixture(mode):
    """C = 3 volumes: channels become extra slices, channel fastest (dino.py:125); mask over D*C positions."""
    g = load_golden("multichannel")
    tl, _, tm = TOL[mode]
    model = build({}, int(g["seed"]), mode)
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    mask = torch.from_numpy(g["src_key_padding_mask"])
    with torch.no_grad():
        logits = model(src, src_key_padding_mask=mask, save_attn=True)
        maps = model.get_attention_maps()
        sa = model.get_slice_attention()
    assert np.abs(logits.cpu().numpy() - g["logits"]).max() < tl
    assert rel_l2(maps.cpu(), g["attention_maps"]) < tm
    assert rel_l2(sa.cpu(), g["slice_attention"]) < tm


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_massive_activation_channels_against_oracle(mode):
    """Pretrained DINOv2 carries a few residual-stream channels with magnitudes in the hundreds.  Emulate them (two fc2
    output channels and their bias scaled x200 in block 3) and check that nothing in the 16-bit paths saturates: the
    LayerNorms see rows dominated by two outliers, the residual stream stays fp32."""
    from oracle import mst_oracle as O
    sd = synth.synth_state_dict("s", 31)
    pre = "encoder.blocks.0.3.mlp.fc2."
    for ch in (7, 200):
        sd[pre + "weight"][ch] *= 200.0
        sd[pre + "bias"][ch] = 150.0
    from mst.models import DinoV2ClassifierSlice
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=mode)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    src = synth.synth_volume((1, 1, 3, 112, 112), 77)
    with torch.no_grad():
        emb, _, _ = model.encode_slices(src.cuda().reshape(3, 112, 112))
        ref, _ = O.vit_encode(sd, src.reshape(3, 112, 112))
    assert bool(torch.isfinite(emb).all())
    assert rel_l2(emb.cpu(), ref) < {"fp32": 2e-4, "fp16": 6e-3, "bf16": 6e-2}[mode]


@pytest.mark.parametrize("shape", [(1, 1, 1, 14, 14), (2, 1, 256, 28, 28), (1, 1, 2, 14, 518), (3, 1, 5, 98, 14)])
def test_extreme_shapes_against_oracle(shape):
    """One slice of one patch (N = 2, L = 2); the maximum slice count of the slice position table (L = 257); one-patch-high
    and one-patch-wide grids (bicubic resampling to a 1 x 37 / 7 x 1 grid)."""
    from oracle import mst_oracle as O
    sd = synth.synth_state_dict("s", 5, use_slice_pos_emb=True)
    from mst.models import DinoV2ClassifierSlice
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", use_slice_pos_emb=True)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    src = synth.synth_volume(shape, 3)
    B, D = shape[0], shape[2]
    mask = torch.zeros(B, D, dtype=torch.bool)
    if D > 2:
        mask[0, -2:] = True
    with torch.no_grad():
        logits = model(src, src_key_padding_mask=mask, save_attn=True)
        maps = model.get_attention_maps()
        ref = O.forward(sd, src, src_key_padding_mask=mask, keep="cls")
    assert np.abs(logits.cpu().numpy() - ref["logits"].numpy()).max() < 1e-4
    ref_maps = O.attention_maps(ref["vit_maps"][-1], ref["slice_map"])
    finite = torch.isfinite(ref_maps)
    assert bool((torch.isfinite(maps.cpu()) == finite).all())       # N = 2: the only patch is zeroed -> 0/0 in the reference too
    if bool(finite.all()):
        assert rel_l2(maps.cpu(), ref_maps) < 1e-3


@pytest.mark.parametrize("mode", ["fp16", "bf16"])
@pytest.mark.parametrize("case", ["nonsquare_fp32_volume", "hub_registers_bf16_volume"])
def test_fused_token_kernel_against_oracle(case, mode):
    """k_patch_rows.hip (patch embedding + prefix rows + block 0's LayerNorm in one pass; taken by the fused 16-bit pipeline from
    12,288 tokens per call): a non-square grid with an fp32 volume and a ragged last chunk of patches, and the hub layout with four
    register tokens (n_prefix = 5) on a 16-bit volume -- against the CPU oracle at the bars of the fixture tests."""
    from oracle import mst_oracle as O
    tl, te, _ = TOL[mode]
    if case == "nonsquare_fp32_volume":
        model = build({}, 17, mode)
        sd = synth.synth_state_dict("s", 17)
        src = synth.synth_volume((1, 1, 13, 518, 392), 5)                 # 13 x (37 x 28 + 1) = 13,481 tokens; 13,468 patches = 420.9 chunks
        ref = O.forward(sd, src, keep="cls")
        vol = src
    else:
        from mst.models import DinoV2ClassifierSlice
        from mst.models.dino import _ViT
        sd = synth.synth_state_dict("s", 9, img_size=518, layerscale=True, chunked=False, num_register_tokens=4)
        model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=mode, use_registers=True)
        model.encoder = _ViT(384, 12, 6, img_size=518, num_register_tokens=4, layerscale=1.0, chunked=False)
        model.load_state_dict(sd, strict=True)
        model = model.cuda().eval()
        src = synth.synth_volume((1, 1, 10, 518, 518), 6)
        vol = src.to(torch.bfloat16 if mode == "bf16" else torch.float16)
        ref = O.forward(sd, vol.float(), keep="cls")
    with torch.no_grad():
        logits = model(vol.cuda())
        emb, _, _ = model.encode_slices(vol.cuda().reshape(-1, vol.shape[-2], vol.shape[-1]))
    assert rel_l2(emb.cpu(), ref["emb"]) < te
    assert float((logits.cpu() - ref["logits"]).abs().max()) < tl


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_prune_last_block_gives_the_same_outputs(mode):
    """Opt-in ``prune_last_block=True``: the last block computes K/V of every token and the attention + MLP of the class tokens
    only.  Logits, embeddings and every attention read-out must match the reference fixture at the same bars as the full
    computation, and the full computation itself closely (different kernels for 64 of 87,680 rows: rounding only)."""
    tl, te, tm = TOL[mode]
    g = load_golden("c3_1x64x518")
    src = synth.synth_volume((1, 1, 64, 518, 518), int(g["seed"]) + 100)
    full = build({}, int(g["seed"]), mode)
    pruned = build({}, int(g["seed"]), mode, prune_last_block=True)
    with torch.no_grad():
        l_full = full(src, save_attn=True)
        l_pr = pruned(src, save_attn=True)
        emb, _, _ = pruned.encode_slices(src.cuda().reshape(64, 518, 518))
    assert rel_l2(emb.cpu(), g["emb"]) < te
    assert np.abs(l_pr.cpu().numpy() - g["logits"]).max() < tl
    assert float((l_pr - l_full).abs().max()) < tl
    sub = g["plane_subset"].tolist()
    assert rel_l2(pruned.get_slice_attention().cpu(), g["slice_attention"]) < tm
    assert rel_l2(pruned.get_plane_attention().cpu()[sub], g["plane_attention"]) < tm
    assert rel_l2(pruned.get_attention_maps().cpu()[sub], g["attention_maps"]) < tm
    # small call (unfused path) and registers: against the full computation
    small = synth.synth_volume((2, 1, 5, 112, 84), 3)
    with torch.no_grad():
        assert float((pruned(small) - full(small)).abs().max()) < tl


@pytest.mark.parametrize("prune", [False, True])
def test_chunked_equals_unchunked_on_the_fused_16bit_pipeline(prune):
    """The fused pipeline (token kernel, weights-in-registers QKV, LDS-DMA attention, block kernel) is row-independent and
    deterministic: encoding 20 slices in chunks of 7 (7 + 7 + 6, the last chunk with other tile / chunk tails) gives bit-identical
    embeddings and logits; with and without the opt-in last-block pruning."""
    src = synth.synth_volume((1, 1, 20, 518, 518), 77).to(torch.bfloat16)
    m1 = build({}, 5, "bf16", prune_last_block=prune)
    m2 = build({}, 5, "bf16", chunk_slices=7, prune_last_block=prune)
    with torch.no_grad():
        l1, l2 = m1(src.cuda(), save_attn=True), m2(src.cuda(), save_attn=True)
        e1, _, _ = m1.encode_slices(src.cuda().reshape(20, 518, 518))
        e2, _, _ = m2.encode_slices(src.cuda().reshape(20, 518, 518))
    assert torch.equal(e1, e2)
    assert torch.equal(l1, l2)
    assert torch.equal(m1.get_attention_maps(), m2.get_attention_maps())
