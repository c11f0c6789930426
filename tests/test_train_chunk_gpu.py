"""train_chunk_slices = k > 0 of the DinoV2ClassifierSlice training step (mst/train.py): the encoder recomputed per chunk of k slices in the
backward instead of its state kept from the forward, and the frozen encoder that keeps nothing.

No bar of its own: float64 autograd at the bar of tests/train_parity.py (1e-4 of max |ref|: tests/test_train_parity_cpu.py justifies it) for
the fp32 step; bit equality where the arithmetic is the same (one chunk; a frozen encoder's head and fusion gradients; a second step under
the deterministic flag); the project's factor 2 between sibling modes (tests/test_train_storage_gpu.py) for the 16-bit modes, chunked against
unchunked, each against the fp32 step; the block-state table (40 E bytes per token and block with 16-bit storage) with that file's 0.75
for the peak; the comparisons and bars of tests/test_shard_train_gpu.py under slice sharding.  Every figure is printed before it is asserted.

Measured on the MI355X: the chunked fp32 step's worst scaled gradient error over the five cases 1.30e-5 (vitb_126tok, the plain step's own
figure), d source 8.8e-6, logits 1.9e-6; 16-bit modes, chunked error / plain error per tensor at most 1.01 (610 tensors); saved state
besides the volume 0.24 % of the plain step's block state; peak of the (1, 1, 8, 518, 518) step 2.59 -> 1.10 GiB (1.59 GB saved, 1.14 GB
asked); sharded and chunked fp32 step against the plain one 5.8e-7 of max |ref|, logits equal; fp16 / flash / 16bit sharded and chunked
(2.65e-3, 6.01e-3, 5.39e-3) against the plain step's (2.65e-3, 6.16e-3, 5.46e-3).
"""
import time
import traceback

import pytest
import torch
import torch.nn.functional as F

import train_parity as P
from mst import synth, train
from test_model_gpu import TOL, build
from test_train_storage_gpu import _deterministic, _reachable_bytes, _rel

pytestmark = pytest.mark.gpu

MODES16 = {
    "fp16_stored_fp32": dict(train_precision="fp16", train_attention="stored", train_storage="fp32"),
    "bf16_flash_fp32": dict(train_precision="bf16", train_attention="flash", train_storage="fp32"),
    "fp16_flash_16bit": dict(train_precision="fp16", train_attention="flash", train_storage="16bit"),
}
FP32 = dict(train_precision="fp32", train_attention="stored", train_storage="fp32")


def _step(model, src, target, mask=None, want_src=True):
    """One step: (logits, {parameter name: gradient or None, "<source>": d source}); the tensors are this step's own."""
    model.zero_grad(set_to_none=True)
    source = src.cuda().requires_grad_(want_src)
    logits = model(source, src_key_padding_mask=mask)
    F.cross_entropy(logits, target.cuda()).backward()
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}
    grads[P.SOURCE] = source.grad
    return logits.detach().clone(), grads


def _assert_same_bits(a, b):
    (la, ga), (lb, gb) = a, b
    assert torch.equal(la, lb)
    assert set(ga) == set(gb)
    for k in ga:
        assert (ga[k] is None and gb[k] is None) or (ga[k] is not None and gb[k] is not None and torch.equal(ga[k], gb[k])), k


# ---- 1: the fp32 step against float64 autograd ------------------------------------------------------------------------------------------

# case -> k: 6 rows as 4 + 2 (ragged, across the volume boundary); 132 as 50 + 50 + 32; 70 as 32 + 32 + 6; 2 as 1 + 1 (the interpolated
# position grid's gradient summed over chunks); 1 row under k = 4 (k >= rows)
CHUNK = {"vitb_126tok": 4, "slices66_mask_pos": 50, "slices70_rope": 32, "grid_1x37": 1, "tokens1370": 4}


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("case", list(P.CASES))
def test_chunked_fp32_step_matches_float64_autograd(case, det):
    kw, src, mask, target = P.inputs(case)
    loss_ref, logits_ref, ref = P.oracle_grads(case, torch.float64)
    with _deterministic(det):
        model = build(kw, P.STATE_SEED, "fp32", train_chunk_slices=CHUNK[case]).train()
        logits, got = _step(model, src, target, mask)
        loss = float(F.cross_entropy(logits, target.cuda()))
        errs = P.scaled_errors(got, ref)
        worst = max(errs, key=errs.get)
        dlogits = float((logits.cpu().double() - logits_ref).abs().max())
        print(f"{case} k={CHUNK[case]} deterministic={det}: worst scaled gradient error {errs[worst]:.3e} ({worst}), source {errs[P.SOURCE]:.3e}, "
              f"logits {dlogits:.3e}, loss {abs(loss - loss_ref):.3e}")
        assert abs(loss - loss_ref) < 1e-4
        assert dlogits < TOL["fp32"][0], dlogits
        for k, g in got.items():
            assert g is None or bool(torch.isfinite(g).all()), k
        P.check(got, ref)
        if det:
            _assert_same_bits(_step(model, src, target, mask), (logits, got))


# ---- 2: one chunk is the plain step -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["fp32", "bf16_flash_16bit"])
def test_a_single_chunk_is_the_plain_step_bit_for_bit(mode):
    """(1, 1, 4, 56, 56) under the deterministic flag: k = 4 (exactly the rows) and k = 8 (more) give the bits of k = 0 -- logits, every
    gradient, d source.  The recomputed forward is the forward, and a first `_Grads.put` keeps what it is given."""
    kw = FP32 if mode == "fp32" else dict(train_precision="bf16", train_attention="flash", train_storage="16bit")
    src, tgt = synth.synth_volume((1, 1, 4, 56, 56), 7), torch.tensor([1])
    with _deterministic():
        model = build({}, 0, "fp32", **kw).train()
        plain = _step(model, src, tgt)
        assert plain[1][P.SOURCE] is not None and sum(g is not None for g in plain[1].values()) > 100
        for k in (4, 8):
            model.train_chunk_slices = k                                          # it may be changed between steps
            _assert_same_bits(_step(model, src, tgt), plain)


# ---- 3: the 16-bit modes ----------------------------------------------------------------------------------------------------------------

def _plain_s(**kw):
    return build({}, 0, "fp32", **kw).train()


def _swiglu_s2(**kw):
    """ViT-S width, two SwiGLU blocks with LayerScale (the reduced model of tests/test_swiglu_gpu.py)."""
    from test_swiglu_gpu import _model
    sd = synth.synth_state_dict("s", 11, img_size=518, layerscale=True, chunked=False, ffn_layer="swiglufused", depth=2)
    return _model(sd, 384, 2, 6, compute_dtype="fp32", **kw).train()


def _registers_s2(**kw):
    """ViT-S width, two blocks, four register tokens, LayerScale, a stored position grid of 4 x 4 patches (img_size 56)."""
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT
    with torch.device("meta"):
        m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", use_registers=True, **kw)
        m.encoder = _ViT(384, 2, 6, img_size=56, num_register_tokens=4, layerscale=1.0, chunked=False)
    m = m.to_empty(device="cuda")
    m.load_state_dict(synth.synth_state_dict("s", 23, img_size=56, layerscale=True, chunked=False, num_register_tokens=4, depth=2), strict=True)
    return m.train()


# name -> (builder, mode, source shape): 10 rows as 3 + 3 + 3 + 1, the second chunk across the volume boundary; 56 x 84 is an interpolated
# grid, which a register encoder does not train at -- it runs at its stored 56 x 56
CASES16 = {
    "s_fp16_stored_fp32": (_plain_s, "fp16_stored_fp32", (2, 1, 5, 56, 84)),
    "s_bf16_flash_fp32": (_plain_s, "bf16_flash_fp32", (2, 1, 5, 56, 84)),
    "s_fp16_flash_16bit": (_plain_s, "fp16_flash_16bit", (2, 1, 5, 56, 84)),
    "swiglu_s2_fp16_flash_16bit": (_swiglu_s2, "fp16_flash_16bit", (2, 1, 5, 56, 84)),
    "registers_s2_fp16_flash_16bit": (_registers_s2, "fp16_flash_16bit", (2, 1, 5, 56, 56)),
}
_FP32_STEP = {}


def _fp32_step(make, shape, src, tgt):
    key = (make.__name__, shape)
    if key not in _FP32_STEP:                                                     # one fp32 step per model and shape, shared and left unchanged
        _FP32_STEP[key] = _step(make(**FP32), src, tgt)
    return _FP32_STEP[key]


def _check_chunked_against_plain(name, chunked, plain, full, only=None):
    """e_chunk <= 2 e_plain per tensor: the rel-L2 errors of the chunked and the unchunked step of one mode, each against the fp32 step."""
    bad = []
    for k, ref in full[1].items():
        if ref is None or (only is not None and k not in only):
            continue
        e_chunk, e_plain = _rel(chunked[1][k], ref), _rel(plain[1][k], ref)
        print(f"{name} {k}: chunked vs fp32 {e_chunk:.3e}, plain vs fp32 {e_plain:.3e}, ratio {e_chunk / max(e_plain, 1e-300):.2f}")
        if not e_chunk <= 2 * e_plain:
            bad.append((k, e_chunk, e_plain))
    print(f"{name} logits: chunked vs fp32 {float((chunked[0] - full[0]).abs().max()):.3e}, plain vs fp32 {float((plain[0] - full[0]).abs().max()):.3e}")
    assert not bad, bad


@pytest.mark.parametrize("case", list(CASES16))
def test_chunked_16bit_steps_are_as_close_to_the_fp32_step_as_the_plain_ones(case):
    make, mode, shape = CASES16[case]
    src, tgt = synth.synth_volume(shape, 3), torch.tensor([1, 0])
    full = _fp32_step(make, shape, src, tgt)
    model = make(**MODES16[mode])
    plain = _step(model, src, tgt)
    model.train_chunk_slices = 3
    chunked = _step(model, src, tgt)
    assert set(k for k, g in chunked[1].items() if g is not None) == set(k for k, g in full[1].items() if g is not None)
    assert all(bool(torch.isfinite(g).all()) for g in chunked[1].values() if g is not None)
    _check_chunked_against_plain(case, chunked, plain, full)


# ---- 4, 5: memory -----------------------------------------------------------------------------------------------------------------------

def test_chunked_forward_keeps_no_block_state():
    """forward_train at (1, 1, 8, 224, 224), fp16 / flash / 16bit, k = 2: no "blocks", no "xL"; what is reachable from the state besides the
    volume is at most 1 % of the 12 x 40 E M bytes the plain step keeps for the blocks (embeddings, fusion state, the token constants)."""
    src = synth.synth_volume((1, 1, 8, 224, 224), 3).cuda()
    E, M = 384, 8 * 257
    m = _plain_s(train_chunk_slices=2, **MODES16["fp16_flash_16bit"])
    with torch.no_grad():
        _, sv = train.forward_train(m, src, None, False)
    torch.cuda.synchronize()
    assert "blocks" not in sv and "xL" not in sv
    assert sv["chunk"] == 2 and sv["mp"] is torch.float16 and sv["storage16"] is True
    vol = sv["vol"].numel() * sv["vol"].element_size()
    rest = _reachable_bytes(sv, {}) - vol
    print(f"chunked saved state besides the volume: {rest} B; the plain step's block state {12 * 40 * E * M} B ({rest / (12 * 40 * E * M):.4%})")
    assert 0 < rest <= 0.01 * 12 * 40 * E * M


def test_chunking_lowers_the_peak_of_a_step():
    """Peak memory of one bf16 / flash / 16bit step at (1, 1, 8, 518, 518): k = 2 below k = 0 by at least 0.75 x 12 blocks x 6 slices x
    1370 tokens x 40 E bytes -- the block-state table for the six slices no longer held."""
    src = synth.synth_volume((1, 1, 8, 518, 518), 5).cuda()
    tgt = torch.tensor([0]).cuda()
    peaks = {}
    for k in (0, 2):
        m = _plain_s(train_chunk_slices=k, train_precision="bf16", train_attention="flash", train_storage="16bit")
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        F.cross_entropy(m(src), tgt).backward()
        torch.cuda.synchronize()
        peaks[k] = torch.cuda.max_memory_allocated()
        del m
        torch.cuda.empty_cache()
    need = 0.75 * 12 * (8 - 2) * 1370 * 40 * 384
    print(f"peak GiB: k=0 {peaks[0] / 2**30:.2f}, k=2 {peaks[2] / 2**30:.2f}; saved {(peaks[0] - peaks[2]) / 1e9:.2f} GB, need {need / 1e9:.2f} GB")
    assert peaks[0] - peaks[2] >= need


# ---- 6: a frozen encoder ----------------------------------------------------------------------------------------------------------------

def _frozen(**kw):
    return build({}, 0, "fp32", freeze=True, **kw).train()


@pytest.mark.parametrize("k", [0, 2])
def test_frozen_encoder_keeps_nothing_and_changes_no_gradient(k):
    """freeze=True, head and fusion trainable, (1, 1, 4, 56, 56).  A source that needs no gradient: the state holds nothing of the blocks;
    under the deterministic flag the gradients of head and fusion are, bit for bit, those of a step whose source does require grad (that
    step goes through the encoder, so it keeps -- k = 0 -- or recomputes -- k = 2 -- the state)."""
    src, tgt = synth.synth_volume((1, 1, 4, 56, 56), 7), torch.tensor([1])
    model = _frozen(train_chunk_slices=k)
    assert not any(p.requires_grad for p in model.encoder.parameters()) and model.linear.weight.requires_grad
    with torch.no_grad():
        _, sv = train.forward_train(model, src.cuda(), None, False)
        assert "blocks" not in sv and "xL" not in sv
        held = _reachable_bytes(sv, {}) - sv["vol"].numel() * 4
        _, kept = train.forward_train(model, src.cuda().requires_grad_(), None, False)
        assert ("blocks" in kept) == (k == 0)
    state = 12 * 66 * 384 * 4 * 17                                               # the fp32 block-state table at 4 slices of 17 tokens
    print(f"frozen encoder, k={k}: {held} B reachable besides the volume; the block state would be {state} B")
    assert held < 0.5 * state
    with _deterministic():
        without = _step(model, src, tgt, want_src=False)
        with_src = _step(model, src, tgt, want_src=True)
    assert without[1][P.SOURCE] is None and with_src[1][P.SOURCE] is not None
    trained = [n for n, g in without[1].items() if g is not None]
    assert trained and not any(n.startswith("encoder.") for n in trained) and "linear.weight" in trained
    assert any(n.startswith("slice_fusion.") for n in trained)
    assert torch.equal(without[0], with_src[0])
    for n, p in model.named_parameters():
        g, h = without[1][n], with_src[1][n]
        assert (g is None and h is None) or torch.equal(g, h), n


def test_frozen_encoder_chunked_source_gradient():
    """freeze=True, k = 2, a source that requires grad, fp16 / flash / 16bit: d source against the fp32 step's is at most twice as far as
    the unchunked step's (check 3's comparison)."""
    shape = (1, 1, 4, 56, 56)
    src, tgt = synth.synth_volume(shape, 7), torch.tensor([1])
    full = _step(_frozen(**FP32), src, tgt)
    model = _frozen(**MODES16["fp16_flash_16bit"])
    plain = _step(model, src, tgt)
    model.train_chunk_slices = 2
    chunked = _step(model, src, tgt)
    assert chunked[1][P.SOURCE].shape == src.shape and bool(torch.isfinite(chunked[1][P.SOURCE]).all())
    assert all(g is None for n, g in chunked[1].items() if n.startswith("encoder."))
    _check_chunked_against_plain("frozen", chunked, plain, full, only={P.SOURCE})


# ---- 7: slice sharding ------------------------------------------------------------------------------------------------------------------

SHARD_SHAPES = {"shards_3_2": (1, 1, 5, 56, 56), "empty_shard": (1, 1, 1, 56, 56)}   # D = 5 over 2 ranks: 3 + 2 slices; D = 1: rank 1 owns nothing


def _shard_worker(rank, world, port, ret):
    try:
        _shard_cases(rank, world, port, ret)
    except BaseException:
        ret[rank] = {"error": traceback.format_exc()}
        raise


def _shard_cases(rank, world, port, ret):
    import os
    import sys
    import torch.distributed as dist
    from conftest import ROOT
    import test_shard_train_gpu as S
    sys.path.insert(0, str(ROOT / "tools"))
    from rehearsal import HostStagedSharding              # both ranks share cuda:0: RCCL refuses duplicate devices
    from mst.models import DinoV2ClassifierSlice
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    res = {}

    def make(shard, **kw):
        m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, **kw)
        m.load_state_dict(synth.synth_state_dict("s", 0), strict=True)
        m = m.cuda().train()
        return m.enable_slice_sharding(sharding=HostStagedSharding()) if shard else m

    def step(model, src):
        logits, grads, dsrc = S._step(model, src.cuda(), None, torch.tensor([1]), want_src=True)
        return logits, grads, dsrc

    torch.use_deterministic_algorithms(True)
    for name, shape in SHARD_SHAPES.items():
        src = synth.synth_volume(shape, 3)
        r = res[name] = {}
        # the fp32 step: chunked and sharded against unsharded and unchunked, test_shard_train_gpu's `_worst` at its bar (1e-4 of max |ref|)
        logits0, grads0, dsrc0 = step(make(False, **FP32), src)
        model = make(True, train_chunk_slices=2, **FP32)
        d0, d1, _ = model._sharding.shard_range(shape[2])
        r["slices"] = d1 - d0
        logits, grads, dsrc = step(model, src)
        ref = {k: v.cpu().double() for k, v in grads0.items()}
        ref[S.SOURCE] = dsrc0.cpu().double()
        r["names_equal"] = set(grads) == set(grads0)
        r["logits_err"] = float((logits - logits0).abs().max())
        r["worst"], r["where"], r["bad"] = S._worst({**grads, S.SOURCE: dsrc}, ref)
        r["ranks_equal"] = S._same_on_all_ranks([logits, dsrc] + [grads[k] for k in sorted(grads)])
        logits2, grads2, dsrc2 = step(model, src)
        r["deterministic"] = bool(torch.equal(logits, logits2)) and S._bit_equal(grads, grads2) and bool(torch.equal(dsrc, dsrc2))
        with torch.no_grad():
            _, sv = train.forward_train(model, src.cuda(), None, False)
            r["no_block_state"] = "blocks" not in sv and "xL" not in sv
            del sv
        # fp16 / flash / 16bit: against the unsharded unchunked fp32 step, `_compare` and its bars, and the unsharded unchunked step of the mode
        mode16 = MODES16["fp16_flash_16bit"]
        full = (logits0, grads0)
        l16, g16, _ = step(make(True, train_chunk_slices=2, **mode16), src)
        p16, q16, _ = step(make(False, **mode16), src)
        r["mode16_sharded_chunked"] = S._compare((l16, g16), full)
        r["mode16_plain"] = S._compare((p16, q16), full)
    torch.cuda.synchronize()
    ret[rank] = res
    dist.destroy_process_group()


def test_chunked_step_under_slice_sharding_two_ranks_one_gpu():
    """Two ranks rehearsed on one GPU (gloo + tools/rehearsal.py, as tests/test_shard_train_gpu.py), k = 2, deterministic flag on.
    (1, 1, 5, 56, 56): rank 0 walks its 3 slices as 2 + 1, rank 1 its 2 as one chunk; (1, 1, 1, 56, 56): rank 1 owns nothing.  The fp32 step
    against the unsharded unchunked fp32 step within 1e-4 of max |ref| per tensor (d source included) and logits within 1e-4; fp16 / flash /
    16bit against that fp32 step within 1e-2 / 1e-2 / 8e-3 (logits, worst parameter, global) and at most 2x the unsharded unchunked step of
    the same mode; both ranks hold the same bits; a second step gives the same bits; no block state between forward and backward."""
    import torch.multiprocessing as mp
    from test_shard_train_gpu import _free_port
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + 300
    for p in procs:                                      # a worker that died ends the wait for its peer at once
        while p.is_alive() and time.monotonic() < deadline and all(q.exitcode in (None, 0) for q in procs):
            p.join(0.5)
    hung = [r for r, p in enumerate(procs) if p.is_alive()]
    for p in procs:
        if p.is_alive():
            p.terminate()
    for r in range(2):
        if "error" in ret.get(r, {}):
            print(f"rank {r} failed:\n{ret[r]['error']}")
    assert [p.exitcode for p in procs] == [0, 0] and not hung, f"exit codes {[p.exitcode for p in procs]}, still running at the limit: {hung}"
    for rank in range(2):
        for name in SHARD_SHAPES:
            print(f"rank {rank} {name}: " + ", ".join(f"{k}={v}" for k, v in ret[rank][name].items()))
    for rank in range(2):
        for name in SHARD_SHAPES:
            r = ret[rank][name]
            assert r["slices"] == {"shards_3_2": 3 - rank, "empty_shard": 1 - rank}[name]
            assert r["names_equal"] and r["logits_err"] < 1e-4 and not r["bad"], (rank, name, r["logits_err"], r["bad"])
            assert r["ranks_equal"] and r["deterministic"] and r["no_block_state"], (rank, name, r)
            d, w, g = r["mode16_sharded_chunked"]
            dp, wp, gp = r["mode16_plain"]
            assert d < 1e-2 and w < 1e-2 and g < 8e-3, (rank, name, d, w, g)
            assert d <= 2 * dp and w <= 2 * wp and g <= 2 * gp, (rank, name, (d, dp), (w, wp), (g, gp))
