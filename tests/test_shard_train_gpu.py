"""The HIP training step under slice sharding (mst/train.py, mst/parallel.py): a volume's slices over two ranks.

ONE pair of worker processes shares cuda:0 (gloo + tools/rehearsal.py::HostStagedSharding, because RCCL refuses two ranks on one device)
and runs every case, since starting the processes is what costs; each worker reports plain numbers and flags, the test asserts on them.
No step has run on more than one GPU: what is checked here is the scheme and its collectives, not a speed-up.

References: float64 torch.autograd through the CPU oracle at the project's bar for the fp32 step (1e-4 * max|ref| per parameter and for
d source, logits within 1e-4: tests/train_parity.py derives it), the unsharded fp32 step at the bars of
tests/test_train_storage_gpu.py::STEP_CASES for the 16-bit modes (1e-2 per parameter and logits, 8e-3 global; at most 2x the unsharded
same-mode step's error).

Measured on the MI355X (MEASURED below; both ranks report the same digits).  Gradients and logits are bit-equal across the two ranks with
the atomic reductions as well as the ordered ones at these shapes; only the ordered ones (torch.use_deterministic_algorithms) promise it.
"""
import socket
import time
import traceback

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from mst import synth

pytestmark = pytest.mark.gpu

BAR = 1e-4
SOURCE = "<source>"
# name -> the golden that fixes seed / shape / mask, or (seed, shape)
SHAPES = {
    "b2_mask": "b2_mask",                                # 2 x 6 x 112 x 140 with a key-padding mask: 3 + 3 slices
    "uneven_2_1": (31, (1, 1, 3, 84, 84)),               # D = 3 over 2 ranks: 2 + 1 slices, one padded row in each collective
    "empty_shard": (37, (1, 1, 1, 28, 28)),              # D = 1 over 2 ranks: rank 1 owns nothing; rank 0 runs 5 token rows
}
MEASURED = {
    # fp32 step against the float64 oracle: max |d logits|, worst parameter (atomic / ordered reductions), d source -- bar 1e-4
    "b2_mask": (4.1e-6, 1.18e-5, 1.18e-5, 9.6e-6), "uneven_2_1": (5.3e-6, 1.48e-5, 1.48e-5, 1.22e-5), "empty_shard": (1.3e-6, 6.6e-6, 6.6e-6, 3.1e-6),
    # fp16 / flash / 16bit at 1 x 4 x 224 x 224 against the unsharded fp32 step: logits, worst parameter, global rel-L2 -- sharded, then the
    # unsharded step of the same mode (ratios 1.00 1.00 1.00: the shard runs the same kernels on half the rows)
    "mode16": ((1.25e-3, 5.512e-3, 3.920e-3), (1.25e-3, 5.512e-3, 3.920e-3)),
}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _inputs(name):
    spec = SHAPES[name]
    if isinstance(spec, str):
        g = load_golden(spec)
        seed, shape = int(g["seed"]), tuple(int(v) for v in g["shape"])
        mask = torch.from_numpy(g["src_key_padding_mask"]) if "src_key_padding_mask" in g else None
    else:
        (seed, shape), mask = spec, None
    return seed, synth.synth_volume(shape, seed + 100), mask, torch.arange(shape[0]) % 2


def _oracle(seed, src, mask, target):
    """float64 autograd through the CPU oracle: (logits, {parameter: gradient or None, SOURCE: d source})."""
    from oracle import mst_oracle as O
    sd = {k: (v.double().requires_grad_() if v.is_floating_point() else v.clone()) for k, v in synth.synth_state_dict("s", seed).items()}
    x = src.double().requires_grad_()
    logits = O.forward(sd, x, src_key_padding_mask=mask)["logits"]
    F.cross_entropy(logits, target).backward()
    grads = {k: v.grad for k, v in sd.items() if v.is_floating_point()}
    grads[SOURCE] = x.grad
    return logits.detach(), grads


def _worst(got, ref):
    """(worst max|got - ref| / max|ref| over the entries the reference has a gradient for, its name, names above BAR * max|ref| + 1e-9)."""
    worst, where, bad = 0.0, None, []
    for k, r in ref.items():
        g = got.get(k)
        if r is None:
            if g is not None and bool(g.any()):
                bad.append(k + " (a gradient where the reference has none)")
            continue
        if g is None or g.shape != r.shape:
            bad.append(k + " (missing)")
            continue
        scale = float(r.abs().max())
        err = float((g.detach().cpu().double() - r).abs().max())
        if err > BAR * scale + 1e-9:
            bad.append(f"{k} {err / scale:.2e}")
        if err / max(scale, 1e-300) > worst:
            worst, where = err / max(scale, 1e-300), k
    return worst, where, bad


def _same_on_all_ranks(tensors):
    """True on every rank iff rank 0's bits of these tensors are every rank's (host broadcast over gloo)."""
    import torch.distributed as dist
    mine = torch.cat([t.detach().reshape(-1).float().cpu() for t in tensors])
    ref = mine.clone()
    dist.broadcast(ref, 0)
    ok = torch.tensor([1 if torch.equal(ref.view(torch.int32), mine.view(torch.int32)) else 0])
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    return bool(ok.item())


def _step(model, src, mask, target, want_src=False):
    """One step: (logits, {parameter name: gradient (absent if none)}, d source or None)."""
    model.zero_grad(set_to_none=True)
    x = src.clone().requires_grad_() if want_src else src
    logits = model(x, src_key_padding_mask=mask)
    F.cross_entropy(logits, target.to(logits.device)).backward()
    return logits.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, (x.grad if want_src else None)


def _bit_equal(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def _reachable_bytes(obj, seen):
    if torch.is_tensor(obj):
        if obj.is_cuda and obj.data_ptr() not in seen:
            seen[obj.data_ptr()] = obj.numel() * obj.element_size()
    elif isinstance(obj, dict):
        for v in obj.values():
            _reachable_bytes(v, seen)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _reachable_bytes(v, seen)
    return sum(seen.values())


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _compare(a, b):
    """(max |d logits|, worst per-parameter rel-L2, global rel-L2) of step a against step b, as tests/test_attn_train_gpu.py::_compare."""
    (la, ga), (lb, gb) = a, b
    assert set(ga) == set(gb)
    worst = max(_rel(ga[k], gb[k]) for k in gb)
    glob = (sum(float((ga[k] - gb[k]).double().square().sum()) for k in gb) / sum(float(gb[k].double().square().sum()) for k in gb)) ** 0.5
    return float((la - lb).abs().max()), worst, glob


def _worker(rank, world, port, ret):
    try:
        _run_cases(rank, world, port, ret)
    except BaseException:
        ret[rank] = {"error": traceback.format_exc()}
        raise


def _run_cases(rank, world, port, ret):
    import os
    import sys
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    from conftest import ROOT
    sys.path.insert(0, str(ROOT / "tools"))
    from rehearsal import HostStagedSharding              # both ranks share cuda:0: RCCL refuses duplicate devices
    from mst import train
    from mst.models import DinoV2ClassifierSlice
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    res = {}

    def build(seed, shard=True, **kw):
        m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, **kw)
        m.load_state_dict(synth.synth_state_dict("s", seed), strict=True)
        m = m.cuda().train()
        return m.enable_slice_sharding(sharding=HostStagedSharding()) if shard else m

    # ---- 1 (fp32 step), 2 (source gradient, pruning, frozen model), 4 (determinism), 5 (saved state) per shape
    kept = {}
    for name in SHAPES:
        seed, src, mask, target = _inputs(name)
        D = src.shape[1] * src.shape[2]
        ref_logits, ref = _oracle(seed, src, mask, target)
        ref_params = {k: v for k, v in ref.items() if k != SOURCE}
        model = build(seed)
        r = res[name] = {}
        for flag in (False, True):                       # the atomic reductions, then the ordered ones (torch.use_deterministic_algorithms)
            torch.use_deterministic_algorithms(flag)
            tag = "ordered" if flag else "atomic"
            logits, grads, _ = _step(model, src, mask, target)
            r[tag + "_logits_err"] = float((logits.cpu().double() - ref_logits).abs().max())
            r[tag + "_logits_equal"] = _same_on_all_ranks([logits])
            r[tag + "_worst"], r[tag + "_where"], r[tag + "_bad"] = _worst(grads, ref_params)
            names = sorted(grads)
            r[tag + "_grads_equal"] = _same_on_all_ranks([grads[k] for k in names])
            r[tag + "_unequal"] = [k for k in names if not _same_on_all_ranks([grads[k]])] if not r[tag + "_grads_equal"] else []
        # flag on from here.  4: a second step gives the same bits
        logits2, grads2, _ = _step(model, src, mask, target)
        r["deterministic"] = bool(torch.equal(logits, logits2)) and _bit_equal(grads, grads2)
        # 2: asking for d source changes no parameter gradient, and every rank holds the whole d source
        logits3, grads3, dsrc = _step(model, src, mask, target, want_src=True)
        r["src_pruning_equal"] = bool(torch.equal(logits, logits3)) and _bit_equal(grads, grads3)
        r["src_shape_ok"] = dsrc is not None and dsrc.shape == src.shape and dsrc.dtype == src.dtype and dsrc.device == src.device
        r["src_worst"], _, r["src_bad"] = _worst({SOURCE: dsrc}, {SOURCE: ref[SOURCE]})
        r["src_equal"] = _same_on_all_ranks([dsrc])
        model.zero_grad(set_to_none=True)
        model.requires_grad_(False)                      # a frozen model: the source-only route of models/dino.py under sharding
        x = src.clone().requires_grad_()
        out = model(x, src_key_padding_mask=mask)
        r["frozen_has_grad_fn"] = out.grad_fn is not None
        F.cross_entropy(out, target.cuda()).backward()
        r["frozen_no_param_grad"] = all(p.grad is None for p in model.parameters())
        r["frozen_src_worst"], _, r["frozen_src_bad"] = _worst({SOURCE: x.grad}, {SOURCE: ref[SOURCE]})
        r["frozen_src_equal"] = _same_on_all_ranks([x.grad])
        model.requires_grad_(True)
        # 5: what a rank keeps for the blocks is what an unsharded step over its slices alone keeps
        d0, d1, dpad = model._sharding.shard_range(D)
        with torch.no_grad():
            _, sv = train.forward_train(model, src, mask, False)
            r["shard_recorded"] = sv["shard"] == (d0, d1, dpad)
            r["saved_bytes"] = _reachable_bytes(sv.get("blocks", []), {})
            del sv
            r["saved_bytes_own_slices"] = 0
            if d1 > d0:
                _, sv = train.forward_train(build(seed, shard=False), src[:, :, d0:d1], None if mask is None else mask[:, d0:d1], False)
                r["saved_bytes_own_slices"] = _reachable_bytes(sv["blocks"], {})
                del sv
        r["slices"] = d1 - d0
        if name == "b2_mask":
            kept = dict(seed=seed, src=src, mask=mask, target=target, grads=grads, logits=logits)
        with pytest.raises(NotImplementedError, match="save_attn"):      # unchanged: no attention read-outs inside a gradient forward
            model(src, src_key_padding_mask=mask, save_attn=True)
        del model

    # ---- 6: the same sharded model under DDP over the two ranks (flag still on): a group's ranks hold identical gradients after the sum,
    # DDP's mean leaves them as they are
    model = build(kept["seed"])
    ddp = DDP(model, find_unused_parameters=True)
    F.cross_entropy(ddp(kept["src"], src_key_padding_mask=kept["mask"]), kept["target"].cuda()).backward()
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None and (k in kept["grads"] or bool(p.grad.any()))}
    res["ddp_equal"] = _bit_equal(got, kept["grads"])
    res["ddp_unequal"] = sorted(k for k in set(got) | set(kept["grads"]) if k not in got or k not in kept["grads"] or not torch.equal(got[k], kept["grads"][k]))[:8]
    del ddp, model, got, kept
    torch.use_deterministic_algorithms(False)

    # ---- 3: the 16-bit modes at 1 x 4 x 224 x 224 (two slices per rank) against the unsharded fp32 step
    src = synth.synth_volume((1, 1, 4, 224, 224), 3).cuda()
    tgt = torch.tensor([1])
    mode16 = dict(train_precision="fp16", train_attention="flash", train_storage="16bit")

    def grads_of(shard, **kw):
        logits, grads, _ = _step(build(0, shard=shard, **kw), src, None, tgt)
        return logits, grads
    full = grads_of(False, train_precision="fp32", train_attention="stored")
    res["mode16_sharded"] = _compare(grads_of(True, **mode16), full)
    res["mode16_unsharded"] = _compare(grads_of(False, **mode16), full)
    # 5 again, in the leanest mode: 40 E bytes per token of this rank's two slices
    with torch.no_grad():
        _, sv = train.forward_train(build(0, **mode16), src, None, False)
        d0, d1, _ = sv["shard"]
        res["mode16_saved_bytes"] = _reachable_bytes(sv["blocks"], {})
        del sv
        _, sv = train.forward_train(build(0, shard=False, **mode16), src[:, :, d0:d1], None, False)
        res["mode16_saved_bytes_own_slices"] = _reachable_bytes(sv["blocks"], {})
        del sv
    torch.cuda.synchronize()
    ret[rank] = res
    dist.destroy_process_group()


def test_sharded_training_step_two_ranks_one_gpu():
    """Cases 1-6 of the sharded step (module docstring); figures are printed before they are asserted."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + 300
    for p in procs:                                      # 300 s for the pair; a worker that died ends the wait for its peer at once
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
        res = ret[rank]
        for name in SHAPES:
            r = res[name]
            print(f"rank {rank} {name} ({r['slices']} slices): " + ", ".join(f"{k}={v}" for k, v in r.items() if k != "slices"))
        print(f"rank {rank}: 16-bit sharded vs fp32 (logits, worst, global) {res['mode16_sharded']}, unsharded {res['mode16_unsharded']}; "
              f"saved bytes {res['mode16_saved_bytes']} / own slices unsharded {res['mode16_saved_bytes_own_slices']}; ddp {res['ddp_equal']} {res['ddp_unequal']}")
    for rank in range(2):
        res = ret[rank]
        for name in SHAPES:
            r = res[name]
            assert r["slices"] == {"b2_mask": 3, "uneven_2_1": 2 - rank, "empty_shard": 1 - rank}[name]
            for tag in ("atomic", "ordered"):            # 1
                assert r[tag + "_logits_equal"] and r[tag + "_logits_err"] < 1e-4, (rank, name, tag, r[tag + "_logits_err"])
                assert not r[tag + "_bad"], (rank, name, tag, r[tag + "_bad"])
                assert r[tag + "_grads_equal"], (rank, name, tag, r[tag + "_unequal"])
            assert r["src_shape_ok"] and r["src_equal"] and not r["src_bad"], (rank, name, r["src_bad"])              # 2
            assert r["src_pruning_equal"], (rank, name)
            assert r["frozen_has_grad_fn"] and r["frozen_no_param_grad"] and r["frozen_src_equal"] and not r["frozen_src_bad"], (rank, name, r)
            assert r["deterministic"], (rank, name)                                                                   # 4
            assert r["shard_recorded"] and r["saved_bytes"] == r["saved_bytes_own_slices"], (rank, name, r)           # 5
            assert (r["saved_bytes"] > 0) == (r["slices"] > 0)
        d, w, g = res["mode16_sharded"]                                                                               # 3
        dp, wp, gp = res["mode16_unsharded"]
        assert d < 1e-2 and w < 1e-2 and g < 8e-3, (d, w, g)
        assert d <= 2 * dp and w <= 2 * wp and g <= 2 * gp, ((d, dp), (w, wp), (g, gp))
        assert res["mode16_saved_bytes"] == res["mode16_saved_bytes_own_slices"] > 0
        assert res["ddp_equal"], (rank, res["ddp_unequal"])                                                           # 6


def _rccl_worker(port, ret):
    import os
    import torch.distributed as dist
    from mst.parallel import SliceSharding
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")   # dmabuf IPC, as tests/test_model_gpu.py
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)                 # backend "nccl" IS RCCL on ROCm
    flat = torch.arange(-500, 531, dtype=torch.float32, device="cuda") / 8
    want = flat.clone()
    out = SliceSharding().all_reduce_sum(flat)
    torch.cuda.synchronize()
    ret[0] = {"backend": dist.get_backend(), "in_place": out.data_ptr() == flat.data_ptr(), "equal": bool(torch.equal(out, want))}
    dist.destroy_process_group()


def test_all_reduce_sum_over_rccl_world_size_one():
    """The product transport of the bucket: `dist.all_reduce` on a DEVICE tensor over backend "nccl" (= RCCL).  One GPU cannot hold two RCCL
    ranks, and a sharding of world size 1 is never consulted by the training step, so this is the only place that call executes."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), ret))
    p.start()
    p.join(300)
    if p.is_alive():
        p.terminate()
        pytest.fail("the worker was still running after 300 s")
    assert p.exitcode == 0
    assert ret[0] == {"backend": "nccl", "in_place": True, "equal": True}, ret[0]
