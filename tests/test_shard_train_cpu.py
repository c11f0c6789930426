"""The training step under slice sharding, the parts that need no GPU: the sum collective of mst/parallel.py over gloo, and the scheme itself
(mst/train.py: a rank differentiates the encoder on its own slices only, the stage behind the all-gather is replicated, the encoder's
gradients are summed over the ranks) carried out with the CPU oracle alone in float64."""
import socket
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from mst import synth


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_values(rank, n=1031):
    """Dyadic rationals (multiples of 1/8 below 2^12) of mixed sign: every partial sum of up to 4 of them is exact in fp32, so the sum is
    the same bits in whatever order a transport adds the ranks."""
    g = torch.Generator().manual_seed(100 + rank)
    return torch.randint(-(1 << 15), 1 << 15, (n,), generator=g).float() / 8.0


def _reduce_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, str(ROOT / "new-vit_amd"))
    from mst.parallel import SliceSharding
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        sh = SliceSharding()
        flat = _rank_values(rank)
        out = sh.all_reduce_sum(flat)
        in_place = out.data_ptr() == flat.data_ptr()
        try:
            sh.all_reduce_sum(torch.zeros(2, 3))
            refused = False
        except ValueError:
            refused = True
        q.put((rank, out.clone(), in_place and refused))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_all_reduce_sum_over_gloo(world):
    """SliceSharding.all_reduce_sum: in place, exactly the locally computed sum of the ranks' buckets, the same bits on every rank."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    want = sum(_rank_values(r).double() for r in range(world)).float()
    assert [r for r, _, _ in res] == list(range(world))
    for r, got, ok in res:
        assert ok, r
        assert torch.equal(got, want), r
        assert torch.equal(got, res[0][1]), r


REPLICATED = ("bottleneck.", "slice_pos_emb.", "slice_fusion.", "cls_token", "linear.")


def test_per_shard_encoder_gradients_sum_to_the_full_gradient_in_the_oracle():
    """2 x 3 x 28 x 42 with a key-padding mask, shards (0, 2) and (2, 3).  A rank's loss is the oracle's loss with the embeddings of the
    slices it does not own detached.  The encoder's gradients of the two ranks sum to the gradient of the whole model (within
    1e-6 * max|ref|: float64 summation order only; measured 5.2e-8), and every parameter behind the all-gather gets the same gradient on
    both ranks, bit for bit (measured 0) -- which is why the training step sums the former and leaves the latter alone."""
    from oracle import mst_oracle as O
    B, D, H, W = 2, 3, 28, 42
    src = synth.synth_volume((B, 1, D, H, W), 7).double()
    mask = torch.tensor([[False, False, True], [False, False, False]])
    target = torch.tensor([1, 0])
    sd0 = synth.synth_state_dict("s", 5, use_bottleneck=True, use_slice_pos_emb=True)

    def fresh():
        return {k: (v.double().requires_grad_() if v.is_floating_point() else v.clone()) for k, v in sd0.items()}

    def grads(sd, logits):
        F.cross_entropy(logits, target).backward()
        return {k: v.grad for k, v in sd.items() if v.is_floating_point() and v.grad is not None}

    sd = fresh()
    ref = grads(sd, O.forward(sd, src, src_key_padding_mask=mask)["logits"])
    assert any(k.startswith("encoder.") for k in ref) and all(any(k.startswith(p) for k in ref) for p in REPLICATED)

    shards = [(0, 2), (2, 3)]
    per_rank = []
    for own in shards:
        sd = fresh()
        parts = []
        for d0, d1 in shards:                            # each shard's rows are encoded the same way on both ranks: identical values
            emb, _ = O.vit_encode(sd, src[:, 0, d0:d1].reshape(B * (d1 - d0), H, W))
            parts.append((emb if (d0, d1) == own else emb.detach()).view(B, d1 - d0, -1))
        emb = torch.cat(parts, dim=1).reshape(B * D, -1)
        per_rank.append(grads(sd, O.fuse(sd, emb, B, D, src_key_padding_mask=mask)["logits"]))

    worst_enc = worst_rep = 0.0
    for k, r in ref.items():
        a, b = per_rank[0][k], per_rank[1][k]
        scale = float(r.abs().max())
        if k.startswith("encoder."):
            err = float((a + b - r).abs().max())
            worst_enc = max(worst_enc, err / scale)
            assert err <= 1e-6 * scale, (k, err, scale)
        else:
            assert k.startswith(REPLICATED), k
            worst_rep = max(worst_rep, float((a - b).abs().max()))
            assert torch.equal(a, b), k
            assert float((a - r).abs().max()) <= 1e-6 * scale, k
    print(f"per-shard encoder gradients vs the full gradient: worst {worst_enc:.2e} of max|ref|; replicated parameters across shards: {worst_rep:g}")
