"""mst/models/prepared.py on CPU tensors (they have ``data_ptr`` and ``_version`` like device tensors): the weight-version key, the
holder of the images built under it, the binding of either model file's slice transformer into ``mst_fusion_weights``, and the
workspace cache with what a captured graph keeps of it."""
import ctypes as C
import weakref

import pytest
import torch

from mst import hip
from mst.models.prepared import Prepared, bind_slice_fusion, cached_workspace, pin_workspaces, version_key

FORMS = pytest.mark.parametrize("full", [True, False], ids=["pairs", "folded"])


def _weak_sum(tensors):
    """The key ResNet used before it shared version_key: versions plus the low 16 pointer bits, summed."""
    return sum(t._version + (t.data_ptr() & 0xFFFF) for t in tensors)


def _tensors():
    return [torch.zeros(8), torch.ones(3, 5), torch.zeros(4, dtype=torch.long)]      # two "parameters", a "buffer"


@FORMS
def test_key_is_stable_and_changes_with_an_edit_of_any_one_tensor(full):
    ts = _tensors()
    assert version_key(ts, full) == version_key(ts, full)
    for t in ts:
        before = version_key(ts, full)
        t.add_(1)
        assert version_key(ts, full) != before
        assert version_key(ts, full) == version_key(ts, full)


@FORMS
def test_key_tells_which_tensor_was_edited(full):
    """The same addresses and the same multiset of versions, on different tensors.  ``.data`` shares the storage under a version
    counter of its own, so both lists exist at once."""
    a, b = torch.zeros(4), torch.zeros(4)
    a2, b2 = a.data, b.data
    a.add_(1)
    b2.add_(1)
    assert [t.data_ptr() for t in (a, b)] == [t.data_ptr() for t in (a2, b2)]
    assert (a._version, b._version, a2._version, b2._version) == (1, 0, 0, 1)
    assert _weak_sum([a, b]) == _weak_sum([a2, b2])
    assert version_key([a, b], full) != version_key([a2, b2], full)


@FORMS
def test_key_keeps_every_pointer_bit(full):
    buf = torch.zeros(16384 + 4)
    lo, hi = buf[0:4], buf[16384:16388]
    assert hi.data_ptr() - lo.data_ptr() == 65536 and lo._version == hi._version
    assert _weak_sum([lo]) == _weak_sum([hi])
    assert version_key([lo], full) != version_key([hi], full)


class _Module(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(8))
        self.b = torch.nn.Parameter(torch.ones(3, 5))
        self.register_buffer("c", torch.zeros(4, dtype=torch.long))


@FORMS
def test_holder_key_follows_a_replaced_tensor_after_invalidate(full):
    mod = _Module()
    held = Prepared()
    before = held.key(mod, full, "extra")
    assert before == ("extra",) + version_key([mod.a, mod.b, mod.c], full)          # parameters, then buffers
    assert held.key(mod, full, "extra") == before and held.key(mod, full, "other") != before
    old, swapped = mod.b, torch.nn.Parameter(torch.ones(3, 5))
    assert swapped._version == old._version and swapped.data_ptr() != old.data_ptr()
    mod.b = swapped
    assert held.key(mod, full, "extra") == before                # the list is cached until invalidated
    held.invalidate()
    assert held.key(mod, full, "extra") != before


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "no_grad"])
def test_holder_builds_once_per_version_and_keeps_named_values_apart(grad):
    mod = _Module()
    held = Prepared()
    built = []

    def build(name):
        built.append(name)
        return object()

    with torch.set_grad_enabled(grad):
        first = held.get(mod, "a", lambda: build("a"), "x")
        assert held.get(mod, "a", lambda: build("a"), "x") is first and built == ["a"]
        other = held.get(mod, "b", lambda: build("b"))
        assert held.get(mod, "a", lambda: build("a"), "x") is first and held.get(mod, "b", lambda: build("b")) is other and built == ["a", "b"]
        with torch.set_grad_enabled(not grad):              # the other form of the key was stored with the value
            assert held.get(mod, "a", lambda: build("a"), "x") is first
        assert held.get(mod, "a", lambda: build("a"), "y") is not first and built == ["a", "b", "a"]     # another extra part
        mod.c.add_(1)                                       # an in-place edit of the buffer
        second = held.get(mod, "a", lambda: build("a"), "y")
        assert held.get(mod, "a", lambda: build("a"), "y") is second and built == ["a", "b", "a", "a"]
        with torch.no_grad():
            mod.a.add_(1)                                   # ... and of a parameter
        third = held.get(mod, "a", lambda: build("a"), "y")
        assert third is not second and built == ["a", "b", "a", "a", "a"]
        held.invalidate()
        assert held.get(mod, "a", lambda: build("a"), "y") is not third and built == ["a", "b", "a", "a", "a", "a"]


OWNED = ("cls_token", "ln1_w", "ln1_b", "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "ln2_w", "ln2_b",
         "lin1_w", "lin1_b", "lin2_w", "lin2_b", "norm_w", "norm_b")


def _slice_fusion(which):
    if which == "dino":
        from mst.models.dino import _SliceFusion
        return _SliceFusion(24, None), 24
    from mst.models.resnet import _SliceFusion
    return _SliceFusion(32), 32


@pytest.mark.parametrize("which", ["dino", "resnet"])
def test_bind_slice_fusion_points_every_owned_field_at_its_tensor(which):
    torch.manual_seed(0)
    sf, E = _slice_fusion(which)
    for p in sf.parameters():
        torch.nn.init.normal_(p)
    cls_token = torch.nn.Parameter(torch.randn(1, 1, E))
    lay = sf.layers[0]
    want = dict(zip(OWNED, (cls_token, lay.norm1.weight, lay.norm1.bias, lay.self_attn.in_proj_weight, lay.self_attn.in_proj_bias,
                            lay.self_attn.out_proj.weight, lay.self_attn.out_proj.bias, lay.norm2.weight, lay.norm2.bias,
                            lay.linear1.weight, lay.linear1.bias, lay.linear2.weight, lay.linear2.bias, sf.norm.weight, sf.norm.bias)))
    assert len({float(t.detach().flatten()[0]) for t in want.values()}) == len(OWNED)
    fw, kept = hip.FusionWeights(), []
    bind_slice_fusion(fw, sf, cls_token, lambda t: kept.append(t.detach()) or kept[-1])
    assert len(kept) == len(OWNED)
    for name, _ in hip.FusionWeights._fields_:
        value = getattr(fw, name)
        if name in want:
            assert value == want[name].data_ptr(), name
            assert C.cast(value, C.POINTER(C.c_float))[0] == float(want[name].detach().flatten()[0]), name
        else:
            assert not value, name                          # NULL or 0: sizes, bottleneck, position table, rotary tables and head are the model's


def test_cached_workspace_keeps_a_large_enough_tensor_and_replaces_a_smaller_one():
    cache, cpu = {}, torch.device("cpu")
    a = cached_workspace(cache, "vit", 100, cpu)
    assert a.dtype == torch.uint8 and a.numel() == 100 and cache["vit"] is a
    assert cached_workspace(cache, "vit", 100, cpu) is a and cached_workspace(cache, "vit", 7, cpu) is a     # same size, smaller: kept
    b = cached_workspace(cache, "vit", 101, cpu)                                                            # one byte more: replaced
    assert b is not a and b.numel() == 101 and cache["vit"] is b
    assert cached_workspace(cache, "fusion", 0, cpu).numel() == 0 and set(cache) == {"vit", "fusion"}       # names are independent
    assert cache["vit"] is b


def test_a_graph_entry_owns_the_workspaces_of_its_capture():
    """pin_workspaces: the entry of a captured graph (a stand-in dict here) holds every workspace tensor that was live at its capture,
    so growth replaces the cache's tensor and leaves the entry's allocated -- for as long as the entry, not longer."""
    cache, cpu = {}, torch.device("cpu")
    vit, fusion = cached_workspace(cache, "vit", 64, cpu), cached_workspace(cache, "fusion", 16, cpu)
    vit.fill_(0xA5)
    ent = {"graph": object(), "calls": 3}
    assert pin_workspaces(ent, cache) is ent
    assert ent["ws"] == {"vit": vit, "fusion": fusion} and ent["ws"] is not cache
    alive, where = weakref.ref(vit), vit.data_ptr()
    del vit
    grown = cached_workspace(cache, "vit", 128, cpu)                     # a larger shape arrives
    assert cache["vit"] is grown and ent["ws"]["vit"] is not grown
    assert alive() is not None and alive().data_ptr() == where and alive().numel() == 64 and bool((alive() == 0xA5).all())
    assert ent["ws"]["fusion"] is cache["fusion"]                        # what did not grow is shared, not copied
    later = pin_workspaces({"graph": object()}, cache)                   # a graph captured after the growth pins the new tensor
    assert later["ws"]["vit"] is grown
    del ent                                                              # the graph goes (invalidate()): so does its workspace
    assert alive() is None
