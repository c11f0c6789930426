"""train_chunk_slices (env MST_TRAIN_CHUNK_SLICES) of DinoV2ClassifierSlice: parsing, validation at construction and again at call time, the
ResNets' lack of it, and the premise the chunked recomputation stands on -- in the float64 CPU oracle the encoder of a chunk of slices is the
encoder of all of them, row for row.  No GPU."""

import warnings

import pytest
import torch

import train_parity as P
from mst.models import DinoV2ClassifierSlice, ResNetSliceTrans
from mst.train_mode import TrainMode, check_chunk, resolve

ENV = ("MST_TRAIN_CHUNK_SLICES", "MST_TRAIN_STORAGE", "MST_TRAIN_ATTENTION", "MST_TRAIN_PRECISION", "MST_CHUNK_SLICES")


def _model(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, **kw)


def _resnet(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ResNetSliceTrans(in_ch=1, out_ch=2, pretrained=False, model=18, **kw)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def test_default_is_zero_and_resolves_to_the_three_field_mode():
    m = _model()
    assert m.train_chunk_slices == 0
    assert resolve(m) == TrainMode(mp=None, flash=False, storage16=False)
    assert resolve(m).chunk == 0
    m = _model(train_precision="bf16", train_attention="flash", train_storage="16bit")
    assert m.train_chunk_slices == 0                                               # never inferred from the other three
    assert resolve(m) == TrainMode(mp=torch.bfloat16, flash=True, storage16=True)


def test_keyword_and_environment_are_read(monkeypatch):
    assert _model(train_chunk_slices=8).train_chunk_slices == 8
    assert resolve(_model(train_chunk_slices=8)) == TrainMode(None, False, False, 8)
    monkeypatch.setenv("MST_TRAIN_CHUNK_SLICES", "16")
    m = _model()
    assert m.train_chunk_slices == 16 and isinstance(m.train_chunk_slices, int) and resolve(m).chunk == 16
    assert _model(train_chunk_slices=4).train_chunk_slices == 4                    # the keyword wins
    assert _model(train_chunk_slices=0).train_chunk_slices == 0
    monkeypatch.setenv("MST_TRAIN_CHUNK_SLICES", "many")
    with pytest.raises(ValueError, match="train_chunk_slices"):
        _model()


def test_it_is_not_the_inference_keyword(monkeypatch):
    m = _model(chunk_slices=3, train_chunk_slices=5)
    assert (m.chunk_slices, m.train_chunk_slices) == (3, 5)
    monkeypatch.setenv("MST_CHUNK_SLICES", "7")
    m = _model()
    assert (m.chunk_slices, m.train_chunk_slices) == (7, 0)
    monkeypatch.delenv("MST_CHUNK_SLICES")
    monkeypatch.setenv("MST_TRAIN_CHUNK_SLICES", "7")
    m = _model()
    assert (m.chunk_slices, m.train_chunk_slices) == (0, 7)


@pytest.mark.parametrize("bad", [-1, 1.5, "x"])
def test_bad_values_raise_at_construction_and_at_resolve(bad):
    with pytest.raises(ValueError, match="train_chunk_slices"):
        _model(train_chunk_slices=bad)
    with pytest.raises(ValueError, match="train_chunk_slices"):
        check_chunk(bad)
    m = _model(train_chunk_slices=2)
    m.train_chunk_slices = bad                                                     # changed after construction: the step checks again
    with pytest.raises(ValueError, match="train_chunk_slices"):
        resolve(m)
    m.train_chunk_slices = 3                                                       # it may be changed between steps
    assert resolve(m).chunk == 3


def test_it_combines_with_every_mode():
    for kw in (dict(), dict(train_precision="fp16"), dict(train_precision="bf16", train_attention="flash"),
               dict(train_precision="fp16", train_attention="flash", train_storage="16bit")):
        m = _model(train_chunk_slices=2, **kw)
        mode = resolve(m)
        assert mode.chunk == 2 and mode[:3] == resolve(_model(**kw))[:3]


def test_the_value_is_a_hyper_parameter_like_train_storage():
    m = _model(train_precision="bf16", train_attention="flash", train_storage="16bit", train_chunk_slices=8)
    assert m.hparams["train_storage"] == "16bit"
    assert m.hparams["train_chunk_slices"] == 8
    assert _model().hparams["train_chunk_slices"] == 0


def test_resnet_slice_trans_has_no_such_mode(monkeypatch):
    """BatchNorm's batch statistics couple the slices of a batch, so the ResNet step cannot recompute per chunk: the keyword is unknown and
    the variable does not reach the model."""
    with pytest.raises(TypeError):
        _resnet(train_chunk_slices=2)
    monkeypatch.setenv("MST_TRAIN_CHUNK_SLICES", "2")
    m = _resnet()
    assert not hasattr(m, "train_chunk_slices")
    assert "train_chunk_slices" not in m.hparams
    assert resolve(m) == TrainMode(mp=None, flash=False, storage16=False) and resolve(m).chunk == 0
    monkeypatch.setenv("MST_TRAIN_CHUNK_SLICES", "x")                              # not even read
    assert resolve(_resnet()).chunk == 0


@pytest.mark.parametrize("case,k", [("vitb_126tok", 4), ("grid_1x37", 1)])
def test_the_encoder_of_a_chunk_is_the_encoder_of_all_slices_in_the_float64_oracle(case, k):
    """Encode the flattened slice rows k at a time (vitb_126tok: 4 + 2 rows across the volume boundary; grid_1x37: one slice each, an
    interpolated position grid) and concatenate: embeddings and logits are those of one pass, to the last bit or within 1e-12 (float64
    values of order one: a few ulp of a batched product that blocks its rows differently).  There is no statistic across slices."""
    from oracle import mst_oracle as O
    kw, src, mask, _ = P.inputs(case)
    sd = {name: (v.double() if v.is_floating_point() else v) for name, v in P.state_dict(kw).items()}
    B, C, D, H, W = src.shape
    rows = src.double().permute(0, 2, 1, 3, 4).reshape(B * D * C, H, W)
    size = kw.get("model_size", "s")
    with torch.no_grad():
        whole, _ = O.vit_encode(sd, rows, size)
        parts = torch.cat([O.vit_encode(sd, rows[r:r + k], size)[0] for r in range(0, rows.shape[0], k)])
        fuse = dict(slice_fusion_type=kw.get("slice_fusion", "transformer"), src_key_padding_mask=mask, rotary=kw.get("rotary_positional_encoding"))
        l_whole = O.fuse(sd, whole, B, D * C, **fuse)["logits"]
        l_parts = O.fuse(sd, parts, B, D * C, **fuse)["logits"]
    assert len(range(0, rows.shape[0], k)) > 1 and parts.shape == whole.shape
    d_emb, d_logits = float((parts - whole).abs().max()), float((l_parts - l_whole).abs().max())
    print(f"{case} in chunks of {k}: max |d emb| {d_emb:.3e}, max |d logits| {d_logits:.3e}")
    assert torch.equal(parts, whole) or d_emb <= 1e-12
    assert torch.equal(l_parts, l_whole) or d_logits <= 1e-12
