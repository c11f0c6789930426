"""Training step of DinoV2ClassifierSlice on the HIP path.

The reference trains through torch.autograd (mst/models/base_model.py:148-181 `_step`: ``pred = self(**batch)``, CE loss;
scripts/main_train.py:110-126 Trainer.fit).  Here ``forward`` under ``torch.enable_grad()`` returns logits that carry ONE
autograd node (`_MSTFunction`): its forward runs the model op by op through the C ABI keeping what the backward needs, its
backward produces the gradient of every parameter with the kernels of csrc/k_train.hip (`mst_gemm_ex`, `mst_layernorm_bwd`,
`mst_softmax_rows_bwd`, `mst_act_bwd`, ...).  The loss itself stays the reference's own ``torch.nn.CrossEntropyLoss`` call on the
[B, out_ch] logits (host code).  torch is used for memory only (allocation, views, concatenation / copies of whole tensors).

The mode (train_precision, train_attention, train_storage and the autocast rule) is described, validated and resolved in
mst/train_mode.py; `forward_train` resolves it once and the saved state carries it to the backward.
RoPE slice transformers, register-token encoders (at their stored position grid) and SwiGLU blocks (ffn_layer='swiglufused': x12 and h
kept, mst_swiglu_bwd between the two lin_bwd calls) train; raise: the LieRE variant, ``save_attn``
inside a training forward.

Source gradient: ``source`` is an input of the node too.  When it requires grad the backward also returns d ``source`` (source's shape,
dtype and device): the encoder's d x chain, then the patch embedding's data gradient (csrc/k_patch_dgrad.hip: the adjoint of the stride-14
convolution and of the grey -> RGB repeat, read straight from the patch rows of d x) and the inverse of the forward's channel / slice
reshape.  A frozen model (no parameter requires grad) reaches this node through models/dino.py when ``source`` requires grad.  The backward
computes only what is asked for: weight, bias, LayerScale, token and position gradients of parameters whose ``needs_input_grad`` is off are
skipped (a source-only backward is the d x chain alone), the encoder's d x chain runs if an encoder parameter or ``source`` needs it, and the
patch-embedding data gradient only for ``source``.

Determinism: while ``torch.use_deterministic_algorithms(True)`` is set (``warn_only`` too; read at every call, so it may be toggled
between steps) every floating-point reduction of the step -- bias / LayerScale / token / pos-embed column sums, the split-K weight-gradient
partials, LayerNorm d gamma / d beta, the bicubic pos-embed adjoint -- takes its fixed-order entry point (csrc/k_colsum.hip, csrc/k_ordered.hip: per-workgroup
slabs summed in ascending order, no floating-point atomics), and two steps on the same state and inputs give bit-identical logits, loss and
gradients.  Flag off: the atomic kernels, as before.  The patch embedding's data gradient has no reduction across workgroups (every pixel is
written once by one workgroup), so one entry point serves both modes.

Slice sharding (mst/parallel.py; ``enable_slice_sharding`` over more than one rank): a rank encodes only its slices [d0, d1) of every volume
(patch rows, blocks, the final LayerNorm's CLS rows), the slice embeddings are all-gathered and everything behind the encoder runs replicated
on the full [B*D, E].  The backward runs the replicated part, takes this rank's rows of d emb through its own slices and sums the gradients of
the ENCODER's parameters over the group as one flat fp32 bucket (only those asked for); bottleneck, slice_pos_emb, slice_fusion, cls_token and
linear are complete and identical on every rank and do not travel.  With a source gradient the rank's [B*dl, H, W] part is all-gathered and
every rank returns the whole d source.  Collectives, the same on every rank whatever its shard holds: forward -- the embeddings; backward -- the
bucket if an encoder parameter needs a gradient, d source if it is asked for; a frozen encoder without a source gradient returns early on every
rank.  A rank with an empty shard (fewer slices than ranks) launches no encoder kernel and contributes zeros.  EVERY RANK OF A GROUP MUST BE FED
THE SAME BATCH AND THE SAME ``dout`` (the same loss on the same targets): the replicated stage is only replicated if its inputs are.  Under DDP
over the same or a larger group the summed gradients are already identical within a sharding group, so DDP's mean leaves them as they are.

Recomputation per slice chunk (``train_chunk_slices = k > 0``, mst/train_mode.py): the whole model is one autograd node, so torch.utils.checkpoint
cannot be put around parts of it; this is the library's own form.  The encoder treats every slice alone -- LayerNorm per token, attention per
slice, no statistic across slices; only the slice transformer behind it couples them -- so encoding the flattened slice rows [B*D] k at a time
is the same function.  Forward: every chunk runs `_encoder_fwd` into a throw-away dict and only its rows of the embeddings are kept; what does
not depend on the chunk (the summed patch kernel, the prefix rows, the interpolated position grid: `_encoder_consts`) is made once.  Between
forward and backward the state holds the volume, the embeddings, the fusion and head state, the resolved mode and k: no per-block tensor.
Backward: head, fusion, slice_pos_emb and bottleneck as ever down to d emb, then per chunk in the forward's order `_encoder_fwd` again, saving, in
the mode the state carries (never resolved again: an autocast region may have ended), and `_encoder_bwd` on that chunk's rows of d emb into the
same `_Grads`, whose `put` adds every later chunk's parameter gradients to the first's (pos_embed, cls_token, register_tokens and the patch
embedding included); d source is written chunk by chunk into one [B*D, H, W] buffer.  The chunk order is fixed, so the step stays bit-reproducible
under the deterministic flag; a single chunk (k >= rows) gives the plain step's bits.  The pruning rules are unchanged.  Peak block state falls
from all slices to k; the price is one more encoder forward per step -- and every chunk issues the launches of two forwards and a backward,
which on model_size='s' makes the host the bound (measured: DESIGN.md 4b, profiles/train_chunk_slices.jsonl).  Under slice sharding each rank chunks its own rows, the collectives are
the same, an empty shard still launches nothing.  The ResNet step (mst/train_resnet.py) has no such mode: BatchNorm's batch statistics couple
the slices of a batch.

The encoder API in grad mode (``encoder_grad=True``; models/dino.py `_ViT._encode`): `encoder_forward_with_grad` is one node per call over
x [n, 3, H, W] (the RGB patch embedding and its own data / weight gradients, csrc/k_features.hip) or [n, 1, H, W] and the parameters, on
`_encoder_fwd` / `_encoder_bwd` in the resolved mode.  Its outputs are the class tokens and the streams behind the asked-for blocks (saved
block inputs: a tap keeps nothing of its own), so gradients enter `_encoder_bwd` at every token row and behind any block; the forward
stops behind the highest block asked for, the backward starts at the highest block a gradient enters behind.  train_chunk_slices and slice
sharding do not apply to these calls (all tokens of local images).

A frozen encoder keeps nothing: when no encoder parameter and not ``source`` needs a gradient (the node's needs_input_grad; `forward_train`'s
``encoder_state``), the forward drops the block state as soon as the embeddings exist, whatever k is -- the backward returns before the
encoder anyway.  Outputs and the remaining gradients are the same bits.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Set, Tuple

import torch

from . import hip, train_mode
from .train_mode import TrainMode

PATCH = 14


def _w16(lin, mp: torch.dtype) -> torch.Tensor:
    return hip.cvt16(lin.weight.detach(), mp)


def _block_fwd_16(blk, nxt, xt: torch.Tensor, xn: torch.Tensor, mode: TrainMode, n: int, N: int, heads: int, E: int):
    """One encoder block (block.py:89-114) of the 16-bit storage mode.  xt: the fp32 residual stream, xn = norm1(xt) in mode.mp (written by
    the LayerNorm that closed the previous block).  Every tensor kept is the one the next kernel reads: no fp32 copy, no second 16-bit image.
    Returns (saved state, x2 fp32, norm(x2) of the next block `nxt` in mode.mp -- None behind the last block)."""
    mp = mode.mp
    g1 = blk.ls1.gamma.detach() if hasattr(blk, "ls1") else None
    g2 = blk.ls2.gamma.detach() if hasattr(blk, "ls2") else None
    s = {"x0": xt, "x16": {}, "xn1": xn}
    s["qkv16"] = hip.gemm(xn, _w16(blk.attn.qkv, mp), blk.attn.qkv.bias.detach(), col_scale=0.125, scale_cols=E)
    s["a"], s["lse"] = hip.attention_train_fwd(s["qkv16"], n, N, heads, out_dtype=mp)
    s["br1"] = hip.gemm(s["a"], _w16(blk.attn.proj, mp), blk.attn.proj.bias.detach())
    s["x1"], s["xn2"] = hip.residual_layernorm16(xt, s["br1"], g1, blk.norm2.weight.detach(), blk.norm2.bias.detach(), 1e-6)
    if _is_swiglu(blk):                                   # SwiGLUFFNFused (swiglu_ffn.py:54-72): x12 and h where the MLP keeps hpre and hact
        s["x12"] = hip.gemm(s["xn2"], _w16(blk.mlp.w12, mp), blk.mlp.w12.bias.detach())
        s["h"] = hip.swiglu_fwd(s["x12"])
        s["br2"] = hip.gemm(s["h"], _w16(blk.mlp.w3, mp), blk.mlp.w3.bias.detach())
    else:
        s["hpre"] = hip.gemm(s["xn2"], _w16(blk.mlp.fc1, mp), blk.mlp.fc1.bias.detach())
        s["hact"] = hip.act_fwd(s["hpre"], 0)
        s["br2"] = hip.gemm(s["hact"], _w16(blk.mlp.fc2, mp), blk.mlp.fc2.bias.detach())
    x2, xn_next = hip.residual_layernorm16(s["x1"], s["br2"], g2, nxt.norm1.weight.detach() if nxt is not None else None,
                                           nxt.norm1.bias.detach() if nxt is not None else None, 1e-6)
    return s, x2, xn_next


def _block_fwd(blk, nxt, xt: torch.Tensor, xn: Optional[torch.Tensor], mode: TrainMode, n: int, N: int, heads: int, E: int):
    """The same block with fp32 storage, `_block_fwd_16`'s signature and return: every tensor kept is fp32 (but qkv16 of 'flash'), each
    16-bit product rounds its operands into images of their own, and the block runs its own norm1 -- xn is not read, xn_next is None."""
    mp = mode.mp
    s = {"x0": xt, "x16": {}}
    k16 = s["x16"] if mp is not None else None
    s["xn1"] = hip.layernorm(xt, blk.norm1.weight.detach(), blk.norm1.bias.detach(), 1e-6)
    if mode.flash:
        # q | k | v straight in the 16-bit type the attention kernels read; kept with the output and the per-row log-sum-exp instead of
        # the [n, heads, N, N] probabilities (the backward recomputes them per tile)
        s["qkv16"] = _lin_fwd(s["xn1"], blk.attn.qkv, mp, k16, out_dtype=mp, col_scale=0.125, scale_cols=E)
        s["a"], s["lse"] = hip.attention_train_fwd(s["qkv16"], n, N, heads)
    else:
        s["qkv"] = _lin_fwd(s["xn1"], blk.attn.qkv, mp, k16, col_scale=0.125, scale_cols=E)        # q * head_dim^-0.5 (attention.py:60)
        s["a"], s["P"] = _attention_fwd(s["qkv"], n, N, heads, 64, 1.0, None)
    s["br1"] = _lin_fwd(s["a"], blk.attn.proj, mp, k16)
    x1 = xt.clone()
    hip.axpby_cols(s["br1"], x1, g=blk.ls1.gamma.detach() if hasattr(blk, "ls1") else None)
    s["x1"] = x1
    s["xn2"] = hip.layernorm(x1, blk.norm2.weight.detach(), blk.norm2.bias.detach(), 1e-6)
    if _is_swiglu(blk):
        s["x12"] = _lin_fwd(s["xn2"], blk.mlp.w12, mp, k16)
        s["h"] = hip.swiglu_fwd(s["x12"])
        s["br2"] = _lin_fwd(s["h"], blk.mlp.w3, mp, k16)
    else:
        s["hpre"] = _lin_fwd(s["xn2"], blk.mlp.fc1, mp, k16)
        s["hact"] = hip.act_fwd(s["hpre"], 0)
        s["br2"] = _lin_fwd(s["hact"], blk.mlp.fc2, mp, k16)
    x2 = x1.clone()
    hip.axpby_cols(s["br2"], x2, g=blk.ls2.gamma.detach() if hasattr(blk, "ls2") else None)
    return s, x2, None


def _is_swiglu(blk) -> bool:
    return hasattr(blk.mlp, "w12")


def _lin_fwd(x: torch.Tensor, lin, mp: Optional[torch.dtype] = None, keep: Optional[dict] = None,
             out_dtype: torch.dtype = torch.float32, **kw) -> torch.Tensor:
    if mp is None:
        return hip.gemm(x, lin.weight.detach(), lin.bias.detach(), **kw)
    x16 = hip.cvt16(x, mp)
    if keep is not None and x.shape[0] <= 12288:         # the weight gradient of this product reads the same image (mst_conv_wgrad16 path)
        keep[id(lin)] = x16
    return hip.gemm(x16, hip.cvt16(lin.weight.detach(), mp), lin.bias.detach(), out_dtype=out_dtype, **kw)


class _Grads:
    def __init__(self, mp: Optional[torch.dtype] = None, needed: Optional[Set[int]] = None):
        self.by_param: Dict[int, torch.Tensor] = {}
        self.mp = mp
        self.needed = needed                             # ids of the parameters whose gradient is asked for (None: all)

    def need(self, param) -> bool:
        return param is not None and (self.needed is None or id(param) in self.needed)

    def put(self, param, g: torch.Tensor):
        if not self.need(param):
            return
        g = g.reshape(param.shape)
        if id(param) in self.by_param:
            hip.axpby_cols(g.reshape(1, -1), self.by_param[id(param)].reshape(1, -1))
        else:
            self.by_param[id(param)] = g

    def lin_bwd(self, dY: torch.Tensor, X: torch.Tensor, lin, need_dx: bool = True, X16: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """nn.Linear backward: d weight = dY^T . X, d bias = column sums of dY (each only if asked for), returns dX = dY . W."""
        M, N = dY.shape
        K = X.shape[1]
        dev = dY.device
        if self.mp is not None and N % 128 == 0 and K % 128 == 0 and M >= 64:
            return self._lin_bwd_16(dY, X, lin, need_dx, X16)
        if X.dtype != torch.float32:                     # an activation saved in 16 bits behind a product too small for the 16-bit kernels
            X = hip.cvt32(X)
        if self.need(lin.weight):
            self._dw(dY, X, lin)
        if self.need(getattr(lin, "bias", None)):
            self.put(lin.bias, hip.colsum(dY, torch.zeros(N, dtype=torch.float32, device=dev)))
        if not need_dx:
            return None
        dX = torch.empty((M, K), dtype=torch.float32, device=dev)
        hip.gemm_ex(dY, lin.weight.detach(), dX, M, K, N, sa=(N, 1), sb=(K, 1), sc=(K, 1))
        return dX

    def _dw(self, dY: torch.Tensor, X: torch.Tensor, lin):
        M, N = dY.shape
        K = X.shape[1]
        dev = dY.device
        # d weight: an [N, K] output reduced over M rows is 36-144 tiles walking thousands of rows each; split the rows into up to
        # 16 slabs (more workgroups than CUs), partial products reduced by mst_colsum
        sp = next((d for d in (16, 8, 4, 2) if M % d == 0 and M // d >= 64), 1)
        if sp > 1:
            part = torch.empty((sp, N * K), dtype=torch.float32, device=dev)
            ch = M // sp
            hip.gemm_ex(dY, X, part, N, K, ch, sa=(1, N), sb=(K, 1), sc=(K, 1), nb=(sp, 1), ba=(ch * N, 0), bb=(ch * K, 0), bc=(N * K, 0))
            dW = hip.colsum(part, torch.zeros(N * K, dtype=torch.float32, device=dev)).view(N, K)
        else:
            dW = torch.empty((N, K), dtype=torch.float32, device=dev)
            hip.gemm_ex(dY, X, dW, N, K, M, sa=(1, N), sb=(K, 1), sc=(K, 1))
        self.put(lin.weight, dW)

    def _lin_bwd_16(self, dY: torch.Tensor, X: torch.Tensor, lin, need_dx: bool, X16: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """The same three results on 16-bit MFMA operands (fp32 accumulation, fp32 results): operands are rounded into scratch images right
        before each product."""
        M, N = dY.shape
        K = X.shape[1]
        dev = dY.device
        mp = self.mp
        dY16 = hip.cvt16(dY, mp)
        want_dw = self.need(lin.weight)
        if want_dw and M <= 12288:
            # d weight = dY^T . X is the weight gradient of a 1 x 1 "convolution" over M one-pixel images: mst_conv_wgrad16 reads both operands
            # row-major (token-major) and transposes the fragments in the LDS read -- no transposed operand images, token-split partial
            # products (1 x 16 x 224^2: 14.4 -> 10.9 ms per step against the form below)
            if X.dtype == mp:
                x16 = X                                  # train_storage='16bit': the saved activation IS the operand image
            else:
                x16 = X16 if (X16 is not None and X16.dtype == mp and X16.shape == X.shape) else hip.cvt16(X, mp)   # the forward's image, if it was kept
            self.put(lin.weight, hip.conv_wgrad(dY16, x16.view(M, 1, 1, K), 1, 1, 0))
        elif want_dw:
            # many tokens: TRANSPOSED operand images (both operands contiguous along the token index) through the 128 x 128 x 64 GEMM with
            # 16-byte fragment reads, split over the tokens (mst_gemm16_splitk): 3 % faster at 16,448 tokens than the transposing reads
            tiles = (N // 128) * (K // 128)
            sp = max(1, min(64, 512 // tiles))
            kc = -(-M // (sp * 64)) * 64                                 # token rows per split, a multiple of the K-step
            xT = hip.transpose16(X, rows_pad=kc * sp) if X.dtype == mp else hip.cvt16(X, mp, transpose=True, rows_pad=kc * sp)
            part = hip.gemm16_splitk(hip.cvt16(dY, mp, transpose=True, rows_pad=kc * sp), xT, sp)
            self.put(lin.weight, hip.colsum(part.view(sp, N * K), torch.zeros(N * K, dtype=torch.float32, device=dev)).view(N, K))
        if self.need(getattr(lin, "bias", None)):
            self.put(lin.bias, hip.colsum(dY, torch.zeros(N, dtype=torch.float32, device=dev)))
        if not need_dx:
            return None
        # dX = dY . W: W^T [K, N] plays nn.Linear's weight
        return hip.gemm(dY16, hip.cvt16(lin.weight.detach(), mp, transpose=True), None, out_dtype=torch.float32)

    def ln_bwd(self, x, x_stride, ln, dy, dy_stride, dres, dres_stride, dx, dx_stride, rows, cols, eps):
        dev = dy.device
        dg = torch.zeros(cols, dtype=torch.float32, device=dev) if self.need(ln.weight) else None
        db = torch.zeros(cols, dtype=torch.float32, device=dev) if self.need(ln.bias) else None
        hip.layernorm_bwd(x, x_stride, ln.weight.detach(), dy, dy_stride, dres, dres_stride, dx, dx_stride, dg, db, rows, cols, eps)
        if dg is not None:
            self.put(ln.weight, dg)
        if db is not None:
            self.put(ln.bias, db)


def _attention_fwd(qkv: torch.Tensor, nb: int, L: int, heads: int, hd: int, alpha: float, mask: Optional[torch.Tensor]):
    """softmax(alpha * q k^T + mask) v on packed rows [nb*L, 3*heads*hd] (q | k | v, head-major).  Returns (out [nb*L, heads*hd], P)."""
    e = heads * hd
    dev = qkv.device
    P = torch.empty((nb, heads, L, L), dtype=torch.float32, device=dev)
    hip.gemm_ex(qkv, qkv, P, L, L, hd, sa=(3 * e, 1), sb=(1, 3 * e), sc=(L, 1), nb=(nb, heads), ba=(L * 3 * e, hd),
                bb=(L * 3 * e, hd), bc=(heads * L * L, L * L), alpha=alpha, offs=(0, e, 0))
    hip.softmax_rows(P, mask, heads * L)
    out = torch.empty((nb * L, e), dtype=torch.float32, device=dev)
    hip.gemm_ex(P, qkv, out, L, hd, L, sa=(L, 1), sb=(3 * e, 1), sc=(e, 1), nb=(nb, heads), ba=(heads * L * L, L * L),
                bb=(L * 3 * e, hd), bc=(L * e, hd), offs=(0, 2 * e, 0))
    return out, P


def _attention_bwd(dout: torch.Tensor, qkv: torch.Tensor, P: torch.Tensor, nb: int, L: int, heads: int, hd: int, alpha: float,
                   q_scale: float) -> torch.Tensor:
    """Gradient w.r.t. the packed qkv rows.  `alpha` multiplied the scores inside the attention; `q_scale` is a factor the stored
    q already carries from the projection's epilogue (its gradient flows to the un-scaled projection output)."""
    e = heads * hd
    dev = qkv.device
    dqkv = torch.empty_like(qkv)
    bP, bq, bo = (heads * L * L, L * L), (L * 3 * e, hd), (L * e, hd)
    # dV = P^T . dO
    hip.gemm_ex(P, dout, dqkv, L, hd, L, sa=(1, L), sb=(e, 1), sc=(3 * e, 1), nb=(nb, heads), ba=bP, bb=bo, bc=bq, offs=(0, 0, 2 * e))
    # dP = dO . V^T
    dP = torch.empty_like(P)
    hip.gemm_ex(dout, qkv, dP, L, L, hd, sa=(e, 1), sb=(1, 3 * e), sc=(L, 1), nb=(nb, heads), ba=bo, bb=bq, bc=bP, offs=(0, 2 * e, 0))
    hip.softmax_rows_bwd(P, dP, alpha)                  # dS (scores before the softmax), alpha folded in
    # dQ = dS . K  (times the epilogue factor of the stored q);  dK = dS^T . Q
    hip.gemm_ex(dP, qkv, dqkv, L, hd, L, sa=(L, 1), sb=(3 * e, 1), sc=(3 * e, 1), nb=(nb, heads), ba=bP, bb=bq, bc=bq,
                alpha=q_scale, offs=(0, e, 0))
    hip.gemm_ex(dP, qkv, dqkv, L, hd, L, sa=(1, L), sb=(3 * e, 1), sc=(3 * e, 1), nb=(nb, heads), ba=bP, bb=bq, bc=bq, offs=(0, 0, e))
    return dqkv


def fusion_fwd(model, tok: torch.Tensor, B: int, D: int, e: int, hs: int, mask: Optional[torch.Tensor]):
    """Slice Transformer (one pre-norm nn.TransformerEncoderLayer with ReLU + final LayerNorm; dino.py:134-153, resnet.py:180-190)
    over [CLS | D slice tokens] per volume; `model` carries slice_fusion.layers[0], slice_fusion.norm and cls_token.  Returns the
    CLS features [B, e] and what the backward needs."""
    dev = tok.device
    lay = model.slice_fusion.layers[0]
    L = D + 1
    hd = e // hs
    xs = torch.cat([model.cls_token.detach().expand(B, 1, e), tok.view(B, D, e)], dim=1).contiguous().view(B * L, e)
    mk = None
    if mask is not None:
        mk = torch.cat([torch.zeros((B, 1), dtype=torch.uint8, device=dev), mask.to(dev).to(torch.uint8)], dim=1).contiguous()
    t = {"xs": xs, "mask": mk}
    t["y1"] = hip.layernorm(xs, lay.norm1.weight.detach(), lay.norm1.bias.detach(), 1e-5)
    t["qkv"] = hip.gemm(t["y1"], lay.self_attn.in_proj_weight.detach(), lay.self_attn.in_proj_bias.detach())
    rot = getattr(lay.self_attn, "rotary_positional_encoding", None)
    t["rope"] = None
    if rot is not None:                                  # RoPE on q and k (transformer_blocks.py:262-264); the rotated rows are what the backward needs
        if not hasattr(rot, "freqs"):
            raise NotImplementedError("training step: the LieRE variant of the slice transformer is not on the HIP backward (its rotation "
                                      "generators are learned: the adjoint of the matrix exponential is not built)")
        t["rope"] = rot.freqs.detach().to(dev, torch.float32).contiguous()
        hip.rope_rows(t["qkv"], L, hs, hd, t["rope"], 1.0)
    t["ao"], t["P"] = _attention_fwd(t["qkv"], B, L, hs, hd, 1.0 / math.sqrt(hd), mk)
    xs1 = xs.clone()
    hip.axpby_cols(_lin_fwd(t["ao"], lay.self_attn.out_proj), xs1)
    t["xs1"] = xs1
    t["y2"] = hip.layernorm(xs1, lay.norm2.weight.detach(), lay.norm2.bias.detach(), 1e-5)
    t["f1"] = _lin_fwd(t["y2"], lay.linear1)
    t["r"] = hip.act_fwd(t["f1"], 1)
    xs2 = xs1.clone()
    hip.axpby_cols(_lin_fwd(t["r"], lay.linear2), xs2)
    t["xs2"] = xs2
    feat = hip.layernorm_rows(xs2, L * e, B, e, model.slice_fusion.norm.weight.detach(), model.slice_fusion.norm.bias.detach(), 1e-5)
    return feat, t


def fusion_bwd(G: "_Grads", model, t, dfeat: torch.Tensor, B: int, D: int, e: int, hs: int) -> torch.Tensor:
    """Backward of `fusion_fwd`: parameter gradients into G, returns the gradient of the slice tokens [B*D, e]."""
    dev = dfeat.device
    lay = model.slice_fusion.layers[0]
    L = D + 1
    hd = e // hs
    dxs2 = torch.zeros((B * L, e), dtype=torch.float32, device=dev)
    G.ln_bwd(t["xs2"], L * e, model.slice_fusion.norm, dfeat, e, None, 0, dxs2, L * e, B, e, 1e-5)      # row 0 of every volume
    dr = G.lin_bwd(dxs2, t["r"], lay.linear2)
    hip.act_bwd(t["f1"], dr, 1)
    dy2 = G.lin_bwd(dr, t["y2"], lay.linear1)
    dxs1 = torch.empty_like(dxs2)
    G.ln_bwd(t["xs1"], e, lay.norm2, dy2, e, dxs2, e, dxs1, e, B * L, e, 1e-5)
    dao = G.lin_bwd(dxs1, t["ao"], lay.self_attn.out_proj)
    dqkv = _attention_bwd(dao, t["qkv"], t["P"], B, L, hs, hd, 1.0 / math.sqrt(hd), 1.0)
    if t["rope"] is not None:
        hip.rope_rows(dqkv, L, hs, hd, t["rope"], -1.0)    # adjoint of the rotation: gradients of the un-rotated projections
    sa = lay.self_attn
    if G.need(sa.in_proj_weight):
        dW = torch.empty_like(sa.in_proj_weight)
        hip.gemm_ex(dqkv, t["y1"], dW, 3 * e, e, B * L, sa=(1, 3 * e), sb=(e, 1), sc=(e, 1))
        G.put(sa.in_proj_weight, dW)
    if G.need(sa.in_proj_bias):
        G.put(sa.in_proj_bias, hip.colsum(dqkv, torch.zeros(3 * e, dtype=torch.float32, device=dev)))
    dy1 = torch.empty((B * L, e), dtype=torch.float32, device=dev)
    hip.gemm_ex(dqkv, sa.in_proj_weight.detach(), dy1, B * L, e, 3 * e, sa=(3 * e, 1), sb=(e, 1), sc=(e, 1))
    dxs = torch.empty_like(dxs2)
    G.ln_bwd(t["xs"], e, lay.norm1, dy1, e, dxs1, e, dxs, e, B * L, e, 1e-5)
    if G.need(model.cls_token):
        dcls = torch.zeros(e, dtype=torch.float32, device=dev)
        hip.colsum(dxs.view(B, L * e)[:, :e], dcls)
        G.put(model.cls_token, dcls)
    return dxs.view(B, L, e)[:, 1:].contiguous().view(B * D, e)


def forward_train(model, source: torch.Tensor, mask: Optional[torch.Tensor], without_linear: bool, encoder_state: Optional[bool] = None):
    """The training forward: (logits or features, the state `backward_train` reads).  encoder_state: whether a backward will go through the
    encoder at all -- the autograd node passes its needs_input_grad; None derives it as the node would (an encoder parameter or ``source``
    requires grad).  Without it nothing of the encoder but the slice embeddings is kept."""
    if model.rotary is not None and model.rotary != "RoPE":
        raise NotImplementedError("training step: the LieRE variant of the slice transformer is not on the HIP backward (its rotation "
                                  "generators are learned: the adjoint of the matrix exponential is not built); RoPE is")
    enc = model.encoder
    dev = model.device
    sh = _sharding_of(model)
    x = source.to(dev) if sh is None else source         # a shard moves its own slices only
    B, C, D0, H, W = x.shape
    if C != 1:
        x = x.permute(0, 2, 1, 3, 4)
    D = D0 * C
    assert H % PATCH == 0, f"Input image height {H} is not a multiple of patch height {PATCH}"
    assert W % PATCH == 0, f"Input image width {W} is not a multiple of patch width: {PATCH}"
    interp = _pos_resampled(enc, H, W)
    d0, d1, dpad = sh.shard_range(D) if sh is not None else (0, D, D)
    dl = d1 - d0                                         # this rank's slices [d0, d1) of every volume: all of them without sharding
    vol = (x.reshape(B, D, H, W)[:, d0:d1].to(dev) if sh is not None else x).reshape(B * dl, H, W).float().contiguous()
    mode = train_mode.resolve(model)                     # before the first collective: a refused mode raises on every rank alike
    sv = {"B": B, "D": D, "H": H, "W": W, "vol": vol, "without_linear": without_linear, "src_shape": (B, C, D0, H, W),
          "interp": interp, "shard": (d0, d1, dpad) if sh is not None else None}
    sv["mp"], sv["storage16"] = mode.mp, mode.storage16   # the backward reads the resolved mode from here (an autocast region may have ended)
    sv["mode"], sv["chunk"] = mode, mode.chunk            # (the chunked backward's recomputation runs in the whole of it)
    if encoder_state is None:
        encoder_state = bool(torch.is_tensor(source) and source.requires_grad) or any(p.requires_grad for p in enc.parameters())
    sv["encoder_state"] = bool(encoder_state)
    if sh is None:
        emb = _encoder_fwd_kept(model, sv, mode, vol, B * D, H, W)
    else:
        # slice sharding: the encoder on this rank's rows alone (no kernel at all on an empty shard: zeros travel), ONE all-gather of the
        # padded shards' slice embeddings, and everything behind the encoder replicated on the full [B*D, E].  Every rank of the group
        # must be given the same batch: the replicated stage and its gradients are only identical across ranks if it is.
        E = enc.embed_dim
        emb_l = torch.zeros((B, dpad, E), dtype=torch.float32, device=dev)
        if dl:
            emb_l[:, :dl].copy_(_encoder_fwd_kept(model, sv, mode, vol, B * dl, H, W).view(B, dl, E))
        emb = sh.all_gather_slices(emb_l, D).reshape(B * D, E)
    sv["emb"] = emb
    return _fusion_head_fwd(model, sv, emb, B, D, mask, without_linear)


def _pos_resampled(enc, H: int, W: int) -> bool:
    """Whether an H x W input resamples the stored position grid; NotImplementedError for a register-token encoder that would."""
    n_stored = enc.pos_embed.shape[1] - 1
    interp = not ((H // PATCH) * (W // PATCH) == n_stored and H == W)
    if interp and int(enc.num_register_tokens):
        # register encoders are the hub's dinov2_vit*14_reg (anti-aliased, size-based resampling: models/dino.py::_pos_patch); the
        # adjoint of that filter is not built -- train them at the stored grid (518 x 518 for the hub weights)
        raise NotImplementedError("training step: register-token encoders train at their stored position grid only (the adjoint of the "
                                  "anti-aliased position resampling is not on the HIP backward)")
    return interp


def _sharding_of(model):
    """The model's SliceSharding if it spans more than one rank, else None."""
    sh = getattr(model, "_sharding", None)
    return sh if sh is not None and sh.world_size > 1 else None


def _encoder_fwd_kept(model, sv, mode: TrainMode, vol: torch.Tensor, n: int, H: int, W: int) -> torch.Tensor:
    """The slice embeddings [n, E] of the n slices in `vol`, and in sv what the forward keeps of the encoder for the backward:
      mode.chunk == 0, a backward through the encoder to come   one pass, its whole state (`_encoder_fwd`);
      mode.chunk == 0, none to come (frozen encoder, no source gradient)   one pass into a throw-away dict: nothing;
      mode.chunk == k > 0   the rows k at a time (the last chunk may be short, a chunk may straddle a volume boundary), each into a
                            throw-away dict: only what does not depend on the chunk (`_encoder_consts`); `_encoder_bwd_chunked`
                            recomputes the rest."""
    if mode.chunk <= 0:
        return _encoder_fwd(model, sv if sv["encoder_state"] else {"interp": sv["interp"]}, mode, vol, n, H, W)
    consts = sv["consts"] = _encoder_consts(model.encoder, sv["interp"], H, W, vol.device)
    emb = torch.empty((n, model.encoder.embed_dim), dtype=torch.float32, device=vol.device)
    for r0 in range(0, n, mode.chunk):
        r1 = min(n, r0 + mode.chunk)
        emb[r0:r1].copy_(_encoder_fwd(model, {}, mode, vol[r0:r1], r1 - r0, H, W, consts))
    return emb


def _encoder_consts(enc, interp: bool, H: int, W: int, dev) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """What the token stage reads besides the volume, the same for every slice: (the position rows of the gh x gw patch grid, the prefix
    rows [1 + R, E], the channel-summed patch kernel [E, 14 * 16])."""
    R = int(enc.num_register_tokens)                     # register tokens (vision_transformer.py:222-230): extra prefix rows without a position
    E = enc.embed_dim
    gh, gw = H // PATCH, W // PATCH
    # ---- tokens (patch_embed.py:68-81; vision_transformer.py:213-232)
    pos = enc.pos_embed.detach()[0]
    Mg = int(math.isqrt(pos.shape[0] - 1))
    pos_patch = hip.pos_embed_interp(pos[1:].contiguous(), Mg, gh, gw, 0.1) if interp else pos[1:].contiguous()
    prefix = torch.zeros((1 + R, E), dtype=torch.float32, device=dev)
    prefix[:1].copy_(pos[:1])
    hip.axpby_cols(enc.cls_token.detach().reshape(1, E), prefix[:1])
    if R:
        prefix[1:].copy_(enc.register_tokens.detach()[0])
    wsum = torch.zeros((E, PATCH * 16), dtype=torch.float32, device=dev)            # three identical input channels: one summed kernel
    w = enc.patch_embed.proj.weight.detach()
    for c in range(3):
        hip.axpby_cols(w[:, c].contiguous().view(E * PATCH, PATCH), wsum, x_stride=PATCH, y_stride=16, rows=E * PATCH, cols=PATCH)
    return pos_patch, prefix, wsum


def _encoder_fwd(model, sv, mode: TrainMode, vol: torch.Tensor, n: int, H: int, W: int, consts=None, n_blocks: Optional[int] = None,
                 want_cls: bool = True) -> Optional[torch.Tensor]:
    """Tokens, blocks and the final LayerNorm's CLS rows of the n slices in `vol`; what the backward needs goes into sv.  Returns the slice
    embeddings [n, E].  consts: `_encoder_consts` of this shape if the caller has them (a chunk of several), else they are made here.
    The encoder API's calls (`encoder_forward_train`) also bring: vol [n, 3, H, W], three distinct channels through the RGB patch embedding
    (mst_patch_embed_rgb on the fp32 kernel image, kept as sv["wrgb"] for its data gradient); n_blocks, the forward stops behind block
    n_blocks - 1 (sv["xL"] is the stream there); want_cls False, no CLS rows (returns None)."""
    enc = model.encoder
    R = int(enc.num_register_tokens)
    E, heads = enc.embed_dim, enc.num_heads
    N = 1 + R + (H // PATCH) * (W // PATCH)
    M = n * N
    sv["R"] = R
    pos_patch, prefix, wsum = consts if consts is not None else _encoder_consts(enc, sv["interp"], H, W, vol.device)
    sv["wsum"] = wsum                                    # the source gradient's kernel (mst_patch_embed_dgrad) reads the same sum
    if vol.dim() == 4:
        sv["wrgb"] = hip.pack_patch_rgb(enc.patch_embed.proj.weight.detach(), torch.float32)
        xt = hip.patch_embed_rgb(vol, sv["wrgb"], enc.patch_embed.proj.bias.detach(), prefix, pos_patch).view(M, E)
    else:
        xt = hip.patch_embed(vol, wsum, enc.patch_embed.proj.bias.detach(), prefix, pos_patch).view(M, E)
    # ---- blocks (block.py:89-114)
    blist = list(enc.block_list())[:n_blocks]
    block_fwd = _block_fwd_16 if mode.storage16 else _block_fwd
    xn = hip.layernorm(xt, blist[0].norm1.weight.detach(), blist[0].norm1.bias.detach(), 1e-6, out_dtype=mode.mp) if mode.storage16 else None
    blocks = []
    for blk, nxt in zip(blist, blist[1:] + [None]):
        s, xt, xn = block_fwd(blk, nxt, xt, xn, mode, n, N, heads, E)
        blocks.append(s)
    sv["blocks"], sv["xL"] = blocks, xt
    if not want_cls:
        return None
    return hip.layernorm_rows(xt, N * E, n, E, enc.norm.weight.detach(), enc.norm.bias.detach(), 1e-6)     # CLS rows


def _fusion_head_fwd(model, sv, emb: torch.Tensor, B: int, D: int, mask: Optional[torch.Tensor], without_linear: bool):
    """The across-slice stage (dino.py:134-166) and the head on the slice embeddings [B*D, E] of whole volumes."""
    import torch.nn as nn
    dev = emb.device
    e = model.emb_ch
    tok = _lin_fwd(emb, model.bottleneck) if hasattr(model, "bottleneck") else emb
    if hasattr(model, "slice_pos_emb"):
        tok = tok.clone()
        p = model.slice_pos_emb.weight.detach()[:D].contiguous()
        for b in range(B):
            hip.axpby_cols(p, tok[b * D:(b + 1) * D])
    ft = model.slice_fusion_type
    if ft == "transformer":
        feat, sv["fusion"] = fusion_fwd(model, tok, B, D, e, 12, mask)
    elif ft == "linear":
        feat = tok.reshape(B, D * e)
    else:                                                                        # 'average' (dino.py:156-157)
        feat = torch.zeros((B, e), dtype=torch.float32, device=dev)
        for b in range(B):
            hip.colsum(tok[b * D:(b + 1) * D], feat[b])
        hip.axpby_cols(feat, feat, alpha=1.0 / D, beta=0.0)
    sv["tok"], sv["feat"] = tok, feat
    if without_linear or isinstance(model.linear, nn.Identity):
        sv["head"] = False
        return feat, sv
    if ft == "linear" and feat.shape[1] != model.linear.weight.shape[1]:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({B}x{feat.shape[1]} and "
                           f"{model.linear.weight.shape[1]}x{model.linear.weight.shape[0]})")
    sv["head"] = True
    return _lin_fwd(feat, model.linear), sv


def backward_train(model, sv, dout: torch.Tensor, needed: Optional[Set[int]] = None,
                   need_src: bool = False) -> Tuple[Dict[int, torch.Tensor], Optional[torch.Tensor]]:
    """Gradients of the parameters whose id is in `needed` (None: all) and, with `need_src`, of the volume the forward read (fp32
    [B*D, H, W], the forward's slice order); products whose result nobody asked for are skipped."""
    G = _Grads(needed=needed)
    enc = model.encoder
    dev = dout.device
    B, D, H, W = sv["B"], sv["D"], sv["H"], sv["W"]
    e = model.emb_ch
    dfeat = G.lin_bwd(dout, sv["feat"], model.linear) if sv["head"] else dout
    ft = model.slice_fusion_type
    if ft == "transformer":
        dtok = fusion_bwd(G, model, sv["fusion"], dfeat, B, D, e, 12)
    elif ft == "linear":
        dtok = dfeat.reshape(B * D, e).contiguous()
    else:
        dtok = dfeat[:, None, :].expand(B, D, e).contiguous().view(B * D, e)
        hip.axpby_cols(dtok, dtok, alpha=1.0 / D, beta=0.0)
    if hasattr(model, "slice_pos_emb") and G.need(model.slice_pos_emb.weight):
        dp = torch.zeros_like(model.slice_pos_emb.weight)
        acc = torch.zeros(D * e, dtype=torch.float32, device=dev)
        hip.colsum(dtok.view(B, D * e), acc)
        dp[:D].copy_(acc.view(D, e))
        G.put(model.slice_pos_emb.weight, dp)
    demb = G.lin_bwd(dtok, sv["emb"], model.bottleneck) if hasattr(model, "bottleneck") else dtok
    if not need_src and not (sv["encoder_state"] and any(p.requires_grad for p in enc.parameters())):
        return G.by_param, None                                                  # frozen encoder (dino.py:65-67)
    if not sv["encoder_state"]:
        raise RuntimeError("training step: this forward was told that no backward goes through the encoder (no encoder parameter and no source "
                           "required grad) and kept nothing of it; a source gradient needs forward_train(..., encoder_state=True)")
    encoder_bwd = _encoder_bwd_chunked if sv["chunk"] > 0 else _encoder_bwd
    if sv["shard"] is None:
        return G.by_param, encoder_bwd(G, model, sv, demb, B * D, need_src)
    # ---- slice sharding: this rank's rows of d emb through its own slices, then the encoder's parameter gradients summed over the group
    # (the replicated parameters above are complete and identical on every rank already: they do not travel) and d source gathered.
    # Every rank issues the same collectives whatever its shard holds; an empty shard launches no kernel and contributes zeros.
    sh = _sharding_of(model)
    d0, d1, dpad = sv["shard"]
    dl = d1 - d0
    dvol = encoder_bwd(G, model, sv, demb.reshape(B, D, -1)[:, d0:d1].reshape(B * dl, -1).contiguous(), B * dl, need_src) if dl else None
    wanted = [p for p in enc.parameters() if G.need(p) and p is not enc.mask_token]                      # (the forward never reads mask_token)
    if wanted:
        # ONE flat fp32 bucket: a single concatenation fills it, the gradients handed back are views of the reduced bucket
        if dl:
            missing = [tuple(p.shape) for p in wanted if id(p) not in G.by_param]
            if missing:
                raise RuntimeError(f"training step under slice sharding: no gradient for encoder parameters of shapes {missing}")
            flat = torch.cat([G.by_param[id(p)].reshape(-1) for p in wanted])
        else:
            flat = torch.zeros(sum(p.numel() for p in wanted), dtype=torch.float32, device=dev)
        sh.all_reduce_sum(flat)
        for p, g in zip(wanted, flat.split([p.numel() for p in wanted])):
            G.by_param[id(p)] = g.view(p.shape)
    if not need_src:
        return G.by_param, None
    dvol_l = torch.zeros((B, dpad, H * W), dtype=torch.float32, device=dev)
    if dl:
        dvol_l[:, :dl].copy_(dvol.view(B, dl, H * W))
    return G.by_param, sh.all_gather_slices(dvol_l, D).view(B * D, H, W)


def _encoder_bwd_chunked(G: "_Grads", model, sv, demb: torch.Tensor, n: int, need_src: bool) -> Optional[torch.Tensor]:
    """`_encoder_bwd`'s results for a forward that kept no encoder state (train_chunk_slices > 0): per chunk of the forward, in its order,
    the encoder forward again with saving -- in the mode the forward resolved -- and straight into that chunk's backward.  The parameter
    gradients of the chunks sum in G (`_Grads.put`: the first is kept, every later one added, a fixed order); each chunk's d volume is
    written into its rows of one [n, H, W] buffer.  One chunk's state lives at a time."""
    H, W, k = sv["H"], sv["W"], sv["chunk"]
    dvol = torch.empty((n, H, W), dtype=torch.float32, device=demb.device) if need_src else None
    for r0 in range(0, n, k):
        r1 = min(n, r0 + k)
        cs = {"H": H, "W": W, "mp": sv["mp"], "interp": sv["interp"], "vol": sv["vol"][r0:r1]}
        _encoder_fwd(model, cs, sv["mode"], cs["vol"], r1 - r0, H, W, sv["consts"])
        _encoder_bwd(G, model, cs, demb[r0:r1], r1 - r0, need_src, dvol[r0:r1] if need_src else None)
        del cs                                           # the chunk's state goes before the next chunk's is made
    return dvol


def _tap_bwd(G: "_Grads", enc, stream: torch.Tensor, dx: Optional[torch.Tensor], dnorm: Optional[torch.Tensor], draw: Optional[torch.Tensor],
             M: int, E: int) -> torch.Tensor:
    """The gradient of a tap joins the running d x where the walk arrives behind its block: `draw` [M, E], the gradient of the stream itself,
    is added; `dnorm`, the gradient of encoder.norm(stream), goes through the dense LayerNorm backward with the running d x as its residual
    input (encoder.norm's d weight / d bias of several taps sum in G, in walk order).  dx None: nothing has arrived from above."""
    if draw is not None:
        dx = draw.clone() if dx is None else hip.axpby_cols(draw, dx)
    if dnorm is not None:
        out = torch.empty((M, E), dtype=torch.float32, device=dnorm.device)
        G.ln_bwd(stream, E, enc.norm, dnorm, E, dx, E if dx is not None else 0, out, E, M, E, 1e-6)
        dx = out
    return dx


def _encoder_bwd(G: "_Grads", model, sv, demb: Optional[torch.Tensor], n: int, need_src: bool, dvol: Optional[torch.Tensor] = None,
                 taps: Optional[Dict[int, Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]]] = None) -> Optional[torch.Tensor]:
    """Backward of `_encoder_fwd` over its n slices from the gradient of their embeddings [n, E]: parameter gradients into G; returns d volume
    ([n, H, W] fp32, or [n, 3, H, W] of an RGB forward; written into `dvol` if the caller brings it) with `need_src`.
    The encoder API's node also brings taps = {block: (d encoder.norm(stream), d stream)} over all N rows of the stream behind that block
    (either may be None), and demb may be None: the walk starts at the highest block a gradient enters behind; the blocks above it are not
    walked and their parameters get no gradient.  Without taps the launches are the classifier's: CLS rows into d x, then every block."""
    enc = model.encoder
    dev = sv["xL"].device
    H, W = sv["H"], sv["W"]
    G.mp = sv["mp"]                                      # the blocks' nn.Linear products on 16-bit operands, as the forward resolved them
    E, heads = enc.embed_dim, enc.num_heads
    gh, gw = H // PATCH, W // PATCH
    Np = gh * gw
    R = sv["R"]
    N = 1 + R + Np
    M = n * N
    blist, taps = enc.block_list(), taps or {}
    dx = None
    if demb is not None:
        dx = torch.zeros((M, E), dtype=torch.float32, device=dev)
        G.ln_bwd(sv["xL"], N * E, enc.norm, demb, E, None, 0, dx, N * E, n, E, 1e-6)                     # CLS rows only
    for i in range(len(blist) - 1 if demb is not None else max(taps), -1, -1):
        blk, s = blist[i], sv["blocks"][i]
        if i in taps:                                    # the stream behind block i is block i + 1's input (the last one: xL)
            dx = _tap_bwd(G, enc, sv["blocks"][i + 1]["x0"] if i + 1 < len(sv["blocks"]) else sv["xL"], dx, *taps[i], M, E)
        # x2 = x1 + ls2 * fc2(gelu(fc1(norm2 x1)))
        dbr = dx
        if hasattr(blk, "ls2"):
            if G.need(blk.ls2.gamma):
                G.put(blk.ls2.gamma, hip.colsum(dx, torch.zeros(E, dtype=torch.float32, device=dev), b=s["br2"]))
            dbr = torch.empty_like(dx)
            hip.axpby_cols(dx, dbr, g=blk.ls2.gamma.detach(), beta=0.0)
        x16 = s.get("x16", {})
        if _is_swiglu(blk):                              # x2 = x1 + ls2 * w3(silu(x1') * x2'), [x1' | x2'] = w12(norm2 x1)
            dh = G.lin_bwd(dbr, s["h"], blk.mlp.w3, X16=x16.get(id(blk.mlp.w3)))
            dx12 = hip.swiglu_bwd(s["x12"], dh)
            dxn2 = G.lin_bwd(dx12, s["xn2"], blk.mlp.w12, X16=x16.get(id(blk.mlp.w12)))
        else:
            dh = G.lin_bwd(dbr, s["hact"], blk.mlp.fc2, X16=x16.get(id(blk.mlp.fc2)))
            hip.act_bwd(s["hpre"], dh, 0)
            dxn2 = G.lin_bwd(dh, s["xn2"], blk.mlp.fc1, X16=x16.get(id(blk.mlp.fc1)))
        dx1 = torch.empty_like(dx)
        G.ln_bwd(s["x1"], E, blk.norm2, dxn2, E, dx, E, dx1, E, M, E, 1e-6)
        # x1 = x0 + ls1 * proj(attn(qkv(norm1 x0)))
        dbr = dx1
        if hasattr(blk, "ls1"):
            if G.need(blk.ls1.gamma):
                G.put(blk.ls1.gamma, hip.colsum(dx1, torch.zeros(E, dtype=torch.float32, device=dev), b=s["br1"]))
            dbr = torch.empty_like(dx1)
            hip.axpby_cols(dx1, dbr, g=blk.ls1.gamma.detach(), beta=0.0)
        da = G.lin_bwd(dbr, s["a"], blk.attn.proj, X16=x16.get(id(blk.attn.proj)))
        if "lse" in s:                                   # train_attention='flash': dQ carries the epilogue's factor like _attention_bwd's q_scale
            dqkv = hip.attention_train_bwd(s["qkv16"], s["a"], da, s["lse"], n, N, heads, dq_scale=0.125)
        else:
            dqkv = _attention_bwd(da, s["qkv"], s["P"], n, N, heads, 64, 1.0, 0.125)
        dxn1 = G.lin_bwd(dqkv, s["xn1"], blk.attn.qkv, X16=x16.get(id(blk.attn.qkv)))
        dx0 = torch.empty_like(dx)
        G.ln_bwd(s["x0"], E, blk.norm1, dxn1, E, dx1, E, dx0, E, M, E, 1e-6)
        dx = dx0
    # ---- tokens
    dsrc = None
    if need_src:                                         # d volume straight from the patch rows of dx (adjoint of the grey -> RGB patch embedding)
        if "wrgb" in sv:
            dsrc = hip.patch_embed_rgb_dgrad(dx, sv["wrgb"], n, H, W, tokens=N, first=1 + R, out=dvol)
        else:
            dsrc = hip.patch_embed_dgrad(dx, sv["wsum"], n, H, W, tokens=N, first=1 + R, out=dvol)
    pe = enc.patch_embed.proj
    if G.need(enc.cls_token) or G.need(enc.pos_embed):
        dcls = torch.zeros(E, dtype=torch.float32, device=dev)
        hip.colsum(dx.view(n, N * E)[:, :E], dcls)
        G.put(enc.cls_token, dcls.clone())
    if R and G.need(enc.register_tokens):                # d register_tokens[r] = sum over slices of row 1 + r
        dreg = torch.zeros((R, E), dtype=torch.float32, device=dev)
        for r in range(R):
            hip.colsum(dx.view(n, N * E)[:, (1 + r) * E:(2 + r) * E], dreg[r])
        G.put(enc.register_tokens, dreg.view(1, R, E))
    if not (G.need(enc.pos_embed) or G.need(pe.bias) or G.need(pe.weight)):
        return dsrc
    dpatch = dx.view(n, N, E)[:, 1 + R:].contiguous().view(n * Np, E)
    if G.need(enc.pos_embed):
        dposp = torch.zeros(Np * E, dtype=torch.float32, device=dev)
        hip.colsum(dpatch.view(n, Np * E), dposp)
        dpos = torch.zeros_like(enc.pos_embed)
        dpos[0, 0].copy_(dcls)
        if sv["interp"]:
            Mg = int(math.isqrt(enc.pos_embed.shape[1] - 1))
            hip.pos_embed_interp_bwd(dposp.view(Np, E), Mg, gh, gw, 0.1, dpos[0, 1:])
        else:
            dpos[0, 1:].copy_(dposp.view(Np, E))
        G.put(enc.pos_embed, dpos)
    if G.need(pe.bias):
        G.put(pe.bias, hip.colsum(dpatch, torch.zeros(E, dtype=torch.float32, device=dev)))
    if G.need(pe.weight) and "wrgb" in sv:               # three distinct channels: the implicit GEMM over the image in place
        G.put(pe.weight, hip.patch_embed_rgb_wgrad(dx, sv["vol"], E, tokens=N, first=1 + R))
    elif G.need(pe.weight):
        col = hip.im2col14(sv["vol"])
        dW = torch.empty((E, 196), dtype=torch.float32, device=dev)
        hip.gemm_ex(dpatch, col, dW, E, 196, n * Np, sa=(1, E), sb=(196, 1), sc=(196, 1))
        G.put(pe.weight, dW.view(E, 1, PATCH, PATCH).expand(E, 3, PATCH, PATCH).contiguous())
    return dsrc


def _source_grad(dvol: torch.Tensor, sv, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """Adjoint of the forward's input handling: [B*D, H, W] fp32 -> source's [B, C, D0, H, W] layout (inverse of the
    permute(0, 2, 1, 3, 4) / reshape), dtype and device."""
    B, C, D0, H, W = sv["src_shape"]
    g = dvol.view(B, D0, C, H, W).permute(0, 2, 1, 3, 4) if C != 1 else dvol.view(B, C, D0, H, W)
    return g.to(device=device, dtype=dtype).contiguous()


def fp32_device_params(model) -> List[torch.nn.Parameter]:
    """The model's parameters, the inputs of its autograd node: all fp32 on the device, or RuntimeError."""
    params = list(model.parameters())
    for p in params:
        if p.dtype != torch.float32 or p.device.type != "cuda":
            raise RuntimeError("training step: parameters must be fp32 on the MI355X (model.float().cuda()); there is no CPU fallback")
    return params


def route_grads(grads: Dict[int, torch.Tensor], params, needs) -> List[Optional[torch.Tensor]]:
    """{id(param): grad} -> the node's returned gradients in `params` order; None where `needs` (needs_input_grad from the first
    parameter on) is off or no gradient was produced."""
    return [grads.get(id(p)) if need else None for p, need in zip(params, needs)]


class _MSTFunction(torch.autograd.Function):
    """One autograd node for the whole model: inputs are the parameters (so that autograd, DDP hooks and optimisers see
    ordinary ``.grad`` accumulation) and the source volume, output the logits (or features)."""

    @staticmethod
    def forward(ctx, model, source, mask, without_linear, *params):
        # a frozen encoder under a source that needs no gradient: no backward reads its state, so the forward keeps none of it
        enc_ids = {id(p) for p in model.encoder.parameters()}
        encoder_state = bool(ctx.needs_input_grad[1]) or any(need and id(p) in enc_ids for p, need in zip(params, ctx.needs_input_grad[4:]))
        with torch.no_grad():
            out, saved = forward_train(model, source, mask, without_linear, encoder_state)
        ctx.model, ctx.saved, ctx.params = model, saved, params
        ctx.src_dtype, ctx.src_device = source.dtype, source.device
        return out

    @staticmethod
    def backward(ctx, dout):
        needed = {id(p) for p, need in zip(ctx.params, ctx.needs_input_grad[4:]) if need}
        need_src = bool(ctx.needs_input_grad[1])
        with torch.no_grad():
            grads, dvol = backward_train(ctx.model, ctx.saved, dout.contiguous().float(), needed, need_src)
            dsrc = _source_grad(dvol, ctx.saved, ctx.src_dtype, ctx.src_device) if need_src else None
        ctx.saved = None
        return (None, dsrc, None, None, *route_grads(grads, ctx.params, ctx.needs_input_grad[4:]))


def forward_with_grad(model, source, mask, without_linear: bool):
    params = fp32_device_params(model)
    return _MSTFunction.apply(model, source, mask, without_linear, *params)


# ---- the encoder API in grad mode (models/dino.py `_ViT._encode` with the owner's ``encoder_grad``) ---------------------------------------
def encoder_forward_train(model, x: torch.Tensor, blocks, norm: bool, want_cls: bool, prenorm: bool = False, encoder_state: bool = True):
    """`_encoder_fwd` for encoder.forward / forward_features / get_intermediate_layers on x [n, 3, H, W] or [n, 1, H, W] (the grey path:
    mst_patch_embed on the channel sum) in the resolved training mode -> ((class tokens [n, E] or None, taps [len(blocks), n, N, E] or None:
    the stream behind the blocks `blocks` (ascending), through encoder.norm when `norm`, the same streams un-normalised when `norm` and
    `prenorm`, else None), the state `encoder_backward_train` reads).  The stream behind block i is block i + 1's saved input, so a tap
    keeps nothing of its own; without class tokens the forward stops behind the highest block asked for.  All tokens of local images:
    train_chunk_slices and slice sharding do not apply here."""
    enc = model.encoder
    dev = model.device
    n, C, H, W = x.shape
    interp = _pos_resampled(enc, H, W)
    mode = train_mode.resolve(model)
    vol = x.detach().to(dev).float()
    vol = (vol.reshape(n, H, W) if C == 1 else vol).contiguous()
    blocks = list(blocks)
    sv = {"H": H, "W": W, "interp": interp, "mp": mode.mp, "vol": vol, "taps": blocks, "norm": bool(norm), "n": n}
    E = enc.embed_dim
    st = sv if encoder_state else {"interp": interp}
    cls = _encoder_fwd(model, st, mode, vol, n, H, W, n_blocks=None if want_cls else max(blocks) + 1, want_cls=want_cls)
    taps = raw = None
    if blocks:
        N = st["xL"].shape[0] // n
        streams = [st["blocks"][i + 1]["x0"] if i + 1 < len(st["blocks"]) else st["xL"] for i in blocks]
        if norm:
            taps = torch.stack([hip.layernorm(t, enc.norm.weight.detach(), enc.norm.bias.detach(), 1e-6) for t in streams]).view(len(blocks), n, N, E)
        if prenorm or not norm:
            raw = torch.stack(streams).view(len(blocks), n, N, E)
        if not norm:
            taps, raw = raw, None
    return (cls, taps, raw), sv


def encoder_backward_train(model, sv, dcls, dtaps, draw, needed: Optional[Set[int]] = None, need_src: bool = False):
    """Gradients of `encoder_forward_train`'s three results (each may be None: nobody used it) -> ({id(param): grad}, d x or None)."""
    G = _Grads(needed=needed)
    n = sv["n"]
    if not sv["norm"]:
        dtaps, draw = None, dtaps
    taps = {}
    for k, i in enumerate(sv["taps"]):
        dn = dtaps[k].reshape(-1, dtaps.shape[-1]).contiguous().float() if dtaps is not None else None
        dr = draw[k].reshape(-1, draw.shape[-1]).contiguous().float() if draw is not None else None
        if dn is not None or dr is not None:
            taps[i] = (dn, dr)
    if dcls is None and not taps:
        return {}, None
    dsrc = _encoder_bwd(G, model, sv, dcls.contiguous().float() if dcls is not None else None, n, need_src, taps=taps)
    return G.by_param, dsrc


class _EncoderFunction(torch.autograd.Function):
    """One autograd node per encoder API call: inputs are x and the model's parameters, outputs the dense tensors of the inference path
    (class tokens, taps, and for forward_features the un-normalised last stream beside the normalised one).  Slicing, reshape and permutes
    stay torch ops behind the node, so an unused row or tap arrives as zeros and an unused output as None."""

    @staticmethod
    def forward(ctx, model, x, blocks, norm, want_cls, prenorm, *params):
        ctx.set_materialize_grads(False)
        enc_ids = {id(p) for p in model.encoder.parameters()}
        state = bool(ctx.needs_input_grad[1]) or any(need and id(p) in enc_ids for p, need in zip(params, ctx.needs_input_grad[6:]))
        with torch.no_grad():
            outs, saved = encoder_forward_train(model, x, blocks, norm, want_cls, prenorm, state)
        ctx.model, ctx.saved, ctx.params = model, (saved if state else False), params         # False: no backward can reach the encoder, nothing kept
        ctx.x_meta = (x.shape, x.dtype, x.device)
        return outs

    @staticmethod
    def backward(ctx, dcls, dtaps, draw):
        if ctx.saved is False:
            return (None,) * (6 + len(ctx.params))
        if ctx.saved is None:
            raise RuntimeError("encoder API: the state of this call is gone (a second backward through the same call)")
        needed = {id(p) for p, need in zip(ctx.params, ctx.needs_input_grad[6:]) if need}
        need_src = bool(ctx.needs_input_grad[1])
        with torch.no_grad():
            grads, dsrc = encoder_backward_train(ctx.model, ctx.saved, dcls, dtaps, draw, needed, need_src)
            if dsrc is not None:
                shape, dtype, device = ctx.x_meta
                dsrc = dsrc.view(shape).to(device=device, dtype=dtype)
        ctx.saved = None
        return (None, dsrc, None, None, None, None, *route_grads(grads, ctx.params, ctx.needs_input_grad[6:]))


def encoder_forward_with_grad(model, x, blocks, norm: bool, want_cls: bool, prenorm: bool = False):
    """(class tokens or None, taps or None, un-normalised taps or None) of one encoder API call, attached to one `_EncoderFunction` node."""
    params = fp32_device_params(model)
    return _EncoderFunction.apply(model, x, tuple(blocks), bool(norm), bool(want_cls), bool(prenorm), *params)
