"""The reference's decoder under training (``models/transformer.py:328-427, 466-517``), restated on the fused differentiable operators.

Written against attribute names: it serves this package's parameter containers and, through ``patch_decoder``, the reference's own modules;
the reference is never imported.

* ``grouped_self_attention``: the reference splits q, k and v into ``group_detr`` groups, concatenates them along the batch, runs its
  ``MultiheadAttention`` (which materialises (B * G * heads, nq, nq) weights) and concatenates the result back. Here one Linear forms q and k
  and one forms v, and ``fused_attention`` reads the three as (B * G, heads, nq, hd) strided views of those outputs: the group is an index.
* ``decoder_layer_forward``: self-attention, ``FusedMSDeformAttnFunction`` cross-attention, FFN, the three post-norms.
* ``decoder_forward``: the published configuration (``lite_refpoint_refine``, ``bbox_reparam``, no ``bbox_embed``): the reference points and
  ``query_pos`` are formed once, through ``query_sine_embed``.

``fused``: None takes a fused operator wherever its limits admit the call and the tensors are on a ROCm device, False is all torch (CPU and
float64 included), True insists. Dropout with p > 0 in training mode raises ``NotImplementedError`` (the attention-weight dropout would live
inside the fused core).
"""
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import attention as A
from . import deform_train as DT
from . import train_glue as TG

_DECODER_ATTRS = ("layers", "norm", "ref_point_head", "lite_refpoint_refine", "bbox_reparam")


def _want(fused, possible, what):
    if fused is None:
        return possible
    if fused and not possible:
        raise RuntimeError(f"{what}: fused=True, but the call is outside the fused operator's range (device, dtype or shape)")
    return bool(fused)


def refuse_dropout(module):
    """Raises when ``module`` is in training mode and holds an active dropout: the fused cores implement none."""
    for m in module.modules():
        if not m.training:
            continue
        if isinstance(m, nn.Dropout) and m.p > 0:
            raise NotImplementedError(f"lwdetr_amd: dropout p = {m.p} under training is not implemented in the fused forward (set dropout to 0)")
        p = getattr(m, "dropout", 0.0) if hasattr(m, "in_proj_weight") else 0.0
        if isinstance(p, float) and p > 0:
            raise NotImplementedError(f"lwdetr_amd: attention-weight dropout p = {p} is not implemented in the fused forward")


def mlp_forward(mlp, x):
    """The reference's ``MLP.forward`` (transformer.py:37-39) over ``mlp.layers``."""
    n = len(mlp.layers)
    for i, layer in enumerate(mlp.layers):
        x = layer(x)
        if i < n - 1:
            x = F.relu(x)
    return x


def grouped_self_attention(self_attn, tgt, query_pos, groups, fused=None):
    """tgt, query_pos (B, groups * nq, d) -> out_proj(attention) (B, groups * nq, d); queries attend inside their own group only.
    ``groups = 1`` is the eval form."""
    B, Qt, d = tgt.shape
    G = int(groups)
    if Qt % G:
        raise RuntimeError(f"grouped_self_attention: {Qt} queries do not split into {G} groups")
    nq, heads = Qt // G, self_attn.num_heads
    hd = d // heads
    W, bias = self_attn.in_proj_weight, self_attn.in_proj_bias
    qk = F.linear(tgt + query_pos, W[:2 * d], None if bias is None else bias[:2 * d]).view(B * G, nq, 2, heads, hd)
    v = F.linear(tgt, W[2 * d:], None if bias is None else bias[2 * d:]).view(B * G, nq, heads, hd).permute(0, 2, 1, 3)
    q, k = qk[:, :, 0].permute(0, 2, 1, 3), qk[:, :, 1].permute(0, 2, 1, 3)
    scale = hd ** -0.5
    possible = tgt.is_cuda and qk.dtype in A._DTYPES and hd in A._HEAD_DIMS
    if _want(fused, possible, "grouped_self_attention"):
        o = A.fused_attention(q, k, v, scale)
    else:
        w = ((q * scale) @ k.transpose(-2, -1)).softmax(-1)
        o = (w @ v).transpose(1, 2).reshape(B * G, nq, d)
    return self_attn.out_proj(o.reshape(B, Qt, d))


def msda_core_torch(value, level_shapes, loc, aw):
    """value (B, S, M, D), loc (B, Q, M, L, P, 2) in (x, y), aw (B, Q, M, L, P) -> (B, Q, M * D): bilinear sampling with zero padding, one
    ``grid_sample`` per level (differentiable on every device and in float64)."""
    b, _, m, d = value.shape
    q = loc.shape[1]
    out, cur = 0, 0
    for lvl, (hl, wl) in enumerate(level_shapes):
        v = value[:, cur:cur + hl * wl].permute(0, 2, 3, 1).reshape(b * m, d, hl, wl)
        grid = (2 * loc[:, :, :, lvl] - 1).transpose(1, 2).flatten(0, 1)
        samp = F.grid_sample(v, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        w = aw[:, :, :, lvl].transpose(1, 2).reshape(b * m, 1, q, -1)
        out = out + (samp * w).sum(-1).view(b, m, d, q).permute(0, 3, 1, 2)
        cur += hl * wl
    return out.reshape(b, q, m * d)


def deformable_cross_attention(cross_attn, query, reference_points, memory, spatial_shapes, level_start_index, padding_mask=None, fused=None):
    """The forward of the reference's ``MSDeformAttn`` (ms_deform_attn.py:96-144) for 4-coordinate reference boxes (B, Q, L, 4)."""
    if reference_points.shape[-1] != 4:
        raise ValueError("lwdetr_amd implements the 4-coordinate (box) reference form used by LW-DETR (ms_deform_attn.py:125-127)")
    B, S, _ = memory.shape
    Q = query.shape[1]
    M, L, P = cross_attn.n_heads, cross_attn.n_levels, cross_attn.n_points
    value = cross_attn.value_proj(memory)
    value = value.view(B, S, M, value.shape[-1] // M)
    offsets, logits = cross_attn.sampling_offsets(query), cross_attn.attention_weights(query)
    possible = query.is_cuda and memory.is_cuda and DT.kernel_supports(M, value.shape[-1], L, P, value.dtype)
    if _want(fused, possible, "deformable_cross_attention"):
        core = DT.FusedMSDeformAttnFunction.apply(value, spatial_shapes, level_start_index, offsets, logits, reference_points, padding_mask)
    else:
        if padding_mask is not None:
            value = value.masked_fill(padding_mask.reshape(B, S, 1, 1), 0.0)
        ref = reference_points.to(value.dtype)
        off = offsets.view(B, Q, M, L, P, 2)
        loc = ref[:, :, None, :, None, :2] + off / P * ref[:, :, None, :, None, 2:] * 0.5
        aw = logits.view(B, Q, M, L * P).softmax(-1).view(B, Q, M, L, P)
        core = msda_core_torch(value, [tuple(s) for s in spatial_shapes.tolist()], loc, aw)
    return cross_attn.output_proj(core)


def decoder_layer_forward(layer, tgt, memory, query_pos, reference_points, spatial_shapes, level_start_index, padding_mask, groups, fused=None):
    """``TransformerDecoderLayer.forward_post`` (transformer.py:466-517) with dropout refused: -> tgt (B, Q, d)."""
    tgt = layer.norm1(tgt + grouped_self_attention(layer.self_attn, tgt, query_pos, groups, fused))
    tgt2 = deformable_cross_attention(layer.cross_attn, tgt + query_pos, reference_points, memory, spatial_shapes, level_start_index,
                                      padding_mask, fused)
    tgt = layer.norm2(tgt + tgt2)
    act = getattr(layer, "activation", F.relu)
    tgt2 = layer.linear2(act(layer.linear1(tgt)))
    return layer.norm3(tgt + tgt2)


def decoder_forward(decoder, tgt, memory, refpoints_unsigmoid, spatial_shapes, level_start_index, valid_ratios, padding_mask, groups,
                    fused=None):
    """``TransformerDecoder.forward`` (transformer.py:328-427) for ``lite_refpoint_refine`` + ``bbox_reparam`` without ``bbox_embed``:
    -> (hs (layers, B, Q, d), references (1, B, Q, 4)). valid_ratios (B, L, 2) or None (no padding: ratios of one)."""
    refuse_dropout(decoder)
    L = spatial_shapes.shape[0]
    obj_center = refpoints_unsigmoid[..., :4]
    if valid_ratios is None:
        refpoints_input = obj_center[:, :, None].expand(-1, -1, L, -1)
    else:
        refpoints_input = obj_center[:, :, None] * torch.cat([valid_ratios, valid_ratios], -1)[:, None]
    boxes = refpoints_input[:, :, 0, :]
    dim = decoder.d_model // 2
    if _want(fused, TG.sine_supports(boxes, dim), "query_sine_embed"):
        sine = TG.query_sine_embed(boxes, dim)
    else:
        sine = TG.query_sine_embed_torch(boxes, dim)
    query_pos = mlp_forward(decoder.ref_point_head, sine)
    output, hs = tgt, []
    for layer in decoder.layers:
        output = decoder_layer_forward(layer, output, memory, query_pos, refpoints_input, spatial_shapes, level_start_index, padding_mask,
                                       groups, fused)
        hs.append(decoder.norm(output))
    return torch.stack(hs), refpoints_unsigmoid.unsqueeze(0)


def _decoder_forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None, pos=None,
                     refpoints_unsigmoid=None, level_start_index=None, spatial_shapes=None, valid_ratios=None):
    if tgt_mask is not None or memory_mask is not None or tgt_key_padding_mask is not None:
        raise NotImplementedError("lwdetr_amd decoder: attention masks on the queries are not implemented (the reference passes none)")
    groups = getattr(self.layers[0], "group_detr", 1) if self.training else 1
    hs, refs = decoder_forward(self, tgt, memory, refpoints_unsigmoid, spatial_shapes, level_start_index, valid_ratios, memory_key_padding_mask,
                               groups)
    return [hs, refs]


def patch_decoder(transformer) -> int:
    """Rebinds ``forward`` of every sub-module of ``transformer`` that has ``layers``, ``norm``, ``ref_point_head``, ``lite_refpoint_refine``
    and ``bbox_reparam`` (the reference's ``TransformerDecoder``) and is in the published configuration - both flags set, ``bbox_embed`` None,
    intermediate outputs returned, not exported - to ``decoder_forward``; it uses the layers' ``group_detr`` groups when ``self.training``,
    else 1. Parameters and state-dict keys are untouched. Returns how many were patched; any other configuration is left alone (0)."""
    count = 0
    for m in transformer.modules():
        if not all(hasattr(m, a) for a in _DECODER_ATTRS):
            continue
        if not (m.lite_refpoint_refine and m.bbox_reparam) or getattr(m, "bbox_embed", None) is not None or m.norm is None:
            continue
        if not getattr(m, "return_intermediate", True) or getattr(m, "_export", False):
            continue
        m.forward = types.MethodType(_decoder_forward, m)
        count += 1
    return count
