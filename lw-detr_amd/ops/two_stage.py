"""Two-stage query selection of the reference's ``Transformer.forward`` under training (``models/transformer.py:224-264``).

The reference runs, per group and over ALL B * S encoder tokens, Linear -> LayerNorm -> class head -> row maximum -> top-k, the three-layer
box head and two gathers; autograd keeps every one of those activations 13 times although only ``num_queries`` rows per group go on.
``two_stage_select`` scores every token for all groups in one fused launch (``csrc/two_stage_train.hip``, nothing kept), takes the top-k with
``lwdetr_topk`` (descending, ties by ascending index - documented here, ``torch.topk`` leaves it open), gathers the winners with
``SelectRowsFunction`` and runs the heads on the selected rows only, as group-batched torch ops under autograd. The class head gets no gradient
through this block (its logits only decide the indices), and the gradient of ``memory`` is summed per row in ascending group order without
atomics: two calls give the same bits.
"""
import types

import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_ATTRS = ("enc_output", "enc_output_norm", "enc_out_class_embed", "enc_out_bbox_embed", "decoder", "group_detr", "num_queries", "two_stage",
          "bbox_reparam")
LN_EPS = 1e-5
MAX_GROUPS, MAX_CLASSES = 16, 384


def kernel_supports(d, ncls, G, dtype) -> bool:
    """The instantiated range of lwdetr_two_stage_scores (include/lwdetr_hip.h)."""
    return dtype in _DTYPES and d in (256, 384) and 1 <= ncls <= MAX_CLASSES and 1 <= G <= MAX_GROUPS


def _require_cuda(*tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("two-stage selection: tensors must live on a ROCm device (cuda:N); there is no CPU path")


def scores_torch(memory, rowvalid, W_eo, b_eo, ln_w, ln_b, W_cls, b_cls):
    """The formulation of lwdetr_two_stage_scores in torch, float32 arithmetic (float64 stays float64): what a configuration outside the
    kernel's range runs."""
    ct = torch.float64 if memory.dtype == torch.float64 else torch.float32
    x = memory.to(ct) * rowvalid.unsqueeze(-1).to(ct)
    out = []
    for g in range(W_eo.shape[0]):
        y = F.layer_norm(F.linear(x, W_eo[g].to(ct), b_eo[g].to(ct)), (x.shape[-1],), ln_w[g].to(ct), ln_b[g].to(ct), LN_EPS)
        out.append(F.linear(y, W_cls[g].to(ct), b_cls[g].to(ct)).amax(-1))
    return torch.stack(out).float()


@torch.no_grad()
def two_stage_scores(memory, rowvalid, W_eo, b_eo, ln_w, ln_b, W_cls, b_cls):
    """memory (B, S, d), rowvalid (B, S) bool, stacked weights (G, d, d), (G, d) x 3, (G, ncls, d), (G, ncls) in memory's dtype
    -> scores (G, B, S) float32: the class maximum of every token for every group. Invalid rows are scored as zero rows."""
    ws = (W_eo, b_eo, ln_w, ln_b, W_cls, b_cls)
    _require_cuda(memory, rowvalid, *ws)
    B, S, d = memory.shape
    G, ncls = W_cls.shape[0], W_cls.shape[1]
    if tuple(W_eo.shape) != (G, d, d) or any(tuple(t.shape) != (G, d) for t in (b_eo, ln_w, ln_b)) or tuple(W_cls.shape) != (G, ncls, d) \
            or tuple(b_cls.shape) != (G, ncls) or tuple(rowvalid.shape) != (B, S):
        raise RuntimeError("two-stage selection: inconsistent shapes")
    if any(t.dtype != memory.dtype for t in ws):
        raise RuntimeError("two-stage selection: memory and the stacked weights must share a dtype")
    if not kernel_supports(d, ncls, G, memory.dtype):
        return scores_torch(memory, rowvalid, *ws)
    mem = memory.detach()
    if mem.stride(2) != 1 or (B > 1 and S > 1 and mem.stride(0) != S * mem.stride(1)) or mem.data_ptr() % 16 != 0:
        mem = mem.contiguous()
    ld = mem.stride(1) if S > 1 else (mem.stride(0) if B > 1 else d)
    if ld < d or (ld * mem.element_size()) % 16 != 0:
        mem, ld = mem.contiguous(), d
    rv = rowvalid.reshape(B * S).to(torch.uint8)
    ws = [t.detach().contiguous() for t in ws]
    scores = torch.empty(G, B, S, dtype=torch.float32, device=memory.device)
    with torch.cuda.device(memory.device):
        rc = N.lib().lwdetr_two_stage_scores(mem.data_ptr(), ld, rv.data_ptr(), *[t.data_ptr() for t in ws], scores.data_ptr(), B * S, d, ncls, G,
                                             N.dtype_code(memory.dtype), N.stream_ptr(memory.device))
    N.check(rc, "two_stage_scores")
    return scores


@torch.no_grad()
def topk_rows(scores, k):
    """scores (G, B, S) float32 -> idx (G, B, k) int64 by lwdetr_topk: descending score, equal scores by ascending index."""
    _require_cuda(scores)
    G, B, S = scores.shape
    scores = scores.contiguous()
    idx = torch.empty(G, B, k, dtype=torch.int64, device=scores.device)
    with torch.cuda.device(scores.device):
        rc = N.lib().lwdetr_topk(scores.data_ptr(), G * B, S, k, idx.data_ptr(), None, N.DT_F32, N.stream_ptr(scores.device))
    N.check(rc, "topk")
    return idx


def select_rows_gather(memory, rowvalid_u8, idx, props):
    """-> x_sel (B, G, nq, d), props_sel (B, G, nq, 4) f32, inv (B, S, G) int32 (lwdetr_two_stage_gather)."""
    B, S, d = memory.shape
    G, nq = idx.shape[0], idx.shape[2]
    dev = memory.device
    x_sel = torch.empty(B, G, nq, d, dtype=memory.dtype, device=dev)
    p_sel = torch.empty(B, G, nq, 4, dtype=torch.float32, device=dev)
    inv = torch.empty(B, S, G, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = N.lib().lwdetr_two_stage_gather(memory.data_ptr(), d, rowvalid_u8.data_ptr(), props.data_ptr(), idx.data_ptr(), x_sel.data_ptr(),
                                             p_sel.data_ptr(), inv.data_ptr(), B, S, G, nq, d, N.dtype_code(memory.dtype), N.stream_ptr(dev))
    N.check(rc, "two_stage_gather")
    return x_sel, p_sel, inv


def select_rows_scatter(grad_x_sel, inv, rowvalid_u8):
    """-> grad_memory (B, S, d), every element written, groups added in ascending g (lwdetr_two_stage_scatter_backward)."""
    B, G, nq, d = grad_x_sel.shape
    S, dev = inv.shape[1], grad_x_sel.device
    gm = torch.empty(B, S, d, dtype=grad_x_sel.dtype, device=dev)
    with torch.cuda.device(dev):
        rc = N.lib().lwdetr_two_stage_scatter_backward(grad_x_sel.data_ptr(), inv.data_ptr(), rowvalid_u8.data_ptr(), gm.data_ptr(), B, S, G, nq,
                                                       d, N.dtype_code(grad_x_sel.dtype), N.stream_ptr(dev))
    N.check(rc, "two_stage_scatter_backward")
    return gm


class SelectRowsFunction(Function):
    """``apply(memory, rowvalid, idx, props=None)`` -> x_sel (B, G, nq, d) [, props_sel (B, G, nq, 4) f32 when props (B, S, 4) f32 is given].

    memory (B, S, d) f32 / f16 / bf16; rowvalid (B, S) bool; idx (G, B, nq) int64, distinct inside a (g, b). x_sel[b, g, q] =
    rowvalid ? memory[b, idx[g, b, q]] : 0. Saves idx's inverse table and rowvalid only; the backward writes every row of grad_memory as the
    f32 sum, in ascending g, of the gradients of the groups that selected it. props_sel is not differentiable."""

    @staticmethod
    def forward(ctx, memory, rowvalid, idx, props=None):
        _require_cuda(memory, rowvalid, idx)
        if memory.dtype not in _DTYPES or idx.dtype != torch.int64 or memory.dim() != 3 or idx.dim() != 3:
            raise RuntimeError("two-stage selection: memory (B, S, d) float32 / float16 / bfloat16 and idx (G, B, nq) int64")
        B, S, d = memory.shape
        if idx.shape[1] != B or tuple(rowvalid.shape) != (B, S):
            raise RuntimeError("two-stage selection: inconsistent shapes")
        with_props = props is not None
        if not with_props:
            props = torch.zeros(B, S, 4, dtype=torch.float32, device=memory.device)
        rv = rowvalid.reshape(B, S).to(torch.uint8).contiguous()
        x_sel, p_sel, inv = select_rows_gather(memory.detach().contiguous(), rv, idx.contiguous(), props.detach().float().contiguous())
        ctx.save_for_backward(inv, rv)
        ctx.with_props = with_props
        if with_props:
            ctx.mark_non_differentiable(p_sel)
            return x_sel, p_sel
        return x_sel

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_x_sel, *unused):
        inv, rv = ctx.saved_tensors
        return select_rows_scatter(grad_x_sel.contiguous(), inv, rv), None, None, None


def proposals(B, level_shapes, mask_flatten, device, unsigmoid):
    """Anchor proposals (B, S, 4) f32 and row validity (B, S) bool of ``gen_encoder_output_proposals`` (transformer.py:71-125) from Python-int
    level shapes: no device tensor is iterated, so nothing synchronises with the host. Invalid rows hold 0 (inf in the unsigmoid form)."""
    props, cur = [], 0
    for lvl, (hl, wl) in enumerate(level_shapes):
        hl, wl = int(hl), int(wl)
        gy, gx = torch.meshgrid(torch.arange(hl, dtype=torch.float32, device=device),
                                torch.arange(wl, dtype=torch.float32, device=device), indexing="ij")
        grid = torch.stack([gx, gy], -1)[None].expand(B, -1, -1, -1)
        if mask_flatten is None:
            scale = torch.tensor([wl, hl], dtype=torch.float32, device=device).view(1, 1, 1, 2)
        else:
            m = mask_flatten[:, cur:cur + hl * wl].view(B, hl, wl)
            scale = torch.stack([(~m[:, 0, :]).sum(1), (~m[:, :, 0]).sum(1)], 1).view(B, 1, 1, 2).float()
        grid = (grid + 0.5) / scale
        wh = torch.ones_like(grid) * 0.05 * (2.0 ** lvl)
        props.append(torch.cat([grid, wh], -1).view(B, -1, 4))
        cur += hl * wl
    props = torch.cat(props, 1)
    valid = ((props > 0.01) & (props < 0.99)).all(-1)
    if mask_flatten is not None:
        valid = valid & ~mask_flatten
    if unsigmoid:
        props = torch.log(props / (1 - props)).masked_fill(~valid.unsqueeze(-1), float("inf"))
    else:
        props = props.masked_fill(~valid.unsqueeze(-1), 0.0)
    return props, valid


def _stack(mods, groups, attr):
    return torch.stack([getattr(mods[g], attr) for g in range(groups)])


def two_stage_select(memory, mask_flatten, level_shapes, enc_output, enc_output_norm, enc_out_class_embed, enc_out_bbox_embed, num_queries,
                     groups, bbox_reparam, return_idx=False):
    """-> (refpoint_embed_ts, memory_ts, boxes_ts), shaped and ordered as ``transformer.py:257-264``: (B, groups * num_queries, 4 | d | 4),
    groups concatenated on dim 1, each group's rows in descending score (ties by ascending token index). memory (B, S, d) on a ROCm device;
    mask_flatten (B, S) bool (True = padding) or None; level_shapes a sequence of Python (h, w); the four module lists are the reference's
    (``enc_out_bbox_embed[g].layers`` a list of Linears). ``groups=1`` is the eval-mode behaviour. boxes_ts is un-sigmoided when
    ``bbox_reparam`` is false, as ``:242-243``; refpoint_embed_ts is boxes_ts.detach(). ``return_idx=True`` appends the selected token indices
    (groups, B, num_queries) int64."""
    _require_cuda(memory)
    B, S, d = memory.shape
    nq, G = int(num_queries), int(groups)
    if sum(int(h) * int(w) for h, w in level_shapes) != S:
        raise RuntimeError("two-stage selection: level_shapes do not add up to memory's rows")
    props, valid = proposals(B, level_shapes, mask_flatten, memory.device, unsigmoid=not bbox_reparam)
    W_eo, b_eo = _stack(enc_output, G, "weight"), _stack(enc_output, G, "bias")
    ln_w, ln_b = _stack(enc_output_norm, G, "weight"), _stack(enc_output_norm, G, "bias")
    eps = enc_output_norm[0].eps
    with torch.no_grad():
        W_cls, b_cls = _stack(enc_out_class_embed, G, "weight"), _stack(enc_out_class_embed, G, "bias")
        if eps == LN_EPS:
            scores = two_stage_scores(memory, valid, W_eo, b_eo, ln_w, ln_b, W_cls, b_cls)
        else:
            raise RuntimeError(f"two-stage selection: LayerNorm eps {eps} (the kernel and its torch formulation use {LN_EPS})")
        idx = topk_rows(scores, nq)
        del scores, W_cls, b_cls
    x_sel, p_sel = SelectRowsFunction.apply(memory, valid, idx, props)
    x = x_sel.transpose(0, 1).reshape(G, B * nq, d)
    y = torch.baddbmm(b_eo.unsqueeze(1), x, W_eo.transpose(1, 2))
    y = F.layer_norm(y, (d,), None, None, eps) * ln_w.unsqueeze(1) + ln_b.unsqueeze(1)
    h = y
    nl = len(enc_out_bbox_embed[0].layers)
    for i in range(nl):
        Wl = torch.stack([enc_out_bbox_embed[g].layers[i].weight for g in range(G)])
        bl = torch.stack([enc_out_bbox_embed[g].layers[i].bias for g in range(G)])
        h = torch.baddbmm(bl.unsqueeze(1), h, Wl.transpose(1, 2))
        if i < nl - 1:
            h = F.relu(h)
    p = p_sel.transpose(0, 1).reshape(G, B * nq, 4).to(memory.dtype)
    if bbox_reparam:
        boxes = torch.cat([h[..., :2] * p[..., 2:] + p[..., :2], h[..., 2:].exp() * p[..., 2:]], -1)
    else:
        boxes = h + p
    memory_ts = y.view(G, B, nq, d).transpose(0, 1).reshape(B, G * nq, d)
    boxes_ts = boxes.view(G, B, nq, 4).transpose(0, 1).reshape(B, G * nq, 4)
    out = (boxes_ts.detach(), memory_ts, boxes_ts)
    return out + (idx,) if return_idx else out


def _valid_ratio(mask):
    _, H, W = mask.shape
    vh, vw = torch.sum(~mask[:, :, 0], 1), torch.sum(~mask[:, 0, :], 1)
    return torch.stack([vw.float() / W, vh.float() / H], -1)


def _transformer_forward(self, srcs, masks, pos_embeds, refpoint_embed, query_feat):
    """``Transformer.forward`` (transformer.py:198-288) with the two-stage block replaced by ``two_stage_select``."""
    src_flatten, pos_flatten, level_shapes = [], [], []
    for src, pos in zip(srcs, pos_embeds):
        bs, _, h, w = src.shape
        level_shapes.append((h, w))
        src_flatten.append(src.flatten(2).transpose(1, 2))
        pos_flatten.append(pos.flatten(2).transpose(1, 2))
    memory = torch.cat(src_flatten, 1)
    pos_flatten = torch.cat(pos_flatten, 1)
    mask_flatten = valid_ratios = None
    if masks is not None:
        mask_flatten = torch.cat([m.flatten(1) for m in masks], 1)
        valid_ratios = torch.stack([_valid_ratio(m) for m in masks], 1)
    spatial_shapes = torch.as_tensor(level_shapes, dtype=torch.long, device=memory.device)
    level_start_index = torch.cat((spatial_shapes.new_zeros((1,)), spatial_shapes.prod(1).cumsum(0)[:-1]))
    groups = self.group_detr if self.training else 1
    refpoint_ts, memory_ts, boxes_ts = two_stage_select(memory, mask_flatten, level_shapes, self.enc_output, self.enc_output_norm,
                                                        self.enc_out_class_embed, self.enc_out_bbox_embed, self.num_queries, groups,
                                                        self.bbox_reparam)
    tgt = query_feat.unsqueeze(0).repeat(bs, 1, 1)
    refpoint_embed = refpoint_embed.unsqueeze(0).repeat(bs, 1, 1)
    if self.bbox_reparam:
        refpoint_embed = torch.cat([refpoint_embed[..., :2] * refpoint_ts[..., 2:] + refpoint_ts[..., :2],
                                    refpoint_embed[..., 2:].exp() * refpoint_ts[..., 2:]], -1)
    else:
        refpoint_embed = refpoint_embed + refpoint_ts
    hs, references = self.decoder(tgt, memory, memory_key_padding_mask=mask_flatten, pos=pos_flatten, refpoints_unsigmoid=refpoint_embed,
                                  level_start_index=level_start_index, spatial_shapes=spatial_shapes,
                                  valid_ratios=valid_ratios.to(memory.dtype) if valid_ratios is not None else None)
    return hs, references, memory_ts, boxes_ts if self.bbox_reparam else boxes_ts.sigmoid()


def patch_two_stage(transformer) -> int:
    """Rebinds ``forward`` of every sub-module of ``transformer`` (itself included) that has ``enc_output``, ``enc_output_norm``,
    ``enc_out_class_embed``, ``enc_out_bbox_embed``, ``decoder``, ``group_detr``, ``num_queries``, ``two_stage`` and ``bbox_reparam`` (the
    reference's ``Transformer`` once ``LWDETR.__init__`` has attached the two heads) and ``two_stage`` set, without importing the reference;
    parameters and state-dict keys are untouched. It uses ``group_detr`` groups when ``self.training``, else 1. Returns how many were patched;
    a ``two_stage=False`` module is left alone and counted as 0."""
    count = 0
    for m in transformer.modules():
        if all(hasattr(m, a) for a in _ATTRS) and m.two_stage:
            m.forward = types.MethodType(_transformer_forward, m)
            count += 1
    return count
