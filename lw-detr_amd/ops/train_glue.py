"""The two GEMM-free pieces of the training forward that the reference runs as chains of small torch launches (``csrc/train_glue.hip``).

``layer_norm_2d``: the channels-first LayerNorm at the end of every projector stage (``models/backbone/projector.py:21-47``). The reference
runs mean, sub, pow, mean, sqrt, div, mul and add over an NCHW tensor and autograd keeps about four tensors of its size; its output is then
flattened, transposed and concatenated into ``memory``. ``LayerNorm2dFunction`` is one launch forward and two backward, saves ``x`` and two
f32 numbers per pixel, and with ``tokens=True`` writes the contiguous (B, H*W, C) rows ``memory`` is made of directly.

``query_sine_embed``: ``gen_sineembed_for_position`` (``models/transformer.py:42-68``) for 4-coordinate boxes: about twenty launches and every
(B, Q, dim / 2) intermediate kept, against one launch each way here that saves the boxes only.

No floating-point atomic: two calls give the same bits. CPU tensors and float64 raise inside the Functions; ``layer_norm_2d_torch`` and
``query_sine_embed_torch`` are the reference's formulations in torch, for callers that ask for them.
"""
import math
import types

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
LN2D_MAX_C, SINE_MAX_DIM = 1024, 256
_WORKSPACES = {}
_INV_TABLES = {}


def ln2d_supports(x) -> bool:
    return x.is_cuda and x.dtype in _DTYPES and x.dim() == 4 and 1 <= x.shape[1] <= LN2D_MAX_C and x.shape[0] >= 1 and x.shape[2] * x.shape[3] >= 1


def sine_supports(boxes, dim) -> bool:
    return (boxes.is_cuda and boxes.dtype in _DTYPES and boxes.dim() == 3 and boxes.shape[-1] == 4 and int(dim) == dim and 2 <= dim <= SINE_MAX_DIM
            and int(dim) % 2 == 0)


def _workspace(nfloats, device):
    """One buffer per (device, stream), grown when a call needs more."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nfloats:
        _WORKSPACES.pop(key, None)
        ws = None
        ws = _WORKSPACES[key] = torch.empty(max(int(nfloats), 1), dtype=torch.float32, device=device)
    return ws


# ------------------------------------------------------------------------------------------------------------------- LayerNorm2d
def layer_norm_2d_torch(x, weight, bias, eps, tokens=False):
    """The reference's formulation (projector.py:41-46), then the flatten / transpose of transformer.py:209 when ``tokens``."""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    y = (x - u) / torch.sqrt(s + eps)
    y = weight[:, None, None] * y + bias[:, None, None]
    return y.flatten(2).transpose(1, 2) if tokens else y


class LayerNorm2dFunction(Function):
    """``apply(x, weight, bias, eps, tokens)``: x (B, C, H, W) -> (B, C, H, W), or the contiguous (B, H*W, C) when ``tokens``. Saves x and the
    per-pixel mean and rstd in f32; the backward returns dx (NCHW), dw and db (per-workgroup partials, added in one fixed order)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, tokens):
        if not (x.is_cuda and weight.is_cuda and bias.is_cuda):
            raise RuntimeError("layer_norm_2d: tensors must live on a ROCm device (cuda:N); there is no CPU path")
        if x.dtype not in _DTYPES:
            raise RuntimeError(f"layer_norm_2d: dtype {x.dtype} is not supported (float32, float16, bfloat16)")
        if x.dim() != 4 or tuple(weight.shape) != (x.shape[1],) or tuple(bias.shape) != (x.shape[1],):
            raise RuntimeError("layer_norm_2d: x must be (B, C, H, W) and weight / bias (C,)")
        B, C, H, W = x.shape
        if not 1 <= C <= LN2D_MAX_C or B < 1 or H * W < 1:
            raise RuntimeError(f"layer_norm_2d: C = {C} is outside the kernel's range [1, {LN2D_MAX_C}] or the tensor is empty")
        x = x.detach().contiguous()
        w32, b32 = weight.detach().float().contiguous(), bias.detach().float().contiguous()
        dev, tokens = x.device, bool(tokens)
        y = torch.empty((B, H * W, C) if tokens else (B, C, H, W), dtype=x.dtype, device=dev)
        mean = torch.empty(B, H * W, dtype=torch.float32, device=dev)
        rstd = torch.empty(B, H * W, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = N.lib().lwdetr_ln2d_forward(x.data_ptr(), w32.data_ptr(), b32.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, C,
                                             H * W, float(eps), int(tokens), N.dtype_code(x.dtype), N.stream_ptr(dev))
        N.check(rc, "ln2d_forward")
        ctx.save_for_backward(x, w32, mean, rstd)
        ctx.tokens, ctx.param_dtypes = tokens, (weight.dtype, bias.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, w32, mean, rstd = ctx.saved_tensors
        B, C, H, W = x.shape
        dev = x.device
        grad_y = grad_y.to(x.dtype).contiguous()
        dx = torch.empty_like(x)
        dw = torch.empty(C, dtype=torch.float32, device=dev)
        db = torch.empty(C, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            nfl = N.lib().lwdetr_ln2d_workspace_floats(B, C, H * W)
            ws = _workspace(nfl, dev)
            rc = N.lib().lwdetr_ln2d_backward(x.data_ptr(), w32.data_ptr(), mean.data_ptr(), rstd.data_ptr(), grad_y.data_ptr(), dx.data_ptr(),
                                              dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nfl, B, C, H * W, int(ctx.tokens),
                                              N.dtype_code(x.dtype), N.stream_ptr(dev))
        N.check(rc, "ln2d_backward")
        return dx, dw.to(ctx.param_dtypes[0]), db.to(ctx.param_dtypes[1]), None, None


def layer_norm_2d(x, weight, bias, eps, tokens=False):
    """x (B, C, H, W) -> per pixel w_c (x - u) / sqrt(s + eps) + b_c with the biased variance over C. ``tokens=False`` returns NCHW,
    ``tokens=True`` the contiguous (B, H*W, C). A non-contiguous or channels-last x is made contiguous first. 1 <= C <= 1024."""
    return LayerNorm2dFunction.apply(x, weight, bias, eps, tokens)


def _layer_norm_2d_forward(self, x):
    return layer_norm_2d(x, self.weight, self.bias, self.eps, False)


def patch_layer_norm_2d(module) -> int:
    """Rebinds ``forward`` of every sub-module of ``module`` that has ``weight``, ``bias``, ``eps`` and a ``normalized_shape`` of length 1 and
    whose class is not ``nn.LayerNorm`` (the reference's channels-first ``LayerNorm`` of projector.py) to ``layer_norm_2d``, without importing
    the reference; parameters and state-dict keys are untouched. Returns how many were patched."""
    count = 0
    for m in module.modules():
        ns = getattr(m, "normalized_shape", None)
        if all(hasattr(m, a) for a in ("weight", "bias", "eps")) and ns is not None and len(ns) == 1 and not isinstance(m, nn.LayerNorm):
            m.forward = types.MethodType(_layer_norm_2d_forward, m)
            count += 1
    return count


# -------------------------------------------------------------------------------------------------------------------- sine embed
def sine_dim_t(dim, device=None):
    """The reference's float32 temperature row (transformer.py:46-47), computed as it computes it."""
    dim_t = torch.arange(int(dim), dtype=torch.float32, device=device)
    return 10000 ** (2 * (dim_t // 2) / dim)


def _inv_table(dim, device):
    """1 / dim_t as two float32 rows (high and low part of the float64 reciprocal of the reference's float32 dim_t), cached per device."""
    key = (int(dim), device)
    t = _INV_TABLES.get(key)
    if t is None:
        inv = 1.0 / sine_dim_t(dim).double()
        hi = inv.float()
        lo = (inv - hi.double()).float()
        t = _INV_TABLES[key] = torch.stack([hi, lo]).contiguous().to(device)
    return t


def query_sine_embed_torch(boxes, dim):
    """``gen_sineembed_for_position`` for (B, Q, 4) boxes: (B, Q, 4 * dim) in the block order y, x, w, h."""
    dim_t = sine_dim_t(dim, boxes.device)
    out = []
    for c in (1, 0, 2, 3):
        e = (boxes[:, :, c] * (2 * math.pi))[:, :, None] / dim_t
        out.append(torch.stack((e[:, :, 0::2].sin(), e[:, :, 1::2].cos()), dim=3).flatten(2))
    return torch.cat(out, dim=2)


def _box_rows(boxes):
    """boxes (B, Q, 4) as rows with one stride (elements): the tensor itself when the ABI takes its strides, else a packed copy."""
    b, q, _ = boxes.shape
    ld = boxes.stride(1) if q > 1 else (boxes.stride(0) if b > 1 else 4)
    ok = boxes.stride(2) == 1 and ld >= 4 and (b == 1 or q == 1 or boxes.stride(0) == q * boxes.stride(1))
    if not ok:
        boxes, ld = boxes.contiguous(), 4
    return boxes, ld


class SineEmbedFunction(Function):
    """``apply(boxes, dim)``: boxes (B, Q, 4), a row-strided view allowed -> (B, Q, 4 * dim). Saves the boxes only; the backward recomputes
    the argument and reduces the 4 * dim columns of a row in one wave, in a fixed order."""

    @staticmethod
    def forward(ctx, boxes, dim):
        if not boxes.is_cuda:
            raise RuntimeError("query_sine_embed: tensors must live on a ROCm device (cuda:N); there is no CPU path")
        if boxes.dtype not in _DTYPES:
            raise RuntimeError(f"query_sine_embed: dtype {boxes.dtype} is not supported (float32, float16, bfloat16)")
        if boxes.dim() != 3 or boxes.shape[-1] != 4:
            raise RuntimeError("query_sine_embed: boxes must be (B, Q, 4)")
        if int(dim) != dim or not 2 <= int(dim) <= SINE_MAX_DIM or int(dim) % 2:
            raise RuntimeError(f"query_sine_embed: dim = {dim} must be even and at most {SINE_MAX_DIM}")
        dim = int(dim)
        B, Q, _ = boxes.shape
        rows, ld = _box_rows(boxes.detach())
        dev = boxes.device
        inv = _inv_table(dim, dev)
        out = torch.empty(B, Q, 4 * dim, dtype=boxes.dtype, device=dev)
        with torch.cuda.device(dev):
            rc = N.lib().lwdetr_sine_embed_forward(rows.data_ptr(), ld, inv[0].data_ptr(), inv[1].data_ptr(), out.data_ptr(), B * Q, dim,
                                                   N.dtype_code(boxes.dtype), N.stream_ptr(dev))
        N.check(rc, "sine_embed_forward")
        ctx.save_for_backward(rows)
        ctx.ld, ctx.dim = ld, dim
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        rows, = ctx.saved_tensors
        B, Q, _ = rows.shape
        dev = rows.device
        inv = _inv_table(ctx.dim, dev)
        grad_out = grad_out.to(rows.dtype).contiguous()
        gb = torch.empty(B, Q, 4, dtype=rows.dtype, device=dev)
        with torch.cuda.device(dev):
            rc = N.lib().lwdetr_sine_embed_backward(rows.data_ptr(), ctx.ld, inv[0].data_ptr(), inv[1].data_ptr(), grad_out.data_ptr(),
                                                    gb.data_ptr(), B * Q, ctx.dim, N.dtype_code(rows.dtype), N.stream_ptr(dev))
        N.check(rc, "sine_embed_backward")
        return gb, None


def query_sine_embed(boxes, dim):
    """boxes (B, Q, 4) -> (B, Q, 4 * dim): block order y, x, w, h; inside a block element j is sin (even j) or cos (odd j) of
    boxes_c * 2 pi / 10000^(2 floor(j / 2) / dim). ``dim`` even, at most 256."""
    return SineEmbedFunction.apply(boxes, dim)
