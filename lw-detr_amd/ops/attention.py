"""Differentiable fused attention for the reference's ViT under training (``models/backbone/vit.py:86-140``).

The reference materialises the (B, heads, N, N) score matrix and autograd keeps its softmax for the backward pass: 123 MB per image
and global block at 640 x 640 in f32. ``FusedAttentionFunction`` runs ``csrc/attention_train.hip`` instead: the forward saves one f32
log-sum-exp per row, the backward recomputes the weights, and nothing of size N x N is ever stored. The kernels read q, k and v as strided
views of the Linear's output and write the three gradients into one (B, N, 3, heads, hd) buffer, so nothing is permuted or copied around the
call. There is no eager fall-back: CPU tensors, f64 and head sizes outside {16, 32, 64} raise.
"""
import math
import types

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N

_HEAD_DIMS = (16, 32, 64)
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _strides(t):
    """(sb, sh, sn) in elements of a (B, heads, N, hd) view; a dimension of size 1 has no stride to speak of."""
    return tuple(0 if t.shape[i] == 1 else t.stride(i) for i in (0, 1, 2))


def _abi_ok(t) -> bool:
    """True when the C ABI takes this (B, heads, N, hd) view as it is: unit inner stride, 16-byte aligned base and strides."""
    esz = t.element_size()
    return t.stride(3) == 1 and t.data_ptr() % 16 == 0 and all((s * esz) % 16 == 0 and s >= 0 for s in _strides(t))


def _rows_ok(t) -> bool:
    """(B, N, C) addressed as one row-strided matrix of B * N rows."""
    esz = t.element_size()
    b, n, _ = t.shape
    return (t.stride(2) == 1 and t.data_ptr() % 16 == 0 and (t.stride(1) * esz) % 16 == 0 and (b == 1 or n == 1 or t.stride(0) == n * t.stride(1))
            and (n > 1 or b == 1 or (t.stride(0) * esz) % 16 == 0))


def _row_ld(t) -> int:
    b, n, c = t.shape
    return t.stride(1) if n > 1 else (t.stride(0) if b > 1 else c)


def _validate(q, k, v, scale):
    for t in (q, k, v):
        if not t.is_cuda:
            raise RuntimeError("fused attention: tensors must live on a ROCm device (cuda:N); there is no CPU path")
    if q.dtype not in _DTYPES:
        raise RuntimeError(f"fused attention: dtype {q.dtype} is not supported (float32, float16, bfloat16)")
    if k.dtype != q.dtype or v.dtype != q.dtype or q.shape != k.shape or q.shape != v.shape or q.dim() != 4:
        raise RuntimeError("fused attention: q, k and v must share one dtype and one (B, heads, N, hd) shape")
    if q.shape[3] not in _HEAD_DIMS:
        raise RuntimeError(f"fused attention: head size {q.shape[3]} is not supported (16, 32 or 64)")
    if min(q.shape) < 1:
        raise RuntimeError("fused attention: empty tensors are not supported")
    if not (math.isfinite(scale) and scale > 0):
        raise RuntimeError(f"fused attention: scale must be finite and positive, got {scale}")


def _desc(q, k, v, o, lse, scale):
    b, h, n, hd = q.shape
    d = N.AttnTrainDesc()
    d.q, d.k, d.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    (d.q_sb, d.q_sh, d.q_sn), (d.k_sb, d.k_sh, d.k_sn), (d.v_sb, d.v_sh, d.v_sn) = _strides(q), _strides(k), _strides(v)
    d.o, d.o_ld, d.lse = o.data_ptr(), _row_ld(o), lse.data_ptr()
    d.B, d.heads, d.N, d.hd, d.scale = b, h, n, hd, float(scale)
    return d


def attn_train_forward(q, k, v, scale, out=None):
    """q, k, v: (B, heads, N, hd) views the ABI accepts -> (o (B, N, heads*hd), lse (B, heads, N) f32). ``out`` may be a row-strided view."""
    b, h, n, hd = q.shape
    o = torch.empty(b, n, h * hd, dtype=q.dtype, device=q.device) if out is None else out
    lse = torch.empty(b, h, n, dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        rc = N.lib().lwdetr_attn_train_forward(_desc(q, k, v, o, lse, scale), N.dtype_code(q.dtype), N.stream_ptr(q.device))
    N.check(rc, "attn_train_forward")
    return o, lse


def attn_train_backward(q, k, v, o, lse, scale, d_o, dq, dk, dv):
    """Writes dq, dk, dv ((B, heads, N, hd) views the ABI accepts) from the forward's operands, its o and lse, and d_o (B, N, heads*hd)."""
    b, h, n, hd = q.shape
    code = N.dtype_code(q.dtype)
    nbytes = N.lib().lwdetr_attn_train_workspace_bytes(b, h, n, hd, code)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device) if nbytes else None
    with torch.cuda.device(q.device):
        rc = N.lib().lwdetr_attn_train_backward(_desc(q, k, v, o, lse, scale), d_o.data_ptr(), _row_ld(d_o), dq.data_ptr(), dk.data_ptr(),
                                                dv.data_ptr(), *[s for t in (dq, dk, dv) for s in (_strides(t)[0], _strides(t)[2], _strides(t)[1])],
                                                ws.data_ptr() if ws is not None else None, code, N.stream_ptr(q.device))
    N.check(rc, "attn_train_backward")


def _heads_view(qkv, i):
    return qkv[:, :, i].permute(0, 2, 1, 3)            # (B, heads, N, hd), no copy


class FusedAttentionFunction(Function):
    """``apply(qkv, scale)``: qkv (B, N, 3, heads, hd) -> softmax(scale q k^T) v as (B, N, heads*hd). Saves qkv, the output and one f32
    log-sum-exp per row; the backward returns one (B, N, 3, heads, hd) gradient."""

    @staticmethod
    def forward(ctx, qkv, scale):
        if qkv.dim() != 5 or qkv.shape[2] != 3:
            raise RuntimeError("FusedAttentionFunction: qkv must be (B, N, 3, heads, hd)")
        scale = float(scale)
        _validate(*(_heads_view(qkv, i) for i in range(3)), scale)
        if not all(_abi_ok(_heads_view(qkv, i)) for i in range(3)):
            qkv = qkv.contiguous()                      # an operand the ABI would refuse for alignment: one packed copy
        q, k, v = (_heads_view(qkv, i) for i in range(3))
        o, lse = attn_train_forward(q, k, v, scale)
        ctx.save_for_backward(qkv, o, lse)
        ctx.scale = scale
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        qkv, o, lse = ctx.saved_tensors
        if not _rows_ok(grad_out):
            grad_out = grad_out.contiguous()
        grad = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
        q, k, v = (_heads_view(qkv, i) for i in range(3))
        dq, dk, dv = (_heads_view(grad, i) for i in range(3))
        attn_train_backward(q, k, v, o, lse, ctx.scale, grad_out, dq, dk, dv)
        return grad, None


class _SeparateFunction(Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        o, lse = attn_train_forward(q, k, v, scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        q, k, v, o, lse = ctx.saved_tensors
        if not _rows_ok(grad_out):
            grad_out = grad_out.contiguous()
        dq, dk, dv = (torch.empty(t.shape, dtype=t.dtype, device=t.device) for t in (q, k, v))
        attn_train_backward(q, k, v, o, lse, ctx.scale, grad_out, dq, dk, dv)
        return dq, dk, dv, None


def fused_attention(q, k, v, scale):
    """The same for three separate (B, heads, N, hd) tensors or views (the decoder's self-attention has this shape): -> (B, N, heads*hd)."""
    scale = float(scale)
    _validate(q, k, v, scale)
    q, k, v = (t if _abi_ok(t) else t.contiguous() for t in (q, k, v))
    return _SeparateFunction.apply(q, k, v, scale)


def _attention_forward(self, x, mask=None):
    """qkv Linear -> fused attention -> proj Linear; the forward that ``Attention`` and ``patch_vit_attention`` share."""
    b, n, c = x.shape
    if getattr(self, "use_cae", False):
        bias = torch.cat((self.q_bias, torch.zeros_like(self.v_bias), self.v_bias))
        qkv = F.linear(x, self.qkv.weight, bias)
    else:
        qkv = self.qkv(x)
    heads = self.num_heads
    qkv = qkv.reshape(b, n, 3, heads, c // heads)
    if mask is None:
        y = FusedAttentionFunction.apply(qkv, self.scale)
    else:                                               # the ViT never passes one (vit.py:361): the materialised formulation, in torch
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
        w = (q * self.scale) @ k.transpose(-2, -1)
        w = w.masked_fill(mask.reshape(b, 1, 1, n).expand_as(w), float("-inf")).softmax(dim=-1)
        y = (w @ v).transpose(1, 2).reshape(b, n, c)
    return self.proj(y)


class Attention(nn.Module):
    """Drop-in for the reference's ViT ``Attention`` (``vit.py:86-140``): the same parameters and state-dict keys (``qkv``, ``proj``, and with
    ``use_cae`` ``q_bias`` / ``v_bias``), the attention core in HIP."""

    def __init__(self, dim, num_heads=8, qkv_bias=True, use_cae=False):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.use_cae = use_cae
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias and not use_cae)
        if use_cae:
            self.q_bias = nn.Parameter(torch.zeros(dim))
            self.v_bias = nn.Parameter(torch.zeros(dim))
        self.proj = nn.Linear(dim, dim)

    forward = _attention_forward


def patch_vit_attention(module) -> int:
    """Rebinds ``forward`` of every sub-module of ``module`` that has ``qkv``, ``proj``, ``num_heads`` and ``scale`` attributes (the
    reference's ViT attention) to the fused path, without importing the reference. Returns how many were patched."""
    count = 0
    for m in module.modules():
        if all(hasattr(m, a) for a in ("qkv", "proj", "num_heads", "scale")):
            m.forward = types.MethodType(_attention_forward, m)
            count += 1
    return count
