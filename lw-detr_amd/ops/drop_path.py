"""Stochastic depth on the residuals of a ViT block under training (``csrc/drop_path.hip``).

The reference's block (``models/backbone/vit.py:216-220``) is ``x + drop_path(gamma * branch)`` with timm's ``DropPath``: one Bernoulli value per
entry of the first dimension of ``x`` - at that point (B * 16, h * w, C), so the unit that is dropped is a WINDOW, one sixteenth of an image -
divided by the keep probability and multiplied in. In torch that is three launches per residual (``gamma * y``, ``* t``, ``x +``) and autograd
keeps two tensors of the size of ``x`` (``y`` and ``gamma * y``). ``DropPathResidualFunction`` is one launch forward, saves ``y`` alone (and
that only when ``gamma`` wants a gradient), and its backward is one launch for ``grad_y`` and the per-workgroup partials of ``grad_gamma`` plus
a small one that adds them in a fixed order; ``grad_x`` is ``grad_out`` itself.

``drop_path_keep`` is the draw exactly as timm makes it, so the default generator is consumed as the reference consumes it;
``drop_path_residual_torch`` is the reference's formulation in torch (any device, float64 included). In float32 the fused forward and
``grad_y`` are the torch formulation's bits. A dropped window copies ``x`` and does not read ``y``: a non-finite ``y`` in a dropped window does
not propagate, where the reference's ``NaN * 0`` would. CPU tensors and float64 raise inside the Function.
"""
import contextlib
import functools

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N
from .train_glue import _workspace

DROP_PATH_MAX_C = 2048
_PAIRS = {(torch.float32, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16),
          (torch.float32, torch.bfloat16)}


def drop_path_supports(x, y, gamma=None) -> bool:
    """Whether the fused form serves: device, shapes, dtype pair, C, and - the fused result is in x's dtype - that torch's promotion of
    x + gamma * y gives x's dtype too (a 16-bit x beside an f32 gamma promotes to f32 in torch: that call stays with torch)."""
    if gamma is not None and torch.promote_types(x.dtype, torch.result_type(gamma, y)) != x.dtype:
        return False
    return (x.is_cuda and y.is_cuda and x.dim() == 3 and x.shape == y.shape and (x.dtype, y.dtype) in _PAIRS and 1 <= x.shape[2] <= DROP_PATH_MAX_C)


def drop_path_keep(like, rows, drop_prob):
    """The draw of timm's ``DropPath`` for ``rows`` units: ``like.new_empty((rows, 1, 1)).bernoulli_(1 - drop_prob)`` on ``like``'s device and
    in its dtype (the default generator advances as in the reference) -> bool (rows,), True where the unit is kept."""
    return like.new_empty((rows, 1, 1)).bernoulli_(1 - drop_prob).reshape(rows) != 0


def _branch_dtype(y, gamma):
    return y.dtype if gamma is None else torch.result_type(gamma, y)


def drop_path_residual_torch(x, y, gamma, keep, drop_prob):
    """The reference's formulation: ``x + (gamma * y) * t``, ``t = keep / (1 - drop_prob)`` in the branch's dtype, one value per entry of the
    first dimension. ``gamma`` None is ``x + y * t``."""
    branch = y if gamma is None else gamma * y
    t = keep.to(branch.dtype).div_(1 - drop_prob).view(-1, 1, 1)
    return x + branch * t


_NULL = contextlib.nullcontext()


def _on(dev):
    """The device guard of a native call: nothing to switch (and nothing to pay) when ``dev`` is the current device already."""
    return _NULL if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


@functools.lru_cache(maxsize=64)
def _workspace_floats(rows, c):
    return N.lib().lwdetr_drop_path_workspace_floats(rows, c)


def _rows(t):
    """t (B', N, C) as rows with one stride (elements): the tensor itself when the ABI takes its strides, else a packed copy."""
    b, n, c = t.shape
    if t.is_contiguous():
        return t, c
    ld = t.stride(1) if n > 1 else (t.stride(0) if b > 1 else c)
    ok = t.stride(2) == 1 and ld >= c and (b == 1 or n == 1 or t.stride(0) == n * t.stride(1))
    if not ok:
        t, ld = t.contiguous(), c
    return t, ld


class DropPathResidualFunction(Function):
    """``apply(x, y, gamma, keep, drop_prob)``: x, y (B', N, C) (row-strided views allowed), gamma (C,) or None, keep bool (B',) ->
    x + (gamma * y) * keep / (1 - drop_prob), contiguous, in x's dtype. Saves y (when gamma wants a gradient), gamma as f32 and the f32 scale."""

    @staticmethod
    def forward(ctx, x, y, gamma, keep, drop_prob):
        if not (x.is_cuda and y.is_cuda and keep.is_cuda and (gamma is None or gamma.is_cuda)):
            raise RuntimeError("drop_path_residual: tensors must live on a ROCm device (cuda:N); there is no CPU path")
        if (x.dtype, y.dtype) not in _PAIRS:
            raise RuntimeError(f"drop_path_residual: dtypes ({x.dtype}, {y.dtype}) are not supported (float32, float16, bfloat16, or a float32 x "
                               "with a 16-bit y)")
        if x.dim() != 3 or x.shape != y.shape or tuple(keep.shape) != (x.shape[0],) or keep.dtype != torch.bool:
            raise RuntimeError("drop_path_residual: x and y must be (B', N, C) and keep a bool (B',)")
        B, n, c = x.shape
        if not 1 <= c <= DROP_PATH_MAX_C or (gamma is not None and tuple(gamma.shape) != (c,)):
            raise RuntimeError(f"drop_path_residual: C = {c} is outside the kernel's range [1, {DROP_PATH_MAX_C}] or gamma is not (C,)")
        if not 0.0 <= drop_prob < 1.0:
            raise RuntimeError(f"drop_path_residual: drop_prob = {drop_prob} is outside [0, 1)")
        dev = x.device
        xr, ldx = _rows(x.detach())
        yr, ldy = _rows(y.detach())
        g32 = None if gamma is None else gamma.detach().float().contiguous()
        scale = keep.to(_branch_dtype(y, gamma)).div_(1 - drop_prob).float().contiguous()
        out = torch.empty((B, n, c), dtype=x.dtype, device=dev)
        if B * n > 0:
            with _on(dev):
                rc = N.lib().lwdetr_drop_path_forward(xr.data_ptr(), ldx, yr.data_ptr(), ldy, None if g32 is None else g32.data_ptr(),
                                                      scale.data_ptr(), out.data_ptr(), c, B * n, c, n, N.dtype_code(x.dtype),
                                                      N.dtype_code(y.dtype), N.stream_ptr(dev))
            N.check(rc, "drop_path_forward")
        want_gamma = gamma is not None and ctx.needs_input_grad[2]
        ctx.save_for_backward(yr if want_gamma else None, g32, scale)
        ctx.ldy, ctx.dims, ctx.dtypes = ldy, (B, n, c), (x.dtype, y.dtype, None if gamma is None else gamma.dtype)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        yr, g32, scale = ctx.saved_tensors
        B, n, c = ctx.dims
        dx, dy, dg = ctx.dtypes
        need_x, need_y, need_g = ctx.needs_input_grad[:3]
        need_g = need_g and g32 is not None
        dev = grad_out.device
        grad_out = grad_out.to(dx)
        grad_y = grad_gamma = None
        if need_y or need_g:
            gr, ldg = _rows(grad_out)
            if need_y:
                grad_y = torch.empty((B, n, c), dtype=dy, device=dev)
            if need_g:
                grad_gamma = torch.zeros(c, dtype=torch.float32, device=dev) if B * n == 0 else torch.empty(c, dtype=torch.float32, device=dev)
            if B * n > 0:
                with _on(dev):
                    nfl = _workspace_floats(B * n, c) if need_g else 0
                    ws = _workspace(nfl, dev) if need_g else None
                    rc = N.lib().lwdetr_drop_path_backward(gr.data_ptr(), ldg, yr.data_ptr() if need_g else None, ctx.ldy,
                                                           None if g32 is None else g32.data_ptr(), scale.data_ptr(),
                                                           grad_y.data_ptr() if need_y else None, c, grad_gamma.data_ptr() if need_g else None,
                                                           ws.data_ptr() if need_g else None, nfl, B * n, c, n, N.dtype_code(dx),
                                                           N.dtype_code(dy), N.stream_ptr(dev))
                N.check(rc, "drop_path_backward")
            if need_g:
                grad_gamma = grad_gamma.to(dg)
        return grad_out if need_x else None, grad_y, grad_gamma, None, None


def drop_path_residual(x, y, gamma, keep, drop_prob):
    """x, y (B', N, C), gamma (C,) f32-convertible or None, keep bool (B',) from ``drop_path_keep`` -> x + (gamma * y) * keep / (1 - drop_prob):
    unit b of the first dimension is dropped as a whole. 1 <= C <= 2048; (x, y) dtypes equal, or a float32 x with a 16-bit y."""
    return DropPathResidualFunction.apply(x, y, gamma, keep, drop_prob)
