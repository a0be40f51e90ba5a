"""Differentiable deformable cross-attention for the reference's decoder under training (``models/ops/modules/ms_deform_attn.py:96-144``).

The reference builds ``sampling_locations`` (B, Q, M, L, P, 2) and the softmaxed weights in torch and autograd keeps them;
``MSDeformAttnFunction`` differentiates in f32 / f64 only and scatters ``grad_value`` with atomics. ``FusedMSDeformAttnFunction`` runs
``csrc/msda_train.hip`` instead: it takes the outputs of the ``sampling_offsets`` and ``attention_weights`` Linears and the per-level reference
boxes as they are, does the location arithmetic and the softmax in the kernel, saves nothing beyond its inputs, works in f32, f16 and bf16
(f32 arithmetic, one rounding per output element), returns the gradient of the reference boxes as well, and uses no floating-point atomic:
two calls give the same bits, ``grad_value`` included. CPU tensors raise; there is no eager fall-back inside the Function.
"""
import types

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N
from .modules import MSDeformAttn as _InferenceModule

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_ATTRS = ("sampling_offsets", "attention_weights", "value_proj", "output_proj", "n_heads", "n_levels", "n_points")
_WORKSPACES = {}


def kernel_supports(M, D, L, P, dtype) -> bool:
    """The instantiated range of lwdetr_msda_train_forward / _backward (include/lwdetr_hip.h)."""
    return dtype in _DTYPES and D % 8 == 0 and 8 <= D <= 64 and 1 <= L <= 4 and P in (1, 2, 4, 8) and L * P <= 16 and 1 <= M <= 256


def _rows(t, rows, width):
    """t (B, Q, ...) as a (rows, width) matrix with a leading dimension: the tensor itself when it is a column view of a Linear's output (unit
    element stride, one row stride of at least `width` for all B * Q rows), a packed copy otherwise - an expanded or overlapping view (row
    stride 0 or below `width`) among them, whose storage does not hold rows * ld elements."""
    try:
        r = t.view(t.shape[0], t.shape[1], width)
    except RuntimeError:
        r = t.reshape(t.shape[0], t.shape[1], width).contiguous()
    b, q, _ = r.shape
    ld = r.stride(1) if q > 1 else (r.stride(0) if b > 1 else width)
    ok = (r.stride(2) == 1 and ld >= width and (b == 1 or q == 1 or r.stride(0) == q * r.stride(1))
          and r.data_ptr() % r.element_size() == 0)
    if not ok:
        r, ld = r.contiguous(), width
    return r, ld


def _value_view(value):
    """(B, S, M, D) with unit channel stride, heads packed, one row stride, 16-byte aligned base and rows - or a packed copy."""
    b, s, m, d = value.shape
    esz = value.element_size()
    ok = (value.stride(3) == 1 and (m == 1 or value.stride(2) == d) and (b == 1 or s == 1 or value.stride(0) == s * value.stride(1))
          and value.data_ptr() % 16 == 0)
    ld = value.stride(1) if s > 1 else (value.stride(0) if b > 1 else m * d)
    if not ok or ld < m * d or (ld * esz) % 16 != 0:
        value = value.contiguous()
        ld = m * d
    return value, ld


def _workspace(nbytes, device):
    """One buffer per (device, stream), grown when a call needs more: a last short batch or another query count reuses it."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        _WORKSPACES.pop(key, None)
        ws = None                                           # the smaller buffer is released before the larger one is allocated
        ws = _WORKSPACES[key] = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.float32, device=device)
    return ws


class _Operands:
    """The operands of one call as the C ABI takes them (views where the ABI accepts the caller's strides, packed copies otherwise)."""

    def __init__(self, value, spatial_shapes, level_start_index, offsets, logits, reference_boxes, padding_mask=None):
        tensors = [value, spatial_shapes, level_start_index, offsets, logits, reference_boxes] + ([] if padding_mask is None else [padding_mask])
        if not all(t.is_cuda for t in tensors):
            raise RuntimeError("fused deformable attention: tensors must live on a ROCm device (cuda:N); there is no CPU path")
        if value.dim() != 4 or reference_boxes.dim() != 4 or reference_boxes.shape[-1] != 4:
            raise RuntimeError("fused deformable attention: value must be (B, S, M, D) and reference_boxes (B, Q, L, 4)")
        if offsets.dtype != value.dtype or logits.dtype != value.dtype:
            raise RuntimeError("fused deformable attention: value, offsets and logits must share a dtype")
        if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
            raise RuntimeError("fused deformable attention: spatial_shapes / level_start_index must be int64")
        b, s, m, d = value.shape
        q, L = reference_boxes.shape[1], spatial_shapes.shape[0]
        width = logits.numel() // max(b * q, 1)
        P = width // max(m * L, 1)
        if tuple(reference_boxes.shape[:3]) != (b, q, L) or width != m * L * P or offsets.numel() != b * q * 2 * width or min(b, s, q, P) < 1:
            raise RuntimeError("fused deformable attention: inconsistent shapes")
        if not kernel_supports(m, d, L, P, value.dtype):
            raise RuntimeError(f"fused deformable attention: M={m} D={d} L={L} P={P} {value.dtype} is outside the kernel's range "
                               "(D % 8 == 0, D <= 64, L <= 4, P in {1, 2, 4, 8}, L * P <= 16, float32 / float16 / bfloat16)")
        self.value, self.ld_v = _value_view(value)
        self.off, self.ld_off = _rows(offsets, b * q, 2 * width)
        self.lg, self.ld_lg = _rows(logits, b * q, width)
        self.ref = reference_boxes.detach().float().contiguous()
        self.mask = None if padding_mask is None else padding_mask.reshape(b, s).contiguous().view(torch.uint8)
        self.shapes, self.lsi = spatial_shapes.contiguous(), level_start_index.contiguous()
        self.dims = (b, s, m, d, L, q, P)

    def desc(self):
        d = N.MsdaTrainDesc()
        d.value, d.value_ld, d.offsets, d.offsets_ld = self.value.data_ptr(), self.ld_v, self.off.data_ptr(), self.ld_off
        d.logits, d.logits_ld, d.ref = self.lg.data_ptr(), self.ld_lg, self.ref.data_ptr()
        d.mask = self.mask.data_ptr() if self.mask is not None else None
        d.shapes, d.level_start = self.shapes.data_ptr(), self.lsi.data_ptr()
        d.B, d.S, d.M, d.D, d.L, d.Q, d.P = self.dims
        d.dtype = N.dtype_code(self.value.dtype)
        return d

    def tensors(self):
        return [self.value, self.off, self.lg, self.ref, self.shapes, self.lsi] + ([] if self.mask is None else [self.mask])


def msda_train_forward(ops, out=None):
    """-> out (B, Q, M*D), contiguous, in the input dtype (`out` may be given: contiguous, 16-byte aligned)."""
    b, s, m, d, L, q, P = ops.dims
    dev = ops.value.device
    if out is None:
        out = torch.empty(b, q, m * d, dtype=ops.value.dtype, device=dev)
    with torch.cuda.device(dev):
        rc = N.lib().lwdetr_msda_train_forward(ops.desc(), out.data_ptr(), N.stream_ptr(dev))
    N.check(rc, "msda_train_forward")
    return out


def msda_train_backward(ops, grad_out, grad_value=None, grad_offsets=None, grad_logits=None, grad_ref=None):
    """-> grad_value (B, S, M, D), grad_offsets (B*Q, M*L*P*2), grad_logits (B*Q, M*L*P) in the input dtype, grad_ref (B, Q, L, 4) f32; all
    contiguous, every element written. grad_out (B, Q, M*D) contiguous."""
    b, s, m, d, L, q, P = ops.dims
    dev, dt = ops.value.device, ops.value.dtype
    gv = torch.empty(b, s, m, d, dtype=dt, device=dev) if grad_value is None else grad_value
    g_off = torch.empty(b * q, m * L * P * 2, dtype=dt, device=dev) if grad_offsets is None else grad_offsets
    g_lg = torch.empty(b * q, m * L * P, dtype=dt, device=dev) if grad_logits is None else grad_logits
    g_ref = torch.empty(b, q, L, 4, dtype=torch.float32, device=dev) if grad_ref is None else grad_ref
    desc = ops.desc()
    with torch.cuda.device(dev):
        nbytes = N.lib().lwdetr_msda_train_workspace_bytes(desc)
        ws = _workspace(nbytes, dev)
        rc = N.lib().lwdetr_msda_train_backward(desc, grad_out.data_ptr(), gv.data_ptr(), g_off.data_ptr(), g_lg.data_ptr(), g_ref.data_ptr(),
                                                ws.data_ptr(), nbytes, N.stream_ptr(dev))
    N.check(rc, "msda_train_backward")
    return gv, g_off, g_lg, g_ref


class FusedMSDeformAttnFunction(Function):
    """``apply(value, spatial_shapes, level_start_index, offsets, logits, reference_boxes, padding_mask=None)`` -> (B, Q, M*D).

    value (B, S, M, D); spatial_shapes (L, 2) / level_start_index (L,) int64 on the device; offsets (B, Q, M*L*P*2) and logits (B, Q, M*L*P)
    (any trailing shape with these widths), the raw outputs of the two Linears; reference_boxes (B, Q, L, 4) = (cx, cy, w, h) per level, f32 or
    the input dtype; padding_mask (B, S) bool, True = padding. Gradients for value, offsets, logits and reference_boxes."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, offsets, logits, reference_boxes, padding_mask=None):
        ops = _Operands(value, spatial_shapes, level_start_index, offsets, logits, reference_boxes, padding_mask)
        out = msda_train_forward(ops)
        ctx.save_for_backward(*ops.tensors())
        ctx.ops = (ops.ld_v, ops.ld_off, ops.ld_lg, ops.dims, ops.mask is not None)
        ctx.shapes_out = (offsets.shape, logits.shape, reference_boxes.dtype)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        ops = _Operands.__new__(_Operands)
        ops.value, ops.off, ops.lg, ops.ref, ops.shapes, ops.lsi, *rest = ctx.saved_tensors
        ops.ld_v, ops.ld_off, ops.ld_lg, ops.dims, has_mask = ctx.ops
        ops.mask = rest[0] if has_mask else None
        grad_out = grad_out.contiguous()
        if grad_out.data_ptr() % 16 != 0:                   # a contiguous slice of an upstream buffer: the ABI wants 16-byte alignment
            grad_out = grad_out.clone()
        gv, g_off, g_lg, g_ref = msda_train_backward(ops, grad_out)
        off_shape, lg_shape, ref_dtype = ctx.shapes_out
        return gv, None, None, g_off.view(off_shape), g_lg.view(lg_shape), g_ref.to(ref_dtype), None


def torch_formulation(value, spatial_shapes, level_start_index, offsets, logits, reference_boxes, padding_mask, n_points, im2col_step=64):
    """The reference's own arithmetic in torch (``ms_deform_attn.py:114-131``) + ``MSDeformAttnFunction``, in float32 (float64 stays float64):
    what a configuration outside the fused kernel's range runs, and what the fused path is measured against."""
    from .functions import MSDeformAttnFunction
    b, s, m, d = value.shape
    q, L = reference_boxes.shape[1], spatial_shapes.shape[0]
    ct = torch.float64 if value.dtype == torch.float64 else torch.float32
    v = value.to(ct)
    if padding_mask is not None:
        v = v.masked_fill(padding_mask.reshape(b, s, 1, 1), 0.0)
    off = offsets.to(ct).reshape(b, q, m, L, n_points, 2)
    ref = reference_boxes.to(ct)
    loc = ref[:, :, None, :, None, :2] + off / n_points * ref[:, :, None, :, None, 2:] * 0.5
    aw = logits.to(ct).reshape(b, q, m, L * n_points).softmax(-1).reshape(b, q, m, L, n_points)
    out = MSDeformAttnFunction.apply(v.contiguous(), spatial_shapes.contiguous(), level_start_index.contiguous(), loc.contiguous(),
                                     aw.contiguous(), im2col_step if b % im2col_step == 0 else b)
    return out.to(value.dtype)


def _deform_forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index, input_padding_mask=None):
    """value / offsets / logits Linears -> fused deformable attention -> output Linear; shared by ``MSDeformAttnTrain`` and
    ``patch_deformable_attention``."""
    if not (query.is_cuda and input_flatten.is_cuda and reference_points.is_cuda):
        raise RuntimeError("fused deformable attention: tensors must live on a ROCm device (cuda:N); there is no CPU path")
    if reference_points.shape[-1] != 4:
        raise ValueError("lwdetr_amd MSDeformAttnTrain implements the 4-coordinate (box) reference form used by LW-DETR "
                         "(ms_deform_attn.py:125-127)")
    n, s, _ = input_flatten.shape
    m, L, P = self.n_heads, self.n_levels, self.n_points
    value = self.value_proj(input_flatten)
    value = value.view(n, s, m, value.shape[-1] // m)
    offsets, logits = self.sampling_offsets(query), self.attention_weights(query)
    if kernel_supports(m, value.shape[-1], L, P, value.dtype):
        core = FusedMSDeformAttnFunction.apply(value, input_spatial_shapes, input_level_start_index, offsets, logits, reference_points,
                                               input_padding_mask)
    else:
        core = torch_formulation(value, input_spatial_shapes, input_level_start_index, offsets, logits, reference_points, input_padding_mask, P)
    return self.output_proj(core)


class MSDeformAttnTrain(nn.Module):
    """Trainable drop-in for the reference's ``MSDeformAttn`` (``ms_deform_attn.py:37-144``): the same parameters, state-dict keys,
    initialisation and forward contract; its four Linears are plain ``nn.Linear`` and the core between them is ``FusedMSDeformAttnFunction``.
    ``reference_points`` must be the 4-coordinate box form (a 2-coordinate one raises ``ValueError``, as the inference module does). A
    configuration the kernel refuses - head width not a multiple of 8 or above 64, more than 4 levels, n_points outside {1, 2, 4, 8}, n_levels * n_points > 16 (the
    reference's own defaults, 4 x 4, fit), float64 - takes the torch formulation + ``MSDeformAttnFunction`` in float32 (float64
    for float64 inputs), which keeps the locations and weights for autograd and scatters ``grad_value`` with atomics."""

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError(f"d_model must be divisible by n_heads, but got {d_model} and {n_heads}")
        self.im2col_step = 64
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)
        self._reset_parameters()

    _reset_parameters = _InferenceModule._reset_parameters
    forward = _deform_forward


def patch_deformable_attention(module) -> int:
    """Rebinds ``forward`` of every sub-module of ``module`` that has ``sampling_offsets``, ``attention_weights``, ``value_proj``,
    ``output_proj``, ``n_heads``, ``n_levels`` and ``n_points`` (the reference's ``MSDeformAttn``) to the fused path, without importing the
    reference; parameters and state-dict keys are untouched. Returns how many were patched."""
    count = 0
    for m in module.modules():
        if all(hasattr(m, a) for a in _ATTRS):
            m.forward = types.MethodType(_deform_forward, m)
            count += 1
    return count
