"""Training criterion behind the reference's interface (``models/matcher.py``, ``models/lwdetr.py:218-506``):
``GroupHungarianMatcher`` and ``TrainSetCriterion`` - grouped matching (``group_detr``), the four classification loss forms
(sigmoid focal, IA-BCE, varifocal, position-supervised) and their gradients, with no host synchronisation.

A forward call is four launches for all layers (final, aux 0..n, enc) together: the cost matrices of ``csrc/match.hip``, then
from ``csrc/match_train.hip`` the assignment (one wave per (layer, image, group) problem), the per-chunk loss partials and the
finish. The backward pass is one more launch for all layers. The whole criterion is one ``torch.autograd.Function`` from
the logits and boxes of every layer to the ``(layers, 5)`` tensor of loss values.

The evaluation-only pair ``criterion.HungarianMatcher`` / ``criterion.SetCriterion`` is untouched by this module.
"""
from collections import OrderedDict

import torch
from torch import nn

from .. import _native
from .._native import NativeError
from .criterion import _LOSS_KEYS, _Packed, _layer_array

_GRAD_ROWS = (0, 2, 3)                                     # loss_ce, loss_bbox, loss_giou of the (layers, 5) output


class _TrainWorkspace:
    """Device buffers of one (shape, groups): ``cap`` packed targets fit. Kept by the matcher across the asynchronous launches."""

    def __init__(self, dev, layers, b, nq, groups, cap):
        self.cap = cap
        self.cost = torch.empty(layers * cap * nq, dtype=torch.float32, device=dev)
        self.idx_q = torch.zeros(layers * groups * cap, dtype=torch.int64, device=dev)
        self.idx_t = torch.zeros(layers * groups * cap, dtype=torch.int64, device=dev)
        self.status = torch.zeros(layers, b, groups, dtype=torch.int32, device=dev)
        self.steps = torch.zeros(layers, b, groups, dtype=torch.int32, device=dev)
        self.partials = torch.empty(max(1, _native.lib().lwdetr_criterion_partials_floats(layers, b, nq)), dtype=torch.float32, device=dev)


def _check_groups(targets, nq, groups):
    """The limits of the grouped solver, refused before anything is launched."""
    if groups < 1:
        raise ValueError(f"group_detr must be >= 1, got {groups}")
    if nq % groups:
        raise ValueError(f"num_queries = {nq} is not divisible by group_detr = {groups}")
    gw = nq // groups
    if gw > _native.MATCH_MAX_NQ:
        raise NativeError(f"lwdetr_amd: the native matcher supports at most {_native.MATCH_MAX_NQ} queries per group, got {gw}")
    most = max((int(t["labels"].shape[0]) for t in targets), default=0)
    if most > gw:
        raise NativeError(f"lwdetr_amd: an image has {most} targets but a group has {gw} queries; the native matcher "
                          f"solves T <= num_queries / group_detr only (unsupported configuration)")


class GroupHungarianMatcher(nn.Module):
    """The reference's ``HungarianMatcher`` (``matcher.py:27-111``) for any ``group_detr``: group g matches the image's targets
    against the queries ``[g nq/G, (g+1) nq/G)``; per image the pairs of the groups follow each other, query indices global and
    ascending inside a group (``matcher.py:104-110``). Index tensors live on the outputs' device and nothing has been
    synchronised when ``forward`` returns. Limits: ``num_queries % group_detr == 0`` (``ValueError``), at most 1024 queries
    per group and at most that many targets per image (``NativeError``). As in the reference the classification cost uses
    alpha = 0.25, not ``focal_alpha`` (``matcher.py:83``)."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1, focal_alpha: float = 0.25):
        super().__init__()
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        self.cost_class, self.cost_bbox, self.cost_giou, self.focal_alpha = cost_class, cost_bbox, cost_giou, focal_alpha
        self._ws, self._offsets, self._keep, self._last = {}, OrderedDict(), None, None

    def _workspace(self, dev, layers, b, nq, ncls, groups, sum_t):
        key = (dev, b, nq, ncls, layers, groups)
        ws = self._ws.get(key)
        if ws is None or ws.cap < sum_t:
            cap = max(sum_t, 8 * b, 2 * ws.cap if ws is not None else 0)
            ws = self._ws[key] = _TrainWorkspace(dev, layers, b, nq, groups, cap)
        return ws

    def _match(self, arr, nlayers, lg0, packed, groups):
        """cost + grouped assign for the layers of ``arr``; returns the workspace (idx_q / idx_t laid out (layers, groups, sum_t))."""
        b, nq, ncls = lg0.shape
        dev = lg0.device
        ws = self._workspace(dev, nlayers, b, nq, ncls, groups, packed.sum_t)
        l = _native.lib()
        with torch.cuda.device(dev):
            st = _native.stream_ptr(dev)
            _native.check(l.lwdetr_match_cost(arr, nlayers, b, nq, ncls, packed.labels.data_ptr(), packed.boxes.data_ptr(),
                                              packed.offsets.data_ptr(), packed.counts_c, float(self.cost_class), float(self.cost_bbox),
                                              float(self.cost_giou), 0.25, ws.cost.data_ptr(), _native.dtype_code(lg0.dtype), st),
                          "lwdetr_match_cost")
            _native.check(l.lwdetr_match_assign_groups(ws.cost.data_ptr(), packed.offsets.data_ptr(), packed.counts_c, nlayers, b, nq,
                                                       groups, ws.idx_q.data_ptr(), ws.idx_t.data_ptr(), ws.status.data_ptr(),
                                                       ws.steps.data_ptr(), st), "lwdetr_match_assign_groups")
        self._last = ws
        return ws

    @staticmethod
    def _indices(idx_q, idx_t, layer, nlayers, groups, packed):
        """[(index_i, index_j)] per image from (layers, groups, sum_t) index buffers: the groups of an image one after the other."""
        n, o = packed.sum_t, packed.host_offsets
        q = idx_q[:nlayers * groups * n].view(nlayers, groups, n)[layer]
        t = idx_t[:nlayers * groups * n].view(nlayers, groups, n)[layer]
        return [(q[:, o[i]:o[i + 1]].reshape(-1), t[:, o[i]:o[i + 1]].reshape(-1)) for i in range(len(packed.counts))]

    @torch.no_grad()
    def forward(self, outputs, targets, group_detr=1):
        """A list of ``(index_i, index_j)`` int64 device tensors per image, ``len == group_detr * num_targets``."""
        lg, bx = outputs["pred_logits"], outputs["pred_boxes"]
        if lg.dim() != 3:
            raise ValueError("pred_logits must be (B, num_queries, num_classes)")
        if len(targets) != lg.shape[0]:
            raise ValueError("len(targets) must equal the batch size")
        _check_groups(targets, lg.shape[1], group_detr)
        arr, keep = _layer_array([(lg, bx)], False)
        packed = _Packed(targets, lg.device, lg.shape[1], self._offsets)
        ws = self._match(arr, 1, keep[0], packed, group_detr)
        self._keep = (keep, packed, arr)                   # alive until the next call (the launches are asynchronous)
        return [(i.clone(), j.clone()) for i, j in self._indices(ws.idx_q, ws.idx_t, 0, 1, group_detr, packed)]

    def status(self):
        """(layers, B, groups) int32 CPU tensor of the last call's solver status words: 0 = ok, 1 = the problem saw a non-finite
        cost (its pairs are still a perfect matching of the image's targets). Synchronises."""
        if self._last is None:
            raise RuntimeError("status() before the first call")
        return self._last.status.cpu()

    def steps(self):
        """(layers, B, groups) int32 CPU tensor: shortest-path steps each problem of the last call took. Synchronises."""
        if self._last is None:
            raise RuntimeError("steps() before the first call")
        return self._last.steps.cpu()


def build_group_matcher(args):
    return GroupHungarianMatcher(cost_class=args.set_cost_class, cost_bbox=args.set_cost_bbox, cost_giou=args.set_cost_giou,
                                 focal_alpha=args.focal_alpha)


class _Call:
    """What one criterion call hands to the autograd Function beside the tensors."""

    def __init__(self, matcher, packed, groups, form, alpha, num_boxes, nlayers):
        self.matcher, self.packed, self.groups, self.form, self.alpha = matcher, packed, groups, form, alpha
        self.num_boxes, self.nlayers = num_boxes, nlayers
        self.idx_q = self.idx_t = None


class _CriterionFunction(torch.autograd.Function):
    """(logits_0, boxes_0, logits_1, boxes_1, ...) -> (layers, 5) f32: loss_ce, class_error, loss_bbox, loss_giou,
    cardinality_error per layer. ``backward`` reads the upstream (layers, 5) gradient on the device in one launch."""

    @staticmethod
    def forward(ctx, call, *tensors):
        layers = [(tensors[2 * n], tensors[2 * n + 1]) for n in range(call.nlayers)]
        arr, keep = _layer_array(layers, True)
        lg0 = keep[0]
        b, nq, ncls = lg0.shape
        dev = lg0.device
        m, packed = call.matcher, call.packed
        ws = m._match(arr, call.nlayers, lg0, packed, call.groups)
        out = torch.empty(call.nlayers, 5, dtype=torch.float32, device=dev)
        l = _native.lib()
        with torch.cuda.device(dev):
            st = _native.stream_ptr(dev)
            _native.check(l.lwdetr_criterion_train_partials(arr, call.nlayers, b, nq, ncls, packed.labels.data_ptr(), packed.boxes.data_ptr(),
                                                            packed.offsets.data_ptr(), packed.counts_c, ws.idx_q.data_ptr(),
                                                            ws.idx_t.data_ptr(), call.groups, call.form, call.alpha, ws.partials.data_ptr(),
                                                            _native.dtype_code(lg0.dtype), st), "lwdetr_criterion_train_partials")
            _native.check(l.lwdetr_criterion_train_finish(ws.partials.data_ptr(), arr, packed.offsets.data_ptr(), packed.counts_c,
                                                          call.nlayers, b, nq, call.groups, call.form, call.num_boxes, out.data_ptr(), st),
                          "lwdetr_criterion_train_finish")
        n = call.nlayers * call.groups * packed.sum_t
        if any(ctx.needs_input_grad[1:]):                  # the workspace is rewritten by the next call: backward keeps this call's pairs
            call.idx_q, call.idx_t = ws.idx_q[:max(n, 1)].clone(), ws.idx_t[:max(n, 1)].clone()
        else:
            call.idx_q, call.idx_t = ws.idx_q, ws.idx_t
        ctx.call, ctx.keep, ctx.arr = call, keep, arr
        ctx.in_dtypes = [t.dtype for t in tensors]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        call, keep = ctx.call, ctx.keep
        lg0 = keep[0]
        b, nq, ncls = lg0.shape
        dev = lg0.device
        packed = call.packed
        grad_out = grad_out.to(device=dev, dtype=torch.float32).contiguous()
        grads = [torch.empty_like(t) for t in keep]
        garr = (_native.CritLayer * call.nlayers)()
        for n in range(call.nlayers):
            garr[n].logits, garr[n].boxes = grads[2 * n].data_ptr(), grads[2 * n + 1].data_ptr()
        l = _native.lib()
        with torch.cuda.device(dev):
            _native.check(l.lwdetr_criterion_backward(ctx.arr, garr, call.nlayers, b, nq, ncls, packed.labels.data_ptr(),
                                                      packed.boxes.data_ptr(), packed.offsets.data_ptr(), packed.counts_c,
                                                      call.idx_q.data_ptr(), call.idx_t.data_ptr(), call.groups, call.form, call.alpha,
                                                      call.num_boxes, grad_out.data_ptr(), _native.dtype_code(lg0.dtype),
                                                      _native.stream_ptr(dev)), "lwdetr_criterion_backward")
        ctx.keep_grad = (grad_out, garr)                   # alive across the asynchronous launch
        return (None, *[g if g.dtype == dt else g.to(dt) for g, dt in zip(grads, ctx.in_dtypes)])


class TrainSetCriterion(nn.Module):
    """The reference's ``SetCriterion`` (``lwdetr.py:218-506``) with its signature, for ``train()`` and ``eval()``:
    ``forward(outputs, targets)`` returns the reference's loss dict (same keys, same insertion order) as 0-dim f32 device
    tensors. When a ``pred_logits`` / ``pred_boxes`` requires grad, ``loss_ce*``, ``loss_bbox*`` and ``loss_giou*`` carry a
    ``grad_fn``; ``class_error`` and ``cardinality_error*`` never do.

    Flag precedence as in the reference (``lwdetr.py:266-339``): ``ia_bce_loss``, then ``use_position_supervised_loss``, then
    ``use_varifocal_loss``, else the sigmoid focal loss. Matching uses ``group_detr`` groups in training mode and one group in
    eval mode (``lwdetr.py:410``). ``num_boxes`` (``lwdetr.py:417-423``) comes from the target shapes on the host; with
    ``torch.distributed`` initialised it is all-reduced, which is the only host read of a call."""

    def __init__(self, num_classes, matcher, weight_dict, focal_alpha, losses, group_detr=1, sum_group_losses=False,
                 use_varifocal_loss=False, use_position_supervised_loss=False, ia_bce_loss=False):
        super().__init__()
        if not isinstance(matcher, GroupHungarianMatcher):
            raise TypeError("the native training criterion needs lwdetr_amd.models.GroupHungarianMatcher (the matching is fused into its call)")
        unknown = set(losses) - {"labels", "boxes", "cardinality"}
        if unknown:
            raise NotImplementedError(f"unknown losses {sorted(unknown)}")
        self.num_classes, self.matcher, self.weight_dict, self.focal_alpha = num_classes, matcher, weight_dict, focal_alpha
        self.losses, self.group_detr, self.sum_group_losses = list(losses), group_detr, sum_group_losses
        self.use_varifocal_loss, self.use_position_supervised_loss = bool(use_varifocal_loss), bool(use_position_supervised_loss)
        self.ia_bce_loss = bool(ia_bce_loss)
        self.last_indices = None

    @property
    def loss_form(self):
        if self.ia_bce_loss:
            return _native.LOSS_IA_BCE
        if self.use_position_supervised_loss:
            return _native.LOSS_POSITION_SUPERVISED
        if self.use_varifocal_loss:
            return _native.LOSS_VARIFOCAL
        return _native.LOSS_FOCAL

    def _num_boxes(self, packed, dev, groups):
        num_boxes = float(packed.sum_t)
        if not self.sum_group_losses:
            num_boxes = num_boxes * groups
        world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            t = torch.as_tensor([num_boxes], dtype=torch.float, device=dev)
            torch.distributed.all_reduce(t)
            world = torch.distributed.get_world_size()
            num_boxes = t.item()
        return max(num_boxes / world, 1.0)

    def forward(self, outputs, targets):
        names, layers = [""], [(outputs["pred_logits"], outputs["pred_boxes"])]
        for i, aux in enumerate(outputs.get("aux_outputs", [])):
            names.append(f"_{i}")
            layers.append((aux["pred_logits"], aux["pred_boxes"]))
        if "enc_outputs" in outputs:
            names.append("_enc")
            layers.append((outputs["enc_outputs"]["pred_logits"], outputs["enc_outputs"]["pred_boxes"]))
        if len(layers) > _native.CRIT_MAX_LAYERS:
            raise NativeError(f"lwdetr_amd: at most {_native.CRIT_MAX_LAYERS} output layers per criterion call, got {len(layers)}")
        lg0 = layers[0][0]
        if lg0.dim() != 3:
            raise ValueError("pred_logits must be (B, num_queries, num_classes)")
        b, nq, _ = lg0.shape
        if len(targets) != b:
            raise ValueError("len(targets) must equal the batch size")
        groups = self.group_detr if self.training else 1   # lwdetr.py:410
        _check_groups(targets, nq, groups)
        for lg, bx in layers:
            _native.require_cuda(lg, bx)
            if lg.shape != lg0.shape or lg.dtype != lg0.dtype or lg.device != lg0.device or tuple(bx.shape) != (*lg0.shape[:2], 4):
                raise ValueError("every layer's pred_logits / pred_boxes must share one shape, dtype and device")
        dev = lg0.device
        m = self.matcher
        packed = _Packed(targets, dev, nq, m._offsets)
        call = _Call(m, packed, groups, self.loss_form, float(self.focal_alpha), float(self._num_boxes(packed, dev, groups)), len(layers))
        out = _CriterionFunction.apply(call, *[t for pair in layers for t in pair])
        self.last_indices = [m._indices(call.idx_q, call.idx_t, n, len(layers), groups, packed) for n in range(len(layers))]
        detached = out.detach()
        want = {"labels": ("loss_ce", "class_error"), "boxes": ("loss_bbox", "loss_giou"), "cardinality": ("cardinality_error",)}
        losses = {}
        for n, suffix in enumerate(names):
            for loss in self.losses:
                for k in want[loss]:
                    if k == "class_error" and n:           # logged for the last layer only (lwdetr.py:436-438, :448-450)
                        continue
                    col = _LOSS_KEYS.index(k)
                    losses[k + suffix] = (out if col in _GRAD_ROWS else detached)[n, col]
        return losses


def build_train_criterion(args, num_classes=None):
    """The criterion of the reference's ``build`` (``lwdetr.py:592-616``) for training: weight dict with the aux / enc keys,
    ``losses = ["labels", "boxes", "cardinality"]``, every loss flag of ``args`` honoured."""
    if num_classes is None:
        num_classes = 366 if args.dataset_file == "o365" else (91 if args.dataset_file == "coco" else 20)
    weight_dict = {"loss_ce": args.cls_loss_coef, "loss_bbox": args.bbox_loss_coef}
    weight_dict["loss_giou"] = args.giou_loss_coef
    if args.aux_loss:
        aux = {}
        for i in range(args.dec_layers - 1):
            aux.update({k + f"_{i}": v for k, v in weight_dict.items()})
        if args.two_stage:
            aux.update({k + "_enc": v for k, v in weight_dict.items()})
        weight_dict.update(aux)
    return TrainSetCriterion(num_classes, matcher=build_group_matcher(args), weight_dict=weight_dict, focal_alpha=args.focal_alpha,
                             losses=["labels", "boxes", "cardinality"], group_detr=args.group_detr,
                             sum_group_losses=getattr(args, "sum_group_losses", False),
                             use_varifocal_loss=getattr(args, "use_varifocal_loss", False),
                             use_position_supervised_loss=getattr(args, "use_position_supervised_loss", False),
                             ia_bce_loss=getattr(args, "ia_bce_loss", False))
