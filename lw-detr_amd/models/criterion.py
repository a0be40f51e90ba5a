"""Inference-time criterion behind the reference's interface (``models/matcher.py``, ``models/lwdetr.py:218-455``):
``HungarianMatcher`` and ``SetCriterion`` with no gradient and no host synchronisation.

From the packed targets on, a call is four launches of ``csrc/match.hip`` for all layers (final, aux 0..n, enc) together:
cost matrices -> assignment (one wave per (layer, image) problem) -> per-chunk loss partials -> finish. Nothing is copied
to the host on the call path; ``HungarianMatcher.status()`` reads the solver's status words on request.
"""
import ctypes as C
from collections import OrderedDict

import torch
from torch import nn

from .. import _native
from .._native import NativeError

_LOSS_KEYS = ("loss_ce", "class_error", "loss_bbox", "loss_giou", "cardinality_error")
_OFFSET_CACHE_MAX = 64


class _Workspace:
    """Device buffers of one criterion shape; ``cap`` packed targets fit. Kept by the owner across the asynchronous launch."""

    def __init__(self, dev, layers, b, nq, cap):
        self.cap = cap
        self.cost = torch.empty(layers * cap * nq, dtype=torch.float32, device=dev)
        self.idx_q = torch.zeros(layers * cap, dtype=torch.int64, device=dev)
        self.idx_t = torch.zeros(layers * cap, dtype=torch.int64, device=dev)
        self.status = torch.zeros(layers, b, dtype=torch.int32, device=dev)
        self.steps = torch.zeros(layers, b, dtype=torch.int32, device=dev)
        self.partials = torch.empty(max(1, _native.lib().lwdetr_criterion_partials_floats(layers, b, nq)), dtype=torch.float32, device=dev)


class _Packed:
    """Targets of one call, packed: labels (sumT) int64, boxes (sumT, 4) f32, offsets (B + 1) int32 on the device, counts on the host."""

    def __init__(self, targets, dev, nq, offset_cache):
        counts = [int(t["labels"].shape[0]) for t in targets]
        for t, n in zip(targets, counts):
            _native.require_cuda(t["labels"], t["boxes"])
            if tuple(t["boxes"].shape) != (n, 4):
                raise ValueError(f"target boxes must be (T, 4) beside {n} labels, got {tuple(t['boxes'].shape)}")
        self.counts = counts
        self.sum_t = sum(counts)
        self.counts_c = (C.c_int32 * len(counts))(*counts)
        key = (dev, tuple(counts))
        offs = offset_cache.get(key)
        if offs is None:                                   # one upload per new tuple of counts; a repeated batch shape (a captured graph) hits the cache
            acc = [0]
            for n in counts:
                acc.append(acc[-1] + n)
            offs = torch.tensor(acc, dtype=torch.int32).to(dev)
            offset_cache[key] = offs
            while len(offset_cache) > _OFFSET_CACHE_MAX:
                offset_cache.popitem(last=False)
        self.offsets = offs
        self.host_offsets = [0]
        for n in counts:
            self.host_offsets.append(self.host_offsets[-1] + n)
        if self.sum_t:
            self.labels = torch.cat([t["labels"] for t in targets]).to(device=dev, dtype=torch.int64).contiguous()
            self.boxes = torch.cat([t["boxes"] for t in targets]).to(device=dev, dtype=torch.float32).contiguous()
        else:
            self.labels = torch.zeros(1, dtype=torch.int64, device=dev)
            self.boxes = torch.zeros(1, 4, dtype=torch.float32, device=dev)


def _check_counts(targets, nq):
    """Refuse T_b > num_queries before anything is launched (lwdetr_match_assign would return LWDETR_ERR_UNSUPPORTED)."""
    most = max((int(t["labels"].shape[0]) for t in targets), default=0)
    if most > nq:
        raise NativeError(f"lwdetr_amd: an image has {most} targets but the model has {nq} queries; the native matcher "
                          f"solves T <= num_queries only (unsupported configuration)")


def _layer_array(layers, class_error_first):
    """(ctypes array of lwdetr_crit_layer, the tensors it points to) for [(logits, boxes), ...] of one shape and dtype."""
    lg0 = layers[0][0]
    if lg0.dim() != 3:
        raise ValueError("pred_logits must be (B, num_queries, num_classes)")
    keep, arr = [], (_native.CritLayer * len(layers))()
    for n, (lg, bx) in enumerate(layers):
        _native.require_cuda(lg, bx)
        if lg.shape != lg0.shape or lg.dtype != lg0.dtype or lg.device != lg0.device or tuple(bx.shape) != (*lg0.shape[:2], 4):
            raise ValueError("every layer's pred_logits / pred_boxes must share one shape, dtype and device")
        lg, bx = lg.detach().contiguous(), bx.detach().to(lg0.dtype).contiguous()
        keep += [lg, bx]
        arr[n].logits, arr[n].boxes = lg.data_ptr(), bx.data_ptr()
        arr[n].class_error = 1 if (class_error_first and n == 0) else 0
    return arr, keep


class HungarianMatcher(nn.Module):
    """The reference's ``HungarianMatcher`` (``matcher.py:27-111``) on the GPU: the same cost, the same optimum as
    ``scipy.optimize.linear_sum_assignment``, pairs in the same order (ascending query index).

    The one difference: the returned index tensors live on the outputs' device, and no synchronisation has happened when
    ``forward`` returns (the reference returns CPU tensors after a ``.cpu()`` of the cost matrix). As in the reference, the
    classification cost uses alpha = 0.25, not ``focal_alpha`` (``matcher.py:83``). Limits: ``num_queries <= 1024`` and at most
    ``num_queries`` targets per image (``NativeError`` otherwise)."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1, focal_alpha: float = 0.25):
        super().__init__()
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        self.cost_class, self.cost_bbox, self.cost_giou, self.focal_alpha = cost_class, cost_bbox, cost_giou, focal_alpha
        self._ws, self._offsets, self._keep, self._last = {}, OrderedDict(), None, None

    def _workspace(self, dev, layers, b, nq, ncls, sum_t):
        key = (dev, b, nq, ncls, layers)
        ws = self._ws.get(key)
        if ws is None or ws.cap < sum_t:
            cap = max(sum_t, 8 * b, 2 * ws.cap if ws is not None else 0)
            ws = self._ws[key] = _Workspace(dev, layers, b, nq, cap)
        return ws

    def _match(self, arr, nlayers, lg0, packed):
        """cost + assign for the layers of ``arr``; returns the workspace (idx_q / idx_t laid out (layers, sum_t))."""
        b, nq, ncls = lg0.shape
        dev = lg0.device
        if nq > _native.MATCH_MAX_NQ:
            raise NativeError(f"lwdetr_amd: the native matcher supports at most {_native.MATCH_MAX_NQ} queries, got {nq}")
        ws = self._workspace(dev, nlayers, b, nq, ncls, packed.sum_t)
        l = _native.lib()
        with torch.cuda.device(dev):
            st = _native.stream_ptr(dev)
            _native.check(l.lwdetr_match_cost(arr, nlayers, b, nq, ncls, packed.labels.data_ptr(), packed.boxes.data_ptr(),
                                              packed.offsets.data_ptr(), packed.counts_c, float(self.cost_class), float(self.cost_bbox),
                                              float(self.cost_giou), 0.25, ws.cost.data_ptr(), _native.dtype_code(lg0.dtype), st),
                          "lwdetr_match_cost")
            _native.check(l.lwdetr_match_assign(ws.cost.data_ptr(), packed.offsets.data_ptr(), packed.counts_c, nlayers, b, nq,
                                                ws.idx_q.data_ptr(), ws.idx_t.data_ptr(), ws.status.data_ptr(), ws.steps.data_ptr(), st),
                          "lwdetr_match_assign")
        self._last = ws
        return ws

    @staticmethod
    def _indices(ws, layer, packed):
        base, o = layer * packed.sum_t, packed.host_offsets
        return [(ws.idx_q[base + o[i]:base + o[i + 1]], ws.idx_t[base + o[i]:base + o[i + 1]]) for i in range(len(packed.counts))]

    @torch.no_grad()
    def forward(self, outputs, targets, group_detr=1):
        """A list of ``(index_i, index_j)`` int64 device tensors per image, ``len == min(num_queries, num_targets)``
        (``matcher.py:50-111``), on the outputs' device; nothing has been synchronised when they are returned."""
        if group_detr != 1:
            raise NotImplementedError("the native matcher matches with one group, as the reference does in eval (lwdetr.py:410)")
        lg, bx = outputs["pred_logits"], outputs["pred_boxes"]
        _check_counts(targets, lg.shape[1])
        arr, keep = _layer_array([(lg, bx)], False)
        packed = _Packed(targets, lg.device, lg.shape[1], self._offsets)
        if len(targets) != lg.shape[0]:
            raise ValueError("len(targets) must equal the batch size")
        ws = self._match(arr, 1, keep[0], packed)
        self._keep = (keep, packed, arr)                   # alive until the next call (the launches are asynchronous)
        return [(i.clone(), j.clone()) for i, j in self._indices(ws, 0, packed)]

    def status(self):
        """(layers, B) int32 CPU tensor of the last call's solver status words: 0 = ok, 1 = the problem saw a non-finite cost
        (its pairs are still a perfect matching of the image's targets, but not an optimum of anything). Synchronises."""
        if self._last is None:
            raise RuntimeError("status() before the first call")
        return self._last.status.cpu()

    def steps(self):
        """(layers, B) int32 CPU tensor: shortest-path steps each problem of the last call took. Synchronises."""
        if self._last is None:
            raise RuntimeError("steps() before the first call")
        return self._last.steps.cpu()


def build_matcher(args):
    return HungarianMatcher(cost_class=args.set_cost_class, cost_bbox=args.set_cost_bbox, cost_giou=args.set_cost_giou,
                            focal_alpha=args.focal_alpha)


class SetCriterion(nn.Module):
    """The reference's ``SetCriterion`` (``lwdetr.py:218-455``) for evaluation: ``forward(outputs, targets)`` returns the
    reference's loss dict (same keys, same insertion order) as 0-dim device tensors, without gradient.

    Loss forms: sigmoid focal loss (all flags off) and ``ia_bce_loss=True``. Training mode is refused; matching always uses one
    group (``lwdetr.py:410``). ``num_boxes`` comes from the target shapes on the host; with ``torch.distributed`` initialised
    it is all-reduced as ``lwdetr.py:416-423`` does, which is the only host read of a call."""

    def __init__(self, num_classes, matcher, weight_dict, focal_alpha, losses, group_detr=1, sum_group_losses=False,
                 use_varifocal_loss=False, use_position_supervised_loss=False, ia_bce_loss=False):
        super().__init__()
        if use_varifocal_loss or use_position_supervised_loss:
            raise NotImplementedError("the native criterion implements the sigmoid focal loss and ia_bce_loss only")
        if not isinstance(matcher, HungarianMatcher):
            raise TypeError("the native criterion needs lwdetr_amd.models.HungarianMatcher (the matching is fused into its call)")
        unknown = set(losses) - {"labels", "boxes", "cardinality"}
        if unknown:
            raise NotImplementedError(f"unknown losses {sorted(unknown)}")
        self.num_classes, self.matcher, self.weight_dict, self.focal_alpha = num_classes, matcher, weight_dict, focal_alpha
        self.losses, self.group_detr, self.sum_group_losses = list(losses), group_detr, sum_group_losses
        self.use_varifocal_loss, self.use_position_supervised_loss, self.ia_bce_loss = False, False, bool(ia_bce_loss)
        self._keep = None
        super().train(False)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("the native criterion is inference only (no gradient); use the reference's criterion to train")
        return super().train(False)

    def _num_boxes(self, packed, dev):
        num_boxes = float(packed.sum_t)                    # one group in eval: group_detr = 1 (lwdetr.py:410, :417-419)
        world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            t = torch.as_tensor([num_boxes], dtype=torch.float, device=dev)
            torch.distributed.all_reduce(t)
            world = torch.distributed.get_world_size()
            num_boxes = t.item()
        return max(num_boxes / world, 1.0)

    @torch.no_grad()
    def forward(self, outputs, targets):
        if self.training:
            raise NotImplementedError("the native criterion is inference only")
        names, layers = [""], [(outputs["pred_logits"], outputs["pred_boxes"])]
        for i, aux in enumerate(outputs.get("aux_outputs", [])):
            names.append(f"_{i}")
            layers.append((aux["pred_logits"], aux["pred_boxes"]))
        if "enc_outputs" in outputs:
            names.append("_enc")
            layers.append((outputs["enc_outputs"]["pred_logits"], outputs["enc_outputs"]["pred_boxes"]))
        if len(layers) > _native.CRIT_MAX_LAYERS:
            raise NativeError(f"lwdetr_amd: at most {_native.CRIT_MAX_LAYERS} output layers per criterion call, got {len(layers)}")
        _check_counts(targets, layers[0][0].shape[1])
        arr, keep = _layer_array(layers, True)
        lg0 = keep[0]
        b, nq, ncls = lg0.shape
        dev = lg0.device
        if len(targets) != b:
            raise ValueError("len(targets) must equal the batch size")
        m = self.matcher
        packed = _Packed(targets, dev, nq, m._offsets)
        num_boxes = self._num_boxes(packed, dev)
        ws = m._match(arr, len(layers), lg0, packed)
        out = torch.empty(len(layers), 5, dtype=torch.float32, device=dev)
        form = _native.LOSS_IA_BCE if self.ia_bce_loss else _native.LOSS_FOCAL
        l = _native.lib()
        with torch.cuda.device(dev):
            st = _native.stream_ptr(dev)
            _native.check(l.lwdetr_criterion_partials(arr, len(layers), b, nq, ncls, packed.labels.data_ptr(), packed.boxes.data_ptr(),
                                                      packed.offsets.data_ptr(), packed.counts_c, ws.idx_q.data_ptr(), ws.idx_t.data_ptr(),
                                                      form, float(self.focal_alpha), ws.partials.data_ptr(),
                                                      _native.dtype_code(lg0.dtype), st), "lwdetr_criterion_partials")
            _native.check(l.lwdetr_criterion_finish(ws.partials.data_ptr(), arr, packed.offsets.data_ptr(), packed.counts_c, len(layers),
                                                    b, nq, form, float(num_boxes), out.data_ptr(), st), "lwdetr_criterion_finish")
        self._keep = (keep, packed, arr)                   # alive until the next call (the launches are asynchronous)
        self.last_indices = [m._indices(ws, n, packed) for n in range(len(layers))]
        want = {"labels": ("loss_ce", "class_error"), "boxes": ("loss_bbox", "loss_giou"), "cardinality": ("cardinality_error",)}
        losses = {}
        for n, suffix in enumerate(names):
            for loss in self.losses:
                for k in want[loss]:
                    if k == "class_error" and n:           # logged for the last layer only (lwdetr.py:436-438, :448-450)
                        continue
                    losses[k + suffix] = out[n, _LOSS_KEYS.index(k)]
        return losses


def native_criterion_supported(args) -> bool:
    return not (getattr(args, "use_varifocal_loss", False) or getattr(args, "use_position_supervised_loss", False))


def build_criterion(args, num_classes=None):
    """The criterion of the reference's ``build`` (``lwdetr.py:592-616``): weight dict with the aux / enc keys,
    ``losses = ["labels", "boxes", "cardinality"]``."""
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
    return SetCriterion(num_classes, matcher=build_matcher(args), weight_dict=weight_dict, focal_alpha=args.focal_alpha,
                        losses=["labels", "boxes", "cardinality"], group_detr=args.group_detr,
                        sum_group_losses=getattr(args, "sum_group_losses", False),
                        use_varifocal_loss=getattr(args, "use_varifocal_loss", False),
                        use_position_supervised_loss=getattr(args, "use_position_supervised_loss", False),
                        ia_bce_loss=getattr(args, "ia_bce_loss", False))
