"""Plain torch fp64 restatement of the reference's evaluation criterion: matcher cost, assignment, losses, key order - and the
deterministic inputs of the criterion fixtures. TEST INFRASTRUCTURE ONLY: nothing under lw-detr_amd/ imports it.

Every function cites the reference lines it follows (paths relative to the reference repository). Inputs of any float dtype
are converted to fp64 first, so `cost_matrix(logits.half(), ...)` is the exact cost of the ROUNDED inputs.
"""
import itertools

import numpy as np
import torch

from lwdetr_amd.synth import _key, uniform01

# (nq, T, C): the single-image fixture problems (tools/gen_golden_criterion.py, tests/golden/criterion_*.npz)
PROBLEMS = [(8, 5, 7), (37, 9, 91), (300, 1, 91), (300, 40, 91), (300, 100, 91), (300, 64, 366), (65, 65, 20)]
BATCH = dict(nq=300, C=91, counts=(0, 7, 40), layers=4)            # final, aux 0, aux 1, enc
BATCH_EMPTY = dict(nq=300, C=91, counts=(0, 0, 0), layers=4)
COST_W = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)       # set_cost_* of configs.py
FOCAL_ALPHA = 0.25
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def problem_name(nq, t, c):
    return f"p_{nq}_{t}_{c}"


# ------------------------------------------------------------------------------------------------------------ inputs
def _normal(name, n, seed):
    u = uniform01(_key(name, seed), 2 * n)
    return np.sqrt(-2.0 * np.log(1.0 - u[:n])) * np.cos(2.0 * np.pi * u[n:])          # Box-Muller on the counter-based hash


def _uniform(name, n, lo, hi, seed):
    return lo + (hi - lo) * uniform01(_key(name, seed), n)


def synth_outputs(layers, b, nq, c, seed):
    """[(logits (B,nq,C) f32, boxes (B,nq,4) f32)] per layer: logits 2 N(0,1) - 3, centres in [0, 1], sizes in [0.02, 0.52]."""
    out = []
    for l in range(layers):
        lg = (2.0 * _normal(f"crit.logits.{l}", b * nq * c, seed) - 3.0).astype(np.float32).reshape(b, nq, c)
        cxy = _uniform(f"crit.cxy.{l}", b * nq * 2, 0.0, 1.0, seed).reshape(b, nq, 2)
        wh = _uniform(f"crit.wh.{l}", b * nq * 2, 0.02, 0.52, seed).reshape(b, nq, 2)
        out.append((torch.from_numpy(lg), torch.from_numpy(np.concatenate([cxy, wh], -1).astype(np.float32))))
    return out


def synth_targets(counts, c, seed):
    tg = []
    for i, t in enumerate(counts):
        lab = np.minimum((_uniform(f"crit.tlab.{i}", t, 0.0, 1.0, seed) * c).astype(np.int64), c - 1)
        cxy = _uniform(f"crit.tcxy.{i}", t * 2, 0.0, 1.0, seed).reshape(t, 2)
        wh = _uniform(f"crit.twh.{i}", t * 2, 0.02, 0.52, seed).reshape(t, 2)
        tg.append({"labels": torch.from_numpy(lab), "boxes": torch.from_numpy(np.concatenate([cxy, wh], -1).astype(np.float32))})
    return tg


def as_outputs(layers):
    """The model's output dict from [(logits, boxes)]: layer 0 final, the last one enc (when there are 4), aux between."""
    out = {"pred_logits": layers[0][0], "pred_boxes": layers[0][1]}
    if len(layers) > 1:
        out["aux_outputs"] = [{"pred_logits": a, "pred_boxes": b} for a, b in layers[1:-1]]
        out["enc_outputs"] = {"pred_logits": layers[-1][0], "pred_boxes": layers[-1][1]}
    return out


def output_layers(outputs):
    """[(suffix, logits, boxes)] in the order the reference walks them (models/lwdetr.py:425-453)."""
    ls = [("", outputs["pred_logits"], outputs["pred_boxes"])]
    ls += [(f"_{i}", a["pred_logits"], a["pred_boxes"]) for i, a in enumerate(outputs.get("aux_outputs", []))]
    if "enc_outputs" in outputs:
        ls.append(("_enc", outputs["enc_outputs"]["pred_logits"], outputs["enc_outputs"]["pred_boxes"]))
    return ls


# ------------------------------------------------------------------------------------------------------------ boxes
def box_cxcywh_to_xyxy(x):                                       # util/box_ops.py:21-25
    xc, yc, w, h = x.unbind(-1)
    w, h = w.clamp(min=0.0), h.clamp(min=0.0)
    return torch.stack([xc - 0.5 * w, yc - 0.5 * h, xc + 0.5 * w, yc + 0.5 * h], -1)


def box_iou(a, b):                                               # util/box_ops.py:36-49
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt, rb = torch.max(a[:, None, :2], b[:, :2]), torch.min(a[:, None, 2:], b[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area1[:, None] + area2 - inter
    return inter / union, union


def generalized_box_iou(a, b):                                   # util/box_ops.py:52-73
    iou, union = box_iou(a, b)
    lt, rb = torch.min(a[:, None, :2], b[:, :2]), torch.max(a[:, None, 2:], b[:, 2:])
    wh = (rb - lt).clamp(min=0)
    area = wh[..., 0] * wh[..., 1]
    return iou - (area - union) / area


# ------------------------------------------------------------------------------------------------------------ matcher
def cost_matrix(logits, boxes, labels, tboxes, cost_class=2.0, cost_bbox=5.0, cost_giou=2.0):
    """(nq, T) fp64 cost of ONE image: models/matcher.py:71-94 (alpha = 0.25, gamma = 2 are the matcher's own constants)."""
    prob = logits.double().sigmoid()
    ob, tb = boxes.double(), tboxes.double()
    giou = generalized_box_iou(box_cxcywh_to_xyxy(ob), box_cxcywh_to_xyxy(tb))
    alpha, gamma = 0.25, 2.0
    neg = (1 - alpha) * (prob ** gamma) * (-(1 - prob + 1e-8).log())
    pos = alpha * ((1 - prob) ** gamma) * (-(prob + 1e-8).log())
    c_class = pos[:, labels] - neg[:, labels]
    c_bbox = torch.cdist(ob, tb, p=1)
    return cost_bbox * c_bbox + cost_class * c_class + cost_giou * (-giou)


def solve(cost):
    """(query indices ascending, target indices) of the optimal assignment of a (nq, T) cost: matcher.py:103."""
    from scipy.optimize import linear_sum_assignment
    i, j = linear_sum_assignment(np.asarray(cost, dtype=np.float64))
    return i.astype(np.int64), j.astype(np.int64)


def solve_brute(cost):
    """The same by enumeration (small problems): every injective map target -> query."""
    cost = np.asarray(cost, dtype=np.float64)
    nq, t = cost.shape
    best, arg = np.inf, None
    for qs in itertools.permutations(range(nq), t):
        s = cost[list(qs), range(t)].sum()
        if s < best:
            best, arg = s, qs
    order = np.argsort(arg)
    return np.asarray(arg, dtype=np.int64)[order], order.astype(np.int64)


def match(logits, boxes, targets, **w):
    """[(index_i, index_j)] per image for (B,nq,C) logits / (B,nq,4) boxes: matcher.py:50-111 with one group."""
    return [solve(cost_matrix(logits[b], boxes[b], t["labels"], t["boxes"], **w).numpy()) if len(t["labels"])
            else (np.zeros(0, np.int64), np.zeros(0, np.int64)) for b, t in enumerate(targets)]


# ------------------------------------------------------------------------------------------------------------ losses
def layer_losses(logits, boxes, targets, indices, num_boxes, ia_bce=False, focal_alpha=FOCAL_ALPHA, log=True):
    """The loss dict of one layer in fp64 (python floats): models/lwdetr.py:256-380."""
    x, bx = logits.double(), boxes.double()
    bsz, nq, ncls = x.shape
    bi = torch.cat([torch.full((len(i),), b, dtype=torch.int64) for b, (i, _) in enumerate(indices)])     # lwdetr.py:382-386
    qi = torch.cat([torch.as_tensor(i, dtype=torch.int64) for i, _ in indices])
    tcls = torch.cat([t["labels"][torch.as_tensor(j, dtype=torch.int64)] for t, (_, j) in zip(targets, indices)])
    tbox = torch.cat([t["boxes"][torch.as_tensor(j, dtype=torch.int64)] for t, (_, j) in zip(targets, indices)]).double()
    src = bx[bi, qi]
    prob = x.sigmoid()
    if ia_bce:                                                   # lwdetr.py:266-290
        alpha, gamma = focal_alpha, 2
        ious = torch.diag(box_iou(box_cxcywh_to_xyxy(src), box_cxcywh_to_xyxy(tbox))[0]) if len(qi) else torch.zeros(0, dtype=torch.float64)
        pos_w, neg_w = torch.zeros_like(x), prob ** gamma
        t = (prob[bi, qi, tcls].pow(alpha) * ious.pow(1 - alpha)).clamp(min=0.01)
        pos_w[bi, qi, tcls] = t
        neg_w[bi, qi, tcls] = 1 - t
        loss_ce = (-pos_w * prob.log() - neg_w * (1 - prob).log()).sum() / num_boxes
    else:                                                        # lwdetr.py:330-339, sigmoid_focal_loss :458-483
        onehot = torch.zeros_like(x)
        onehot[bi, qi, tcls] = 1.0
        ce = torch.nn.functional.binary_cross_entropy_with_logits(x, onehot, reduction="none")
        p_t = prob * onehot + (1 - prob) * (1 - onehot)
        loss = ce * ((1 - p_t) ** 2)
        loss = (focal_alpha * onehot + (1 - focal_alpha) * (1 - onehot)) * loss
        loss_ce = loss.mean(1).sum() / num_boxes * nq
    out = {"loss_ce": float(loss_ce)}
    if log:                                                      # lwdetr.py:344, util/misc.py accuracy (top-1; 0 when there is no target)
        acc = float((x[bi, qi].argmax(-1) == tcls).double().sum() * (100.0 / len(qi))) if len(qi) else 0.0
        out["class_error"] = 100.0 - acc
    out["loss_bbox"] = float((src - tbox).abs().sum() / num_boxes)                                       # lwdetr.py:371-374
    giou = torch.diag(generalized_box_iou(box_cxcywh_to_xyxy(src), box_cxcywh_to_xyxy(tbox))) if len(qi) else torch.zeros(0, dtype=torch.float64)
    out["loss_giou"] = float((1 - giou).sum() / num_boxes)                                               # lwdetr.py:376-379
    card = (x.argmax(-1) != ncls - 1).sum(1).double()                                                    # lwdetr.py:354-357
    out["cardinality_error"] = float((card - torch.tensor([float(len(t["labels"])) for t in targets], dtype=torch.float64)).abs().mean())
    return out


def criterion(outputs, targets, ia_bce=False, focal_alpha=FOCAL_ALPHA, weights=COST_W):
    """(loss dict in the reference's key order, [[(i, j)] per layer]): models/lwdetr.py:403-455 in eval mode, world size 1."""
    num_boxes = max(float(sum(len(t["labels"]) for t in targets)), 1.0)                                   # lwdetr.py:417-423
    losses, all_idx = {}, []
    for n, (suffix, lg, bx) in enumerate(output_layers(outputs)):
        idx = match(lg, bx, targets, **weights)
        all_idx.append(idx)
        d = layer_losses(lg, bx, targets, idx, num_boxes, ia_bce, focal_alpha, log=n == 0)
        # the reference walks self.losses = labels, boxes, cardinality: layer_losses fills its dict in that order
        losses.update({k + suffix: v for k, v in d.items()})
    return losses, all_idx


def loss_keys(aux_layers, enc=True):
    keys = ["loss_ce", "class_error", "loss_bbox", "loss_giou", "cardinality_error"]
    for s in [f"_{i}" for i in range(aux_layers)] + (["_enc"] if enc else []):
        keys += [k + s for k in ("loss_ce", "loss_bbox", "loss_giou", "cardinality_error")]
    return keys


def to_dtype(layers, name):
    """The f32 layers rounded to a storage dtype ("f32" / "f16" / "bf16"), boxes included, as the model's outputs would be."""
    return [(a.to(DTYPES[name]), b.to(DTYPES[name])) for a, b in layers]
