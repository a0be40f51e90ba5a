"""Plain torch fp64 restatement of the reference's TRAINING criterion (models/lwdetr.py:218-506 in train() mode, models/matcher.py:50-111):
grouped matching with scipy, the four classification loss forms, gradients by torch autograd - and the deterministic inputs of
tests/golden/criterion_train.npz. TEST INFRASTRUCTURE ONLY: nothing under lw-detr_amd/ imports it. Builds on tests/criterion_ref.py.

Inputs of any float dtype are converted to fp64 first, so every function computes the exact result of the ROUNDED inputs.

The synthetic boxes sit on grids that keep every matched pair away from the kinks of the box losses by construction: prediction
coordinates are (4 k + 1) / 256, target coordinates k / 64. A coordinate difference (the |x| of the L1 loss) is then an odd multiple
of 1 / 256, and the difference of any prediction edge and any target edge (the max / min / clamp of IoU and GIoU) an odd multiple of
1 / 512 - both above 1e-3, both exact in f32, f16 and bf16.
"""
import numpy as np
import torch

import criterion_ref as R

FORMS = ("focal", "iabce", "varifocal", "possup")
FORM_FLAGS = {"focal": {}, "iabce": dict(ia_bce_loss=True), "varifocal": dict(use_varifocal_loss=True),
              "possup": dict(use_position_supervised_loss=True)}
# name -> shape of a fixture batch. g3: group edges (37, 74) cross the 32-query chunks and the 64-lane columns, T_b = group width;
# g13: the reference's 13 x 300 queries; c366: Objects365's class count; empty: no target anywhere; h7 / h91: the host problems
BATCHES = {
    "g3": dict(nq=111, G=3, C=7, counts=(7, 0, 1, 37), layers=4),
    "g13": dict(nq=3900, G=13, C=91, counts=(1, 0, 40), layers=4),
    "c366": dict(nq=74, G=2, C=366, counts=(5, 0, 9), layers=2),
    "empty": dict(nq=111, G=3, C=7, counts=(0, 0, 0), layers=4),
    "h7": dict(nq=37, G=1, C=7, counts=(9,), layers=1),
    "h91": dict(nq=37, G=1, C=91, counts=(9,), layers=1),
}
GRAD_SAMPLES = 256                                               # points per gradient tensor kept in the fixture
KINK = 1e-3


# ------------------------------------------------------------------------------------------------------------ inputs
def _grid(name, n, lo, hi, seed):
    """n integers in [lo, hi] from the counter-based hash."""
    return np.minimum((R._uniform(name, n, 0.0, 1.0, seed) * (hi - lo + 1)).astype(np.int64) + lo, hi)


def synth_outputs(layers, b, nq, c, seed):
    """[(logits (B,nq,C) f32, boxes (B,nq,4) f32)] per layer: logits 2 N(0,1) - 3; centres (4k+1)/256 in (0, 1), sizes (4k+1)/256 in [0.02, 0.52]."""
    out = []
    for l in range(layers):
        lg = (2.0 * R._normal(f"crit.logits.{l}", b * nq * c, seed) - 3.0).astype(np.float32).reshape(b, nq, c)
        cxy = (4 * _grid(f"critT.cxy.{l}", b * nq * 2, 0, 63, seed) + 1).reshape(b, nq, 2) / 256.0
        wh = (4 * _grid(f"critT.wh.{l}", b * nq * 2, 1, 33, seed) + 1).reshape(b, nq, 2) / 256.0
        out.append((torch.from_numpy(lg), torch.from_numpy(np.concatenate([cxy, wh], -1).astype(np.float32))))
    return out


def synth_targets(counts, c, seed):
    tg = []
    for i, t in enumerate(counts):
        lab = np.minimum((R._uniform(f"crit.tlab.{i}", t, 0.0, 1.0, seed) * c).astype(np.int64), c - 1)
        cxy = _grid(f"critT.tcxy.{i}", t * 2, 1, 63, seed).reshape(t, 2) / 64.0
        wh = _grid(f"critT.twh.{i}", t * 2, 2, 33, seed).reshape(t, 2) / 64.0
        tg.append({"labels": torch.from_numpy(lab), "boxes": torch.from_numpy(np.concatenate([cxy, wh], -1).astype(np.float32))})
    return tg


def batch_inputs(name, seed, dn="f32"):
    s = BATCHES[name]
    return R.to_dtype(synth_outputs(s["layers"], len(s["counts"]), s["nq"], s["C"], seed), dn), synth_targets(s["counts"], s["C"], seed)


def loss_weights(keys, seed=7):
    """One distinct weight in [0.5, 1.5) per loss key: a swapped row of the upstream gradient shows."""
    return dict(zip(keys, (0.5 + R._uniform("critT.weights", len(keys), 0.0, 1.0, seed)).tolist()))


# ------------------------------------------------------------------------------------------------------------ matcher
def match_groups(logits, boxes, targets, groups, **w):
    """[[(i, j) per group] per image] for (B,nq,C) logits / (B,nq,4) boxes: matcher.py:97-110, query indices global."""
    nq = logits.shape[1]
    assert nq % groups == 0
    gw = nq // groups
    out = []
    for b, t in enumerate(targets):
        per = []
        for g in range(groups):
            if len(t["labels"]):
                cost = R.cost_matrix(logits[b, g * gw:(g + 1) * gw], boxes[b, g * gw:(g + 1) * gw], t["labels"], t["boxes"], **w).numpy()
                i, j = R.solve(cost)
            else:
                i, j = np.zeros(0, np.int64), np.zeros(0, np.int64)
            per.append((i + g * gw, j))
        out.append(per)
    return out


def flatten_groups(per_image):
    """[(index_i, index_j)] per image, the groups one after the other (matcher.py:107-110)."""
    return [(np.concatenate([i for i, _ in per]), np.concatenate([j for _, j in per])) for per in per_image]


# ------------------------------------------------------------------------------------------------------------ losses
def layer_losses(x, bx, targets, indices, num_boxes, form, focal_alpha=R.FOCAL_ALPHA, log=True):
    """The loss dict of one layer as fp64 torch scalars (differentiable in x and bx): models/lwdetr.py:256-380, :458-506."""
    bsz, nq, ncls = x.shape
    bi = torch.cat([torch.full((len(i),), b, dtype=torch.int64) for b, (i, _) in enumerate(indices)])
    qi = torch.cat([torch.as_tensor(i, dtype=torch.int64) for i, _ in indices])
    tcls = torch.cat([t["labels"][torch.as_tensor(j, dtype=torch.int64)] for t, (_, j) in zip(targets, indices)])
    tbox = torch.cat([t["boxes"][torch.as_tensor(j, dtype=torch.int64)] for t, (_, j) in zip(targets, indices)]).double()
    src = bx[bi, qi]
    prob = x.sigmoid()
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    n = len(qi)
    ious = (torch.diag(R.box_iou(R.box_cxcywh_to_xyxy(src.detach()), R.box_cxcywh_to_xyxy(tbox))[0]) if n else torch.zeros(0, dtype=torch.float64)).detach()
    if form == "iabce":                                          # lwdetr.py:266-290
        alpha, gamma = focal_alpha, 2
        pos_w, neg_w = torch.zeros_like(x), prob ** gamma
        t = (prob[bi, qi, tcls].pow(alpha) * ious.pow(1 - alpha)).clamp(min=0.01).detach()
        pos_w = pos_w.index_put((bi, qi, tcls), t)
        neg_w = neg_w.index_put((bi, qi, tcls), 1 - t)
        loss_ce = (-pos_w * prob.log() - neg_w * (1 - prob).log()).sum() / num_boxes
    elif form == "possup":                                       # lwdetr.py:292-311, :497-506
        tgt = torch.zeros_like(x).detach().index_put((bi, qi, tcls), ious)
        tgt = tgt / (tgt.view(bsz, -1, 1).amax(1, True) + 1e-8)
        loss = bce(x, tgt, reduction="none") * (torch.abs(tgt - prob) ** 2)
        loss = (focal_alpha * (tgt > 0.0).double() + (1 - focal_alpha) * (tgt <= 0.0).double()) * loss
        loss_ce = loss.mean(1).sum() / num_boxes * nq
    elif form == "varifocal":                                    # lwdetr.py:313-328, :486-494
        tgt = torch.zeros_like(x).detach().index_put((bi, qi, tcls), ious)
        fw = tgt * (tgt > 0.0).double() + (1 - focal_alpha) * (prob - tgt).abs().pow(2) * (tgt <= 0.0).double()
        loss_ce = (bce(x, tgt, reduction="none") * fw).mean(1).sum() / num_boxes * nq
    else:                                                        # lwdetr.py:330-339, :458-483
        onehot = torch.zeros_like(x).detach().index_put((bi, qi, tcls), torch.ones(n, dtype=torch.float64))
        p_t = prob * onehot + (1 - prob) * (1 - onehot)
        loss = bce(x, onehot, reduction="none") * ((1 - p_t) ** 2)
        loss = (focal_alpha * onehot + (1 - focal_alpha) * (1 - onehot)) * loss
        loss_ce = loss.mean(1).sum() / num_boxes * nq
    out = {"loss_ce": loss_ce}
    if log:                                                      # lwdetr.py:344, util/misc.py accuracy (top-1; 0 when there is no target)
        acc = float((x.detach()[bi, qi].argmax(-1) == tcls).double().sum() * (100.0 / n)) if n else 0.0
        out["class_error"] = torch.tensor(100.0 - acc, dtype=torch.float64)
    out["loss_bbox"] = (src - tbox).abs().sum() / num_boxes                                               # lwdetr.py:371-374
    giou = torch.diag(R.generalized_box_iou(R.box_cxcywh_to_xyxy(src), R.box_cxcywh_to_xyxy(tbox))) if n else torch.zeros(0, dtype=torch.float64)
    out["loss_giou"] = (1 - giou).sum() / num_boxes                                                       # lwdetr.py:376-379
    card = (x.detach().argmax(-1) != ncls - 1).sum(1).double()                                            # lwdetr.py:354-357
    out["cardinality_error"] = (card - torch.tensor([float(len(t["labels"])) for t in targets], dtype=torch.float64)).abs().mean()
    return out


def criterion(layers, targets, form, groups, sum_group_losses=False, training=True, focal_alpha=R.FOCAL_ALPHA, weights=R.COST_W, indices=None):
    """(loss dict of fp64 torch scalars in the reference's key order, [[(i, j) per image] per layer], the fp64 leaves [(x, bx)]):
    models/lwdetr.py:403-455, world size 1. `indices` (per layer, per image) replaces the matching when given."""
    g = groups if training else 1                                                                         # lwdetr.py:410
    num_boxes = float(sum(len(t["labels"]) for t in targets))
    if not sum_group_losses:
        num_boxes *= g                                                                                    # lwdetr.py:417-419
    num_boxes = max(num_boxes, 1.0)
    leaves = [(a.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)) for a, b in layers]
    suffixes = [""] + [f"_{i}" for i in range(len(layers) - 2)] + (["_enc"] if len(layers) > 1 else [])
    losses, all_idx = {}, []
    for n, ((x, bx), suffix) in enumerate(zip(leaves, suffixes)):
        idx = indices[n] if indices is not None else flatten_groups(match_groups(x.detach(), bx.detach(), targets, g, **weights))
        all_idx.append(idx)
        d = layer_losses(x, bx, targets, idx, num_boxes, form, focal_alpha, log=n == 0)
        losses.update({k + suffix: v for k, v in d.items()})
    return losses, all_idx, leaves


def gradients(layers, targets, form, groups, weights, **kw):
    """({key: float}, [(d/d logits, d/d boxes) fp64 per layer], indices) of sum_k weights[k] * loss_k over the keys that carry a gradient."""
    losses, idx, leaves = criterion(layers, targets, form, groups, **kw)
    total = sum(weights[k] * v for k, v in losses.items() if v.requires_grad)
    flat = [t for pair in leaves for t in pair]
    gr = torch.autograd.grad(total, flat, allow_unused=True) if torch.is_tensor(total) and total.requires_grad else [None] * len(flat)
    gr = [torch.zeros_like(t) if g is None else g for g, t in zip(gr, flat)]
    return {k: float(v.detach()) for k, v in losses.items()}, [(gr[2 * n], gr[2 * n + 1]) for n in range(len(leaves))], idx


# ------------------------------------------------------------------------------------------------------------ kinks
def kink_distance(boxes, targets, indices):
    """The smallest distance of any matched pair of one layer to a kink of the box losses: a coordinate difference (|x| of the L1 loss),
    any prediction edge against any target edge of the same axis (max / min ties, touching boxes, the intersection clamp), a size
    against zero (the width clamp); and the smallest gap between an image's largest matched IoU and its next one (the arg-max of the
    position-supervised normaliser). Returns (box distance, IoU gap); inf where there is no pair."""
    dist, gap = np.inf, np.inf
    for b, (i, j) in enumerate(indices):
        if not len(i):
            continue
        o = boxes[b].double()[torch.as_tensor(i)]
        t = targets[b]["boxes"].double()[torch.as_tensor(j)]
        dist = min(dist, float((o - t).abs().min()), float(o[:, 2:].min()))
        oe, te = R.box_cxcywh_to_xyxy(o), R.box_cxcywh_to_xyxy(t)
        for axis in (0, 1):
            d = (oe[:, [axis, axis + 2]][:, :, None] - te[:, [axis, axis + 2]][:, None, :]).abs()
            dist = min(dist, float(d.min()))
        iou = torch.diag(R.box_iou(oe, te)[0]).sort(descending=True).values
        if len(iou) > 1:
            gap = min(gap, float(iou[0] - iou[1]))
    return dist, gap


def sample_points(n):
    """At most GRAD_SAMPLES indices into a flattened gradient tensor of n elements, odd stride."""
    if n <= GRAD_SAMPLES:
        return np.arange(n)
    stride = -(-n // GRAD_SAMPLES)
    stride += 1 - (stride % 2)
    return np.arange(0, n, stride)[:GRAD_SAMPLES]
