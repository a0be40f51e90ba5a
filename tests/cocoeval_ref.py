"""Oracle of the COCO box evaluator: a plain loop-for-loop restatement of pycocotools' COCOeval for iouType 'bbox' in numpy / Python
floats (IEEE f64, no fused multiply-add) - ``_prepare``, ``computeIoU`` (maskApi.c ``bbIou``), ``evaluateImg``, ``accumulate``,
``summarize``. Written for obviousness, not speed, and independent of the kernels' data layout: it works on COCO's own lists of dicts.

One deliberate difference from pycocotools, shared with the kernels and documented in include/lwdetr_hip.h: a detection is "matched" when
the greedy walk found a ground truth, not when the stored ground-truth ID is truthy (pycocotools reads an annotation id of 0 as unmatched).
"""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]


def results_from_packed(image_ids, packed):
    """prepare_for_coco_detection (datasets/coco_eval.py:90-112) on (B, K, 6) f32 records (score, label, x0, y0, x1, y1):
    convert_to_xywh subtracts in f32, ``.tolist()`` widens to Python floats."""
    packed = np.asarray(packed, dtype=np.float32)
    out = []
    for b, image_id in enumerate(image_ids):
        for rec in packed[b]:
            w, h = np.float32(rec[4]) - np.float32(rec[2]), np.float32(rec[5]) - np.float32(rec[3])
            label = float(rec[1])
            out.append({"image_id": int(image_id), "category_id": int(label) if label == int(label) else label,
                        "bbox": [float(rec[2]), float(rec[3]), float(w), float(h)], "score": float(rec[0])})
    return out


def bb_iou(d, g, crowd):
    """maskApi.c bbIou for one pair of xywh boxes."""
    ga = g[2] * g[3]
    da = d[2] * d[3]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


class CocoEvalRef:
    def __init__(self, dataset):
        self.img_ids_all = sorted({im["id"] for im in dataset["images"]})
        self.cat_ids = sorted({c["id"] for c in dataset["categories"]})
        self.img_to_anns = {}
        for ann in dataset["annotations"]:
            self.img_to_anns.setdefault(ann["image_id"], []).append(ann)

    # ---- COCO.loadRes + COCOeval._prepare + computeIoU + evaluateImg over the given images
    def evaluate(self, results, img_ids):
        assert set(r["image_id"] for r in results) <= set(self.img_ids_all), "Results do not correspond to current coco set"
        self.img_ids = sorted(set(img_ids))
        cats = set(self.cat_ids)
        self.gts, self.dts = {}, {}
        for img in self.img_ids:
            for ann in self.img_to_anns.get(img, []):
                if ann["category_id"] in cats:
                    g = dict(ann)
                    g["ignore"] = 1 if ("iscrowd" in g and g["iscrowd"]) else 0       # the annotation's own 'ignore' is overwritten
                    self.gts.setdefault((img, ann["category_id"]), []).append(g)
        for n, r in enumerate(results):
            if r["image_id"] in set(self.img_ids) and r["category_id"] in cats:
                d = dict(r)
                d["area"] = d["bbox"][2] * d["bbox"][3]
                d["id"] = n + 1
                d["iscrowd"] = 0
                d["slot"] = n
                self.dts.setdefault((r["image_id"], r["category_id"]), []).append(d)
        self.ious = {(i, c): self.compute_iou(i, c) for i in self.img_ids for c in self.cat_ids}
        self.eval_imgs = {(c, a, i): self.evaluate_img(i, c, AREA_RNG[a], MAX_DETS[-1])
                          for c in self.cat_ids for a in range(len(AREA_RNG)) for i in self.img_ids}

    def compute_iou(self, img, cat):
        gt, dt = self.gts.get((img, cat), []), self.dts.get((img, cat), [])
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in inds]
        if len(dt) > MAX_DETS[-1]:
            dt = dt[0:MAX_DETS[-1]]
        if len(dt) == 0 or len(gt) == 0:
            return []
        ious = np.zeros((len(dt), len(gt)))
        for j, g in enumerate(gt):
            for i, d in enumerate(dt):
                ious[i, j] = bb_iou(d["bbox"], g["bbox"], int(g["iscrowd"]) if "iscrowd" in g else 0)
        return ious

    def evaluate_img(self, img, cat, a_rng, max_det):
        gt, dt = self.gts.get((img, cat), []), self.dts.get((img, cat), [])
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            g["_ignore"] = 1 if (g["ignore"] or (g["area"] < a_rng[0] or g["area"] > a_rng[1])) else 0
        gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[0:max_det]]
        iscrowd = [int(o["iscrowd"]) if "iscrowd" in o else 0 for o in gt]
        ious = self.ious[img, cat][:, gtind] if len(self.ious[img, cat]) > 0 else self.ious[img, cat]
        T, G, D = len(IOU_THRS), len(gt), len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        gt_ig = np.array([g["_ignore"] for g in gt])
        dt_ig = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(IOU_THRS):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = 1                 # "has a gt" (pycocotools stores gt[m]['id'] and tests it for truth)
                    gtm[tind, m] = 1
        a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"dtSlots": [d["slot"] for d in dt], "dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig,
                "dtIgnore": dt_ig}

    # ---- COCOeval.accumulate
    def accumulate(self):
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(self.cat_ids), len(AREA_RNG), len(MAX_DETS)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        scores = -np.ones((T, R, K, A, M))
        self.npig = np.zeros((K, A), dtype=np.int64)
        for k, cat in enumerate(self.cat_ids):
            for a in range(A):
                for m, max_det in enumerate(MAX_DETS):
                    E = [self.eval_imgs[cat, a, i] for i in self.img_ids]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                    inds = np.argsort(-dt_scores, kind="mergesort")
                    dt_scores_sorted = dt_scores[inds]
                    dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                    npig = np.count_nonzero(gt_ig == 0)
                    self.npig[k, a] = npig
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dt_ig))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp = np.array(tp)
                        fp = np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,))
                        ss = np.zeros((R,))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = pr.tolist()
                        q = q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, REC_THRS, side="left")
                        try:
                            for ri, pi in enumerate(inds):
                                q[ri] = pr[pi]
                                ss[ri] = dt_scores_sorted[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
                        scores[t, :, k, a, m] = np.array(ss)
        self.eval = {"counts": [T, R, K, A, M], "precision": precision, "recall": recall, "scores": scores}
        return self.eval

    # ---- COCOeval.summarize (the numbers)
    def summarize(self):
        def one(ap, iou_thr=None, area=0, max_dets=100):
            m = MAX_DETS.index(max_dets)
            s = self.eval["precision"] if ap == 1 else self.eval["recall"]
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, :, area, m] if ap == 1 else s[:, :, area, m]
            return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        stats = np.zeros((12,))
        stats[0] = one(1)
        stats[1] = one(1, iou_thr=.5)
        stats[2] = one(1, iou_thr=.75)
        stats[3], stats[4], stats[5] = one(1, area=1), one(1, area=2), one(1, area=3)
        stats[6], stats[7], stats[8] = one(0, max_dets=1), one(0, max_dets=10), one(0, max_dets=100)
        stats[9], stats[10], stats[11] = one(0, area=1), one(0, area=2), one(0, area=3)
        self.stats = stats
        return stats

    # ---- the per-detection view the kernels are compared in
    def detection_table(self, n_slots):
        """For results slot n: (category index, rank, 40-bit matched mask, 40-bit ignored mask), bit = area * 10 + threshold;
        category -1 for a result that takes no part (unknown category, rank >= 100)."""
        cat = -np.ones(n_slots, dtype=np.int64)
        rank = -np.ones(n_slots, dtype=np.int64)
        matched = np.zeros(n_slots, dtype=np.int64)
        ignored = np.zeros(n_slots, dtype=np.int64)
        for (c, a, _img), e in self.eval_imgs.items():
            if e is None:
                continue
            for r, slot in enumerate(e["dtSlots"]):
                cat[slot] = self.cat_ids.index(c)
                rank[slot] = r
                for t in range(len(IOU_THRS)):
                    if e["dtMatches"][t, r]:
                        matched[slot] |= 1 << (a * 10 + t)
                    if e["dtIgnore"][t, r]:
                        ignored[slot] |= 1 << (a * 10 + t)
        return cat, rank, matched, ignored
