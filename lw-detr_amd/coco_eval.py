"""Native COCO box evaluator: the reference's ``CocoEvaluator`` (``datasets/coco_eval.py:33-78``) without pycocotools.

The reference class wraps ``pycocotools.cocoeval.COCOeval``; here the per-image matching (``evaluateImg``) and the precision / recall
curves (``accumulate``) run as HIP kernels (``csrc/cocoeval.hip``) in f64 in COCOeval's operation order, so the numbers are COCOeval's
bit for bit. The detections stay on the device: ``update`` builds the ``(B, K, 6)`` record that ``PostProcess.select_packed`` writes,
``update_packed`` takes that record directly, and only the result arrays cross to the host in ``accumulate``.

    evaluator = CocoEvaluator(base_ds, ("bbox",))        # base_ds: a COCO dict, a JSON path, or anything with a ``.dataset`` dict
    evaluator.update({image_id: {"scores", "labels", "boxes"}, ...})
    evaluator.synchronize_between_processes(); evaluator.accumulate(); evaluator.summarize()
    evaluator.coco_eval["bbox"].stats                     # numpy (12,)

Not reproduced from pycocotools: it tests the stored ground-truth ID for truth when it asks whether a detection is matched, so an
annotation with ``id`` 0 reads as unmatched there; here "matched" means "has a ground truth". Category ids must be below 2^24 (they travel
as f32 in the detection record). Limits (refused, never truncated): 1024 detections per image, 256 annotations per (image, category),
1024 categories.
"""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _native as N

# Params.setDetParams of pycocotools/cocoeval.py, expression for expression
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_RNG_LBL = ["all", "small", "medium", "large"]
_REC_COLS = 7            # per-detection record of the store: entry, image row, category, rank, score bits, matched mask, ignored mask


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data if a.size else None
    return a.data_ptr() if a.numel() else None


class CocoGroundTruth:
    """The ground truth of a COCO-format dataset packed for the kernels: image rows in ascending image id, categories dense in ascending
    category id, every image's annotations grouped by category with the dataset order kept inside a group (``COCO.getAnnIds`` /
    ``COCOeval._prepare``). Annotations of unknown images or categories take no part, as in COCOeval. No pycocotools import."""

    def __init__(self, source):
        if isinstance(source, (str, os.PathLike)):
            with open(source) as f:
                ds = json.load(f)
        elif isinstance(source, dict):
            ds = source
        elif isinstance(getattr(source, "dataset", None), dict):
            ds = source.dataset
        else:
            raise TypeError("CocoGroundTruth: expected a COCO dict, a path to a JSON file or an object with a .dataset dict, got "
                            f"{type(source).__name__}")
        self.dataset = ds
        self.img_ids = np.unique(np.asarray([im["id"] for im in ds.get("images", [])], dtype=np.int64))
        self.cat_ids = np.unique(np.asarray([c["id"] for c in ds.get("categories", [])], dtype=np.int64))
        if self.cat_ids.size == 0:
            raise ValueError("CocoGroundTruth: the dataset lists no categories")
        if self.cat_ids[0] < 0 or self.cat_ids[-1] >= 2 ** 24:
            raise ValueError("CocoGroundTruth: category ids must lie in [0, 2^24) (they travel as f32 in the detection record)")
        n_img, n_cat = len(self.img_ids), len(self.cat_ids)
        anns = ds.get("annotations", [])
        img = np.asarray([a["image_id"] for a in anns], dtype=np.int64)
        cat = np.asarray([a["category_id"] for a in anns], dtype=np.int64)
        row = np.searchsorted(self.img_ids, img)
        k = np.searchsorted(self.cat_ids, cat)
        known = np.zeros(len(anns), dtype=bool)
        if len(anns):
            known = (row < n_img) & (k < n_cat)
            known[known] = (self.img_ids[row[known]] == img[known]) & (self.cat_ids[k[known]] == cat[known])
        sel = np.nonzero(known)[0]
        key = row[sel] * n_cat + k[sel]
        order = sel[np.argsort(key, kind="stable")]                       # dataset order kept inside a (row, category) group
        counts = np.bincount(key, minlength=n_img * n_cat) if n_img else np.zeros(0, dtype=np.int64)
        if len(order) >= 2 ** 31:
            raise N.NativeError("lwdetr_amd: more than 2^31 - 1 annotations")
        self.grp_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.box = np.asarray([anns[i]["bbox"] for i in order], dtype=np.float64).reshape(-1, 4)
        self.area = np.asarray([anns[i]["area"] for i in order], dtype=np.float64)
        self.crowd = np.asarray([1 if ("iscrowd" in anns[i] and anns[i]["iscrowd"]) else 0 for i in order], dtype=np.uint8)
        self.cat = k[order].astype(np.int32)
        self.cat_lut = np.full(int(self.cat_ids[-1]) + 1, -1, dtype=np.int32)
        self.cat_lut[self.cat_ids] = np.arange(n_cat, dtype=np.int32)
        self.max_group = int(counts.max()) if counts.size else 0
        self._host = None
        self._dev = {}

    def _struct(self, t):
        return N.CocoGt(_ptr(t.grp_off), _ptr(t.box), _ptr(t.area), _ptr(t.crowd), _ptr(t.cat), _ptr(t.cat_lut), len(self.img_ids),
                        len(self.cat_ids), len(self.cat_lut), len(self.area), self.max_group, 0)

    def host_tables(self):
        if self._host is None:
            t = SimpleNamespace(grp_off=self.grp_off, box=self.box, area=self.area, crowd=self.crowd, cat=self.cat, cat_lut=self.cat_lut)
            t.struct = self._struct(t)
            self._host = t
        return self._host

    def tables(self, device):
        """The tables on ``device``, uploaded once per device."""
        device = torch.device(device)
        if device.type != "cuda":
            raise N.NativeError("lwdetr_amd: the evaluator's tables live on a ROCm device (cuda:N)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._dev.get(device)
        if t is None:
            t = SimpleNamespace(**{n: torch.from_numpy(getattr(self, n)).to(device)
                                   for n in ("grp_off", "box", "area", "crowd", "cat", "cat_lut")})
            t.img_ids = torch.from_numpy(self.img_ids).to(device)
            t.struct = self._struct(t)
            self._dev[device] = t
        return t

    def rows_of(self, image_ids):
        """Rows of the table for a host sequence of image ids; ``ValueError`` for an id the ground truth does not hold (``loadRes``
        asserts the same)."""
        ids = np.asarray([int(i) for i in image_ids], dtype=np.int64).reshape(-1)
        rows = np.searchsorted(self.img_ids, ids)
        ok = rows < len(self.img_ids)
        ok[ok] = self.img_ids[rows[ok]] == ids[ok]
        if not ok.all():
            raise ValueError(f"CocoEvaluator: image ids {ids[~ok].tolist()[:8]} are not in the ground truth")
        return rows.astype(np.int32)


def match_host(coco_gt, image_ids, packed):
    """``lwdetr_cocoeval_match_host``: the per-image matching of one batch on host arrays - the kernel's per-(image, category) code with the
    lanes emulated. ``packed`` (B, K, 6) f32 numpy. Returns numpy ``cat, score, rank, matched, ignored`` of shape (B, K)."""
    packed = np.ascontiguousarray(packed, dtype=np.float32)
    assert packed.ndim == 3 and packed.shape[2] == 6, packed.shape
    B, K = packed.shape[:2]
    rows = coco_gt.rows_of(image_ids)
    assert len(rows) == B
    out = (np.empty((B, K), np.int32), np.empty((B, K), np.float32), np.empty((B, K), np.int32), np.empty((B, K), np.int64),
           np.empty((B, K), np.int64))
    thr = np.ascontiguousarray(IOU_THRS, dtype=np.float64)
    N.check(N.lib().lwdetr_cocoeval_match_host(C.byref(coco_gt.host_tables().struct), _ptr(packed), _ptr(rows), B, K, _ptr(thr),
                                               *(_ptr(o) for o in out)), "cocoeval_match_host")
    return dict(zip(("cat", "score", "rank", "matched", "ignored"), out))


def first_occurrence(keys):
    """Boolean mask over a 1-D integer tensor: True where the value appears for the first time. An image seen twice - on one rank or on
    two, ``DistributedSampler`` pads by repetition - counts once and the first occurrence wins, as ``merge``'s
    ``np.unique(..., return_index=True)`` (coco_eval.py:181-200) keeps it. Pure tensor code, any device."""
    keys = keys.reshape(-1)
    if keys.numel() == 0:
        return torch.zeros(0, dtype=torch.bool, device=keys.device)
    s, perm = torch.sort(keys, stable=True)
    head = torch.ones_like(s, dtype=torch.bool)
    head[1:] = s[1:] != s[:-1]
    mask = torch.zeros_like(head)
    mask[perm] = head
    return mask


def score_order_key(cat, score):
    """int64 key whose ascending STABLE sort orders by (category, descending score): the f32 score mapped to a monotone integer
    (-0 = +0, NaN last as numpy's argsort(-score) puts it). Pure tensor code."""
    s = score.to(torch.float32) + 0.0
    bits = s.contiguous().view(torch.int32).to(torch.int64)
    key = torch.where(bits < 0, bits ^ 0x7FFFFFFF, bits)
    key = torch.where(torch.isnan(s), torch.full_like(key, -2 ** 31), key)
    return cat.to(torch.int64) * 2 ** 32 + (2 ** 31 - 1 - key)


def summarize_stats(precision, recall, quiet=False):
    """COCOeval.summarize: the twelve numbers (means over entries > -1, else -1) and, unless ``quiet``, its twelve lines."""
    def _one(ap, iou_thr=None, area="all", max_dets=100):
        a = AREA_RNG_LBL.index(area)
        m = MAX_DETS.index(max_dets)
        s = precision if ap == 1 else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, a, m] if ap == 1 else s[:, :, a, m]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        if not quiet:
            iou = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1]) if iou_thr is None else "{:0.2f}".format(iou_thr)
            print(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
                "Average Precision" if ap == 1 else "Average Recall", "(AP)" if ap == 1 else "(AR)", iou, area, max_dets, mean_s))
        return mean_s
    stats = np.zeros((12,))
    stats[0] = _one(1)
    stats[1] = _one(1, iou_thr=.5, max_dets=MAX_DETS[2])
    stats[2] = _one(1, iou_thr=.75, max_dets=MAX_DETS[2])
    stats[3] = _one(1, area="small", max_dets=MAX_DETS[2])
    stats[4] = _one(1, area="medium", max_dets=MAX_DETS[2])
    stats[5] = _one(1, area="large", max_dets=MAX_DETS[2])
    stats[6] = _one(0, max_dets=MAX_DETS[0])
    stats[7] = _one(0, max_dets=MAX_DETS[1])
    stats[8] = _one(0, max_dets=MAX_DETS[2])
    stats[9] = _one(0, area="small", max_dets=MAX_DETS[2])
    stats[10] = _one(0, area="medium", max_dets=MAX_DETS[2])
    stats[11] = _one(0, area="large", max_dets=MAX_DETS[2])
    return stats


class BboxEval:
    """What ``coco_evaluator.coco_eval['bbox']`` is in the reference (a COCOeval): ``params``, ``eval`` and ``stats``."""

    def __init__(self, coco_gt):
        self.params = SimpleNamespace(iouType="bbox", useCats=1, imgIds=[], catIds=coco_gt.cat_ids.tolist(), iouThrs=IOU_THRS,
                                      recThrs=REC_THRS, maxDets=list(MAX_DETS), areaRng=[list(a) for a in AREA_RNG],
                                      areaRngLbl=list(AREA_RNG_LBL))
        self.eval = {}
        self.stats = []

    def summarize(self):
        if not self.eval:
            raise Exception("Please run accumulate() first")
        self.stats = summarize_stats(self.eval["precision"], self.eval["recall"])


class CocoEvaluator:
    """Drop-in for the reference's ``CocoEvaluator`` (``datasets/coco_eval.py:33-78``) for ``iou_types = ('bbox',)``."""

    def __init__(self, coco_gt, iou_types):
        assert isinstance(iou_types, (list, tuple))
        for t in iou_types:
            if t in ("segm", "keypoints"):
                raise NotImplementedError(f"CocoEvaluator: iou type {t!r} is not implemented (boxes only)")
            if t != "bbox":
                raise ValueError("Unknown iou type {}".format(t))
        self.coco_gt = coco_gt if isinstance(coco_gt, CocoGroundTruth) else CocoGroundTruth(coco_gt)
        self.iou_types = iou_types
        self.coco_eval = {t: BboxEval(self.coco_gt) for t in iou_types}
        self.img_ids = []
        self.collectives_run = 0
        self._batches = []
        self._store = None

    # ------------------------------------------------------------------------------------------------------------ per batch
    def update(self, predictions):
        """``{image_id: {"scores", "labels", "boxes"}}`` as ``engine.py:144`` builds it; device or host tensors, f32 / f16 / bf16 scores
        and boxes (widened to f32: other f32 values, nothing else). No per-image ``.tolist()``."""
        ids = list(predictions.keys())
        rows = self.coco_gt.rows_of(ids)
        self.img_ids.extend(list(np.unique(ids)) if ids else [])
        if not ids or "bbox" not in self.coco_eval:
            return
        preds = [predictions[i] for i in ids]
        device = next((p[f].device for p in preds if len(p) for f in ("scores", "labels", "boxes") if p[f].is_cuda), None)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        counts = [int(p["scores"].shape[0]) if len(p) else 0 for p in preds]
        K = max(counts)
        if min(counts) == K and K > 0:
            sc = torch.stack([p["scores"] for p in preds]).to(device=device, dtype=torch.float32)
            lb = torch.stack([p["labels"] for p in preds]).to(device=device, dtype=torch.float32)
            bx = torch.stack([p["boxes"] for p in preds]).to(device=device, dtype=torch.float32)
            packed = torch.cat([sc.unsqueeze(-1), lb.unsqueeze(-1), bx.reshape(len(preds), K, 4)], dim=-1)
        else:                                             # ragged: pad with label -1, which is no category and is dropped
            packed = torch.zeros((len(preds), K, 6), dtype=torch.float32, device=device)
            packed[:, :, 1] = -1.0
            for b, (p, n) in enumerate(zip(preds, counts)):
                if n:
                    packed[b, :n, 0] = p["scores"].to(device=device, dtype=torch.float32)
                    packed[b, :n, 1] = p["labels"].to(device=device, dtype=torch.float32)
                    packed[b, :n, 2:] = p["boxes"].to(device=device, dtype=torch.float32).reshape(n, 4)
        self._match(torch.from_numpy(rows).to(device), packed.contiguous())

    def update_packed(self, image_ids, packed):
        """One batch as the ``(B, K, 6)`` f32 device record of ``model.detect`` / ``PostProcess.select_packed``. ``image_ids``: a host
        sequence (checked at once: ``ValueError`` for an unknown id) or a DEVICE integer tensor - then nothing touches the host (the call
        can be captured in a HIP graph) and an unknown id raises at ``synchronize_between_processes``."""
        if "bbox" not in self.coco_eval:
            return
        N.require_cuda(packed)
        if packed.dim() != 3 or packed.shape[2] != 6 or packed.dtype != torch.float32:
            raise N.NativeError(f"lwdetr_amd: update_packed expects a (B, K, 6) float32 record, got {tuple(packed.shape)} {packed.dtype}")
        if torch.is_tensor(image_ids) and image_ids.is_cuda:
            t = self.coco_gt.tables(packed.device)
            ids = image_ids.to(torch.int64).reshape(-1)
            n = t.img_ids.numel()
            pos = torch.searchsorted(t.img_ids, ids).clamp(max=max(n - 1, 0))
            rows = torch.where(t.img_ids[pos] == ids, pos, torch.full_like(pos, -1)).to(torch.int32) if n else \
                torch.full_like(ids, -1, dtype=torch.int32)
            self._match(rows, packed.contiguous(), dev_ids=ids)
        else:
            ids = [int(i) for i in (image_ids.tolist() if torch.is_tensor(image_ids) else image_ids)]
            rows = self.coco_gt.rows_of(ids)
            self.img_ids.extend(list(np.unique(ids)) if ids else [])
            self._match(torch.from_numpy(rows).to(packed.device), packed.contiguous())

    def _match(self, rows, packed, dev_ids=None):
        B, K = packed.shape[:2]
        if rows.numel() != B:
            raise N.NativeError(f"lwdetr_amd: {rows.numel()} image ids for a batch of {B}")
        dev = packed.device
        t = self.coco_gt.tables(dev)
        out = (torch.empty((B, K), dtype=torch.int32, device=dev), torch.empty((B, K), dtype=torch.float32, device=dev),
               torch.empty((B, K), dtype=torch.int32, device=dev), torch.empty((B, K), dtype=torch.int64, device=dev),
               torch.empty((B, K), dtype=torch.int64, device=dev))
        thr = np.ascontiguousarray(IOU_THRS, dtype=np.float64)
        with torch.cuda.device(dev):
            N.check(N.lib().lwdetr_cocoeval_match(C.byref(t.struct), _ptr(packed), _ptr(rows), B, K, _ptr(thr), *(_ptr(o) for o in out),
                                                  N.stream_ptr(dev)), "cocoeval_match")
        self._batches.append(SimpleNamespace(rows=rows, K=K, out=out, dev_ids=dev_ids))
        self._store = None
        return out

    # ------------------------------------------------------------------------------------------------------------ gather
    def _device(self):
        return self._batches[0].rows.device if self._batches else torch.device("cuda", torch.cuda.current_device())

    def _local_records(self):
        """(entries (E,) int64 = the image row of every (batch, image) in arrival order, records (N, 7) int64 of the kept detections)."""
        dev = self._device()
        ents, recs, base = [], [], 0
        for bt in self._batches:
            B, K = bt.rows.numel(), bt.K
            rows = bt.rows.to(device=dev, dtype=torch.int64)
            ents.append(rows)
            cat, score, rank, matched, ignored = (o.to(dev).reshape(-1) for o in bt.out)
            entry = (torch.arange(B, device=dev, dtype=torch.int64) + base).repeat_interleave(K)
            rec = torch.stack([entry, rows.repeat_interleave(K), cat.to(torch.int64), rank.to(torch.int64),
                               score.contiguous().view(torch.int32).to(torch.int64), matched, ignored], dim=1)
            recs.append(rec[cat >= 0])
            base += B
        if not ents:
            return torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros((0, _REC_COLS), dtype=torch.int64, device=dev)
        return torch.cat(ents), torch.cat(recs)

    @staticmethod
    def _all_gather_var(t):
        """all_gather of tensors whose first dimension differs between ranks: sizes first, then padded blocks; tensor collectives only."""
        import torch.distributed as dist
        world = dist.get_world_size()
        n = torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)
        sizes = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(sizes, n)
        sizes = [int(s.item()) for s in sizes]
        cap = max(max(sizes), 1)
        pad = torch.zeros((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        pad[:t.shape[0]] = t
        blocks = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(blocks, pad)
        return [b[:s] for b, s in zip(blocks, sizes)]

    def synchronize_between_processes(self):
        """Leaves every rank with the full store (as the reference leaves every rank able to ``accumulate``). With ``torch.distributed``
        initialised the per-detection records travel through tensor collectives - no pickles; shard sizes may differ between ranks."""
        for bt in self._batches:                          # batches whose ids arrived as device tensors: the deferred part of update_packed
            if bt.dev_ids is not None:
                ids = bt.dev_ids.tolist()
                self.coco_gt.rows_of(ids)
                self.img_ids.extend(list(np.unique(ids)) if ids else [])
                bt.dev_ids = None
        entries, recs = self._local_records()
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            e_parts = self._all_gather_var(entries)
            r_parts = self._all_gather_var(recs)
            base = 0
            for e, r in zip(e_parts, r_parts):
                r[:, 0] += base
                base += e.shape[0]
            entries, recs = torch.cat(e_parts), torch.cat(r_parts)
            self.collectives_run += 1
        keep = first_occurrence(entries)
        recs = recs[keep[recs[:, 0]]] if recs.shape[0] else recs
        rows_eval = torch.sort(entries[keep]).values.to(torch.int32)
        self._store = SimpleNamespace(rows=rows_eval, recs=recs)
        img_ids = self.coco_gt.img_ids[rows_eval.cpu().numpy()].tolist()
        for ev in self.coco_eval.values():
            ev.params.imgIds = img_ids

    # ------------------------------------------------------------------------------------------------------------ curves
    def accumulate(self):
        if "bbox" not in self.coco_eval:
            return
        if self._store is None:
            self.synchronize_between_processes()
        st, gt = self._store, self.coco_gt
        dev = st.recs.device
        t = gt.tables(dev)
        n_cats = len(gt.cat_ids)
        recs = st.recs
        # COCOeval's accumulate mergesorts by descending score over the per-image lists concatenated in sorted image id order. The store
        # holds the detections of an image in detection order, so: a stable sort by image row, then ONE stable torch.sort on the composite
        # (category, descending score) key - plumbing, not arithmetic; the kernel below reads the result.
        o1 = torch.sort(recs[:, 1], stable=True).indices
        recs = recs[o1]
        score = recs[:, 4].to(torch.int32).view(torch.float32)
        o2 = torch.sort(score_order_key(recs[:, 2], score), stable=True).indices
        recs = recs[o2]
        cat = recs[:, 2].contiguous()
        score = score[o2].contiguous()
        rank = recs[:, 3].to(torch.int32).contiguous()
        matched, ignored = recs[:, 5].contiguous(), recs[:, 6].contiguous()
        seg_off = torch.searchsorted(cat, torch.arange(n_cats + 1, device=dev, dtype=torch.int64)).contiguous()
        npig = torch.empty((n_cats, 4), dtype=torch.int32, device=dev)
        T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
        precision = torch.full((T, R, n_cats, A, M), -1.0, dtype=torch.float64, device=dev)
        scores = torch.full((T, R, n_cats, A, M), -1.0, dtype=torch.float64, device=dev)
        recall = torch.full((T, n_cats, A, M), -1.0, dtype=torch.float64, device=dev)
        rec_thrs = np.ascontiguousarray(REC_THRS, dtype=np.float64)
        lib = N.lib()
        with torch.cuda.device(dev):
            N.check(lib.lwdetr_cocoeval_npig(C.byref(t.struct), _ptr(st.rows), st.rows.numel(), _ptr(npig), N.stream_ptr(dev)),
                    "cocoeval_npig")
            N.check(lib.lwdetr_cocoeval_curves(_ptr(seg_off), _ptr(score), _ptr(rank), _ptr(matched), _ptr(ignored), _ptr(npig),
                                               _ptr(rec_thrs), n_cats, recs.shape[0], _ptr(precision), _ptr(scores), _ptr(recall),
                                               N.stream_ptr(dev)), "cocoeval_curves")
        ev = self.coco_eval["bbox"]
        ev.eval = {"params": ev.params, "counts": [T, R, n_cats, A, M], "precision": precision.cpu().numpy(),
                   "recall": recall.cpu().numpy(), "scores": scores.cpu().numpy(), "npig": npig.cpu().numpy()}
        ev.stats = summarize_stats(ev.eval["precision"], ev.eval["recall"], quiet=True)
        self.sorted_store = SimpleNamespace(cat=cat, score=score, rank=rank, matched=matched, ignored=ignored, row=recs[:, 1])

    def summarize(self):
        for iou_type, coco_eval in self.coco_eval.items():
            print("IoU metric: {}".format(iou_type))
            coco_eval.summarize()
