"""TEST INFRASTRUCTURE ONLY - numpy restatement of the staged, crop-window algorithm of csrc/augment.hip, built on the Pillow-pinned
resampler of oracle/preprocess_ref.py (``resample_coeffs`` / ``_resample_axis``, imported), plus the loaders of tests/golden/augment.npz
and the deterministic images that the fixture's large cases and the GPU shape sweep are generated from."""
import os

import numpy as np
import torch

from oracle.preprocess_ref import PRECISION_BITS, _resample_axis, resample_coeffs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz")
TARGET_KEYS = ("boxes", "labels", "image_id", "area", "iscrowd", "orig_size", "size")
SUB = (37, 41)                       # row / column stride of the stored subsample of a default-parameter case


def synth_image(h, w, seed):
    """(h, w, 3) uint8, noise-like, from integer arithmetic only (the same bytes on every machine)."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(3, dtype=np.uint64), indexing="ij")
    v = (x * np.uint64(73856093)) ^ (y * np.uint64(19349663)) ^ (c * np.uint64(83492791)) ^ np.uint64(seed * 2654435761 + 12345)
    v = (v * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    return ((v >> np.uint64(41)) & np.uint64(255)).astype(np.uint8)


def _resample_window(img, out_size, axis, start, count):
    """Output positions [start, start + count) of the resample of ``img`` along ``axis`` to ``out_size``: the taps of the full axis."""
    a = np.moveaxis(img, axis, 0).astype(np.int64)
    bounds, k = resample_coeffs(a.shape[0], out_size)
    out = np.empty((count,) + a.shape[1:], np.uint8)
    for i in range(count):
        xmin, n = bounds[start + i]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k[start + i, :n].astype(np.int64), a[xmin:xmin + n], axes=(0, 0))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def augment_u8(img, flip, resize1, crop, out_size):
    """(H, W, 3) uint8 -> (oh, ow, 3) uint8: flip, stage 1 (resize to ``resize1``, computed for the ``crop`` window only), stage 2 (resize to
    ``out_size``); horizontal pass first, uint8 between passes and stages, a pass with equal lengths skipped."""
    a = np.ascontiguousarray(img)
    if flip:
        a = a[:, ::-1]
    h, w = a.shape[:2]
    h1, w1 = resize1 if resize1 is not None else (h, w)
    top, left, ch, cw = crop if crop is not None else (0, 0, h1, w1)
    a = _resample_window(a, w1, 1, left, cw) if w1 != w else a[:, left:left + cw]
    a = _resample_window(a, h1, 0, top, ch) if h1 != h else a[top:top + ch]
    oh, ow = out_size
    if ow != cw:
        a = _resample_axis(a, ow, 1)
    if oh != ch:
        a = _resample_axis(a, oh, 0)
    return np.ascontiguousarray(a)


def augment_params_u8(img, params):
    return augment_u8(img, params.flip, params.resize1, params.crop, params.out_size)


def lut_f32(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    v = torch.arange(256, dtype=torch.float32).view(1, 256)
    return v.div(255).sub(torch.tensor(mean).view(3, 1)).div(torch.tensor(std).view(3, 1))


def expected_batch(u8_list, table, dtype=torch.float32):
    """[(oh, ow, 3) uint8] -> (batch (B,3,Hc,Wc), mask (B,Hc,Wc) bool) as nested_tensor_from_tensor_list pads table[uint8]."""
    hc = max((u.shape[0] for u in u8_list), default=0)
    wc = max((u.shape[1] for u in u8_list), default=0)
    batch = torch.zeros(len(u8_list), 3, hc, wc, dtype=torch.float32)
    mask = torch.ones(len(u8_list), hc, wc, dtype=torch.bool)
    for i, u in enumerate(u8_list):
        idx = torch.from_numpy(np.ascontiguousarray(u)).long()
        oh, ow = u.shape[:2]
        for c in range(3):
            batch[i, c, :oh, :ow] = table[c][idx[:, :, c]]
        mask[i, :oh, :ow] = False
    return batch.to(dtype), mask


def recover_u8(planes, table):
    """(3, oh, ow) f32 produced through ``table`` -> (oh, ow, 3) uint8 (the table is strictly increasing per channel)."""
    out = [torch.searchsorted(table[c].contiguous(), planes[c].contiguous().float()) for c in range(3)]
    u = torch.stack(out, -1)
    assert all(torch.equal(table[c][u[..., c].clamp(max=255)], planes[c].float()) for c in range(3)), "a value that is not in the table"
    return u.to(torch.uint8).numpy()


def clipped_to_zero_width(boxes, params, src_size):
    """How many boxes (xyxy in source pixels) the crop of ``params`` leaves with no width but some height - the boxes that lie wholly to the
    left or right of the window while overlapping its rows. Plain float arithmetic; it selects and describes a fixture case, nothing more."""
    if params.crop is None:
        return 0
    h, w = src_size
    h1, w1 = params.resize1 if params.resize1 is not None else (h, w)
    top, left, ch, cw = params.crop
    n = 0
    for x0, y0, x1, y1 in boxes.tolist():
        if params.flip:
            x0, x1 = w - x1, w - x0
        x0, x1 = (min(max(v * w1 / w - left, 0.0), cw) for v in (x0, x1))
        y0, y1 = (min(max(v * h1 / h - top, 0.0), ch) for v in (y0, y1))
        n += x1 <= x0 and y1 > y0
    return n


class Case:
    """One golden case: recipe, seed, source image, annotations, the reference's uint8 output (or its digest) and its targets."""

    def __init__(self, g, i):
        p = f"c{i}_"
        self.index, self.name = i, str(g[p + "name"])
        self.seed = int(g[p + "seed"])
        self.square = bool(g[p + "square"])
        self.scales = [int(v) for v in g[p + "scales"]]
        self.resize_sizes = [int(v) for v in g[p + "resize_sizes"]]
        self.crop_range = tuple(int(v) for v in g[p + "crop_range"])
        self.max_size = int(g[p + "max_size"]) if int(g[p + "max_size"]) > 0 else None
        self.image_id = int(g[p + "image_id"])
        if p + "image" in g.files:
            self.image = g[p + "image"]
        else:
            h, w, s = (int(v) for v in g[p + "image_synth"])
            self.image = synth_image(h, w, s)
        self.annotations = []
        for bbox, cat, area, crowd in zip(g[p + "ann_bbox"], g[p + "ann_category"], g[p + "ann_area"], g[p + "ann_iscrowd"]):
            obj = {"bbox": [float(v) for v in bbox], "category_id": int(cat), "area": float(area)}
            if int(crowd) >= 0:                  # -1: the annotation carries no iscrowd key
                obj["iscrowd"] = int(crowd)
            self.annotations.append(obj)
        self.out = g[p + "out"] if p + "out" in g.files else None
        self.out_shape = tuple(int(v) for v in g[p + "out_shape"])
        self.out_sha256 = str(g[p + "out_sha256"])
        self.out_sub = g[p + "out_sub"]
        self.converted = {k: torch.from_numpy(g[p + "cv_" + k]) for k in TARGET_KEYS}
        self.target = {k: torch.from_numpy(g[p + "tg_" + k]) for k in TARGET_KEYS}

    @property
    def recipe(self):
        return dict(square=self.square, scales=self.scales, resize_sizes=self.resize_sizes, crop_range=self.crop_range, max_size=self.max_size)

    def sample(self):
        """The parameters lwdetr_amd draws for this case's image under the case's seed."""
        import random
        from lwdetr_amd.augment import sample_train_params
        random.seed(self.seed)
        torch.manual_seed(self.seed)
        return sample_train_params(self.image.shape[1], self.image.shape[0], **self.recipe)


def load_cases():
    g = np.load(GOLD, allow_pickle=False)
    return g, [Case(g, i) for i in range(int(g["num_cases"]))]
