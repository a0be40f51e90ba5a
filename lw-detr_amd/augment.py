"""Training-time input transforms on the GPU: the reference's train recipes

    make_coco_transforms_square_div_64('train')  /  make_coco_transforms('train')          (datasets/coco.py:86-160)
      = Compose([RandomHorizontalFlip(), RandomSelect(resize, Compose([RandomResize([400, 500, 600]), RandomSizeCrop(384, 600), resize])),
                 ToTensor(), Normalize(mean, std)])                                         (datasets/transforms.py)

followed by the collate's ``nested_tensor_from_tensor_list`` (util/misc.py:317-339), as one call on a batch of uint8 images. The random
draws are made here, on the host, by the same calls in the same order on the same generators as the reference's ``Compose`` makes them
(``sample_train_params``), the boxes follow on the host in the reference's own f32 torch operations (``transform_target``), and the pixels
are produced by ``csrc/augment.hip``: Pillow's fixed-point resampler per stage, bit for bit, flip and crop folded into the passes, padding
and mask out of the last launch. There is no CPU implementation of the pixel path here."""
import ctypes as C
import dataclasses
import random
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native as _nat
from .models.nested import NestedTensor
from .preprocess import IMAGENET_MEAN, IMAGENET_STD, SquareResizeNormalize, resample_tables

SQUARE_SCALES = (448, 512, 576, 640, 704, 768, 832, 896)                             # datasets/coco.py:133
ASPECT_SCALES = (480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800)              # datasets/coco.py:93
ASPECT_MAX_SIZE = 1333
GRID_LIMIT = 65535


class AugmentImage(C.Structure):      # mirrors lwdetr_augment_image (include/lwdetr_hip.h)
    _fields_ = [("src", C.c_void_p), ("height", C.c_int), ("width", C.c_int), ("row_stride", C.c_long), ("flip", C.c_int),
                ("h1", C.c_int), ("w1", C.c_int), ("top", C.c_int), ("left", C.c_int), ("ch", C.c_int), ("cw", C.c_int),
                ("oh", C.c_int), ("ow", C.c_int), ("row0", C.c_int), ("rows", C.c_int),
                ("bounds_off", C.c_int * 4), ("coef_off", C.c_int * 4), ("ksize", C.c_int * 4), ("scratch_off", C.c_long * 3)]


@dataclasses.dataclass
class AugmentParams:
    """One image's outcome of the train recipe's draws. ``resize1`` = (h1, w1) and ``crop`` = (top, left, h, w) inside it are the
    RandomResize + RandomSizeCrop branch (both None in the other branch); ``out_size`` = (oh, ow) is the last resize."""
    flip: bool
    resize1: Optional[Tuple[int, int]]
    crop: Optional[Tuple[int, int, int, int]]
    out_size: Tuple[int, int]


def short_side_size(width, height, size, max_size=None):
    """(oh, ow) that puts the shorter side of a width x height image at ``size`` and keeps the aspect ratio, the longer side truncated; with
    ``max_size``, ``size`` is first lowered so that the longer side stays within it. The same float arithmetic, in the same order, as the
    size rule of the reference's ``resize`` (datasets/transforms.py:97-115): the results are its results."""
    short, long_ = float(min(width, height)), float(max(width, height))
    if max_size is not None and long_ / short * size > max_size:
        size = int(round(max_size * short / long_))
    if min(width, height) == size:
        return (height, width)
    if width < height:
        return (int(size * height / width), size)
    return (size, int(size * width / height))


def sample_train_params(width, height, square=True, scales=None, resize_sizes=(400, 500, 600), crop_range=(384, 600), max_size=None,
                        rng=random):
    """Draws one image's AugmentParams with the calls the reference's Compose makes, in its order: rng.random() (flip), rng.random()
    (select), then rng.choice(scales) - or rng.choice(resize_sizes), rng.randint (crop width), rng.randint (crop height),
    torch.randint (top), torch.randint (left; neither when the crop is the whole image: torchvision's RandomCrop.get_params) and
    rng.choice(scales). After ``random.seed(k); torch.manual_seed(k)`` the result is what the reference does to an image of this size."""
    if scales is None:
        scales = SQUARE_SCALES if square else ASPECT_SCALES
    if max_size is None and not square:
        max_size = ASPECT_MAX_SIZE
    scales, resize_sizes = list(scales), list(resize_sizes)

    def last_resize(w, h):
        size = rng.choice(scales)
        return (size, size) if square else short_side_size(w, h, size, max_size)

    flip = rng.random() < 0.5
    if rng.random() < 0.5:
        return AugmentParams(flip, None, None, last_resize(width, height))
    h1, w1 = short_side_size(width, height, rng.choice(resize_sizes))
    cw = rng.randint(crop_range[0], min(w1, crop_range[1]))
    ch = rng.randint(crop_range[0], min(h1, crop_range[1]))
    top = left = 0
    if not (w1 == cw and h1 == ch):
        top = int(torch.randint(0, h1 - ch + 1, size=(1,)).item())
        left = int(torch.randint(0, w1 - cw + 1, size=(1,)).item())
    return AugmentParams(flip, (h1, w1), (top, left, ch, cw), last_resize(cw, ch))


def convert_coco(annotations, width, height, image_id):
    """The reference's ConvertCoco (datasets/coco.py:43-83): COCO annotation dicts of one image -> the target dict of tensors."""
    w, h = width, height
    image_id = torch.tensor([image_id])
    anno = [obj for obj in annotations if "iscrowd" not in obj or obj["iscrowd"] == 0]
    boxes = [obj["bbox"] for obj in anno]
    boxes = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    boxes[:, 2:] += boxes[:, :2]
    boxes[:, 0::2].clamp_(min=0, max=w)
    boxes[:, 1::2].clamp_(min=0, max=h)
    classes = torch.tensor([obj["category_id"] for obj in anno], dtype=torch.int64)
    keep = (boxes[:, 3] > boxes[:, 1]) & (boxes[:, 2] > boxes[:, 0])
    area = torch.tensor([obj["area"] for obj in anno])
    iscrowd = torch.tensor([obj["iscrowd"] if "iscrowd" in obj else 0 for obj in anno])
    return {"boxes": boxes[keep], "labels": classes[keep], "image_id": image_id, "area": area[keep], "iscrowd": iscrowd[keep],
            "orig_size": torch.as_tensor([int(h), int(w)]), "size": torch.as_tensor([int(h), int(w)])}


def _resize_target(target, old_wh, new_hw):
    h, w = new_hw
    ratio_width, ratio_height = tuple(float(s) / float(s_orig) for s, s_orig in zip((w, h), old_wh))
    target = target.copy()
    if "boxes" in target:
        target["boxes"] = target["boxes"] * torch.as_tensor([ratio_width, ratio_height, ratio_width, ratio_height])
    if "area" in target:
        target["area"] = target["area"] * (ratio_width * ratio_height)
    target["size"] = torch.tensor([h, w])
    return target


def _crop_target(target, region):
    target = target.copy()
    i, j, h, w = region
    target["size"] = torch.tensor([h, w])
    fields = ["labels", "area", "iscrowd"]
    if "boxes" in target:
        max_size = torch.as_tensor([w, h], dtype=torch.float32)
        cropped_boxes = target["boxes"] - torch.as_tensor([j, i, j, i])
        cropped_boxes = torch.min(cropped_boxes.reshape(-1, 2, 2), max_size)
        cropped_boxes = cropped_boxes.clamp(min=0)
        area = (cropped_boxes[:, 1, :] - cropped_boxes[:, 0, :]).prod(dim=1)
        target["boxes"] = cropped_boxes.reshape(-1, 4)
        target["area"] = area
        fields.append("boxes")
        cropped_boxes = target["boxes"].reshape(-1, 2, 2)
        keep = torch.all(cropped_boxes[:, 1, :] > cropped_boxes[:, 0, :], dim=1)
        for field in fields:
            if field in target:
                target[field] = target[field][keep]
    return target


def transform_target(target, params, src_size):
    """What the reference's hflip / resize / crop / Normalize (datasets/transforms.py:34-152, 437-453) make of a ConvertCoco target under
    ``params``, in the same f32 torch operations in the same order; ``src_size`` = (height, width) of the source image. Host tensors."""
    height, width = int(src_size[0]), int(src_size[1])
    target = target.copy()
    if params.flip and "boxes" in target:
        w = width
        target["boxes"] = target["boxes"][:, [2, 1, 0, 3]] * torch.as_tensor([-1, 1, -1, 1]) + torch.as_tensor([w, 0, w, 0])
    cur = (width, height)
    if params.resize1 is not None or params.crop is not None:
        h1, w1 = params.resize1 if params.resize1 is not None else (height, width)
        if params.resize1 is not None:
            target = _resize_target(target, cur, (h1, w1))
        region = params.crop if params.crop is not None else (0, 0, h1, w1)
        if params.crop is not None:
            target = _crop_target(target, region)
        cur = (region[3], region[2])
    target = _resize_target(target, cur, params.out_size)
    h, w = params.out_size
    if "boxes" in target:
        x0, y0, x1, y1 = target["boxes"].unbind(-1)
        boxes = torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0), (y1 - y0)], dim=-1)
        target["boxes"] = boxes / torch.tensor([w, h, w, h], dtype=torch.float32)
    return target


def _stages(params, height, width):
    """AugmentParams -> (h1, w1, top, left, ch, cw, oh, ow), validated; no stage 1 = the source size and the full window."""
    h1, w1 = (int(v) for v in params.resize1) if params.resize1 is not None else (height, width)
    top, left, ch, cw = (int(v) for v in params.crop) if params.crop is not None else (0, 0, h1, w1)
    oh, ow = (int(v) for v in params.out_size)
    if min(h1, w1, oh, ow) <= 0 or max(h1, w1, oh, ow) > GRID_LIMIT:
        raise ValueError(f"resize sizes must be in 1 ... {GRID_LIMIT}: {params}")
    if ch <= 0 or cw <= 0 or top < 0 or left < 0 or top + ch > h1 or left + cw > w1:
        raise ValueError(f"crop {(top, left, ch, cw)} is empty or outside the resized image {(h1, w1)}")
    return h1, w1, top, left, ch, cw, oh, ow


class _AxisTables:
    """Pillow's coefficient tables (preprocess.resample_tables) per (input length, output length) in one device buffer of int32 elements.
    Training draws new length pairs with every batch out of a finite set (the square recipe's stage 2: crop lengths x scales; stage 1: the
    dataset's image sides x three sizes), so nothing is ever dropped before ``limit``: a full buffer is replaced by one of twice the size
    that takes the old content over with a device copy, every offset staying valid. Only at ``limit`` elements (512 MB) does the cache
    start over with the tables of the batch at hand. The (first tap, tap count) bounds stay on the host as well: they size the stage-1
    row range."""

    def __init__(self, device, capacity=1 << 21, limit=1 << 27):
        self.device, self.limit = device, limit
        self.buf = torch.empty(capacity, dtype=torch.int32, device=device)
        self.length = 0
        self.entries = {}                    # (in, out) -> (bounds offset, coef offset, ksize, bounds (out, 2) numpy)
        self.retired = []                    # a replaced buffer: earlier (asynchronous) launches may still read it

    def require(self, pairs):
        pairs = sorted(set(pairs))
        built = {p: self._build(p) for p in pairs if p not in self.entries}
        need = sum(bo.size + co.size for bo, co, _ in built.values())
        if self.length + need > self.buf.numel():
            if self.length + need > self.limit:              # start over with this batch's tables
                built = {p: built[p] if p in built else self._build(p) for p in pairs}
                need = sum(bo.size + co.size for bo, co, _ in built.values())
                self.entries.clear()
                self.length = 0
            if self.length + need > self.buf.numel():
                grown = torch.empty(max(2 * self.buf.numel(), self.length + need), dtype=torch.int32, device=self.device)
                grown[:self.length].copy_(self.buf[:self.length])          # ordered on the stream after the launches that read the old one
                self.retired = [self.buf]
                self.buf = grown
        if built:
            off, chunks = self.length, []
            for p, (bo, co, ks) in built.items():
                self.entries[p] = (off, off + bo.size, ks, bo.reshape(-1, 2))
                chunks += [bo, co]
                off += bo.size + co.size
            self.buf[self.length:off].copy_(torch.from_numpy(np.concatenate(chunks).astype(np.int32, copy=False)))
            self.length = off

    @staticmethod
    def _build(pair):
        bounds, coef = resample_tables(*pair)
        return np.ascontiguousarray(bounds).reshape(-1), np.ascontiguousarray(coef).reshape(-1), coef.shape[1]


class TrainTransform:
    """``TrainTransform(dtype, device, square=True, ...)(images, targets, params=None) -> (NestedTensor(batch, mask), targets)``.

    ``images``: a list of uint8 tensors (H, W, 3) RGB, on the host or the device; ``targets``: one ConvertCoco dict per image (host
    tensors, ``convert_coco``); ``params``: one AugmentParams per image, or None to draw them (image by image, in order, with
    ``sample_train_params`` and this transform's recipe). ``batch`` is (B, 3, Hc, Wc) in ``dtype`` with Hc, Wc the largest output height and
    width of the batch, zero outside each image; ``mask`` (B, Hc, Wc) bool is True there. The returned targets live on ``device``."""

    def __init__(self, dtype=torch.float16, device="cuda", square=True, scales=None, resize_sizes=(400, 500, 600), crop_range=(384, 600),
                 max_size=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, rng=random):
        self.dtype, self.device = dtype, torch.device(device)
        self.recipe = dict(square=square, scales=scales, resize_sizes=resize_sizes, crop_range=crop_range, max_size=max_size)
        self.rng = rng
        m = torch.tensor(mean, dtype=torch.float32).view(3, 1)
        s = torch.tensor(std, dtype=torch.float32).view(3, 1)
        v = torch.arange(256, dtype=torch.float32).view(1, 256)
        self.lut = v.div(255).sub(m).div(s).contiguous().to(self.device)       # ToTensor, then F.normalize: same f32 ops
        self._tables = _AxisTables(self.device)
        self._keep = None

    def sample(self, width, height):
        return sample_train_params(width, height, rng=self.rng, **self.recipe)

    def prebuild(self):
        """Builds and uploads, once, every stage-2 table the square recipe can draw (crop lengths x scales: 1736 pairs, 28 MB, a few tenths
        of a second at the default parameters), so that no training batch builds one inside a call. The aspect recipe's stage-2 lengths and
        every recipe's stage-1 lengths depend on the images and are built when first met. Returns the number of pairs resident."""
        if self.recipe["square"]:
            scales = self.recipe["scales"] if self.recipe["scales"] is not None else SQUARE_SCALES
            lo, hi = self.recipe["crop_range"]
            self._tables.require([(c, int(v)) for c in range(int(lo), int(hi) + 1) for v in scales if c != int(v)])
        return len(self._tables.entries)

    def describe(self, imgs, params):
        """(descriptor array, scratch bytes, Hc, Wc) for device images and their parameters; the tables are resident afterwards."""
        geo, pairs = [], []
        for im, p in zip(imgs, params):
            h, w = int(im.shape[0]), int(im.shape[1])
            if max(h, w) > GRID_LIMIT:
                raise ValueError(f"image sides must be at most {GRID_LIMIT}")
            h1, w1, top, left, ch, cw, oh, ow = g = _stages(p, h, w)
            geo.append(g)
            pairs += [pr for pr in ((w, w1), (h, h1), (cw, ow), (ch, oh)) if pr[0] != pr[1]]
        self._tables.require(pairs)
        ent = self._tables.entries
        descs = (AugmentImage * max(len(imgs), 1))()
        off = 0
        for d, im, p, (h1, w1, top, left, ch, cw, oh, ow) in zip(descs, imgs, params, geo):
            h, w = int(im.shape[0]), int(im.shape[1])
            d.src, d.height, d.width, d.row_stride, d.flip = im.data_ptr(), h, w, im.stride(0), int(bool(p.flip))
            d.h1, d.w1, d.top, d.left, d.ch, d.cw, d.oh, d.ow = h1, w1, top, left, ch, cw, oh, ow
            d.row0, d.rows = top, ch
            for ax, pr in enumerate(((w, w1), (h, h1), (cw, ow), (ch, oh))):
                if pr[0] != pr[1]:
                    d.bounds_off[ax], d.coef_off[ax], d.ksize[ax] = ent[pr][:3]
            if h1 != h:                      # the source rows the window's rows tap
                b = ent[(h, h1)][3]
                d.row0 = int(b[top, 0])
                d.rows = int(b[top + ch - 1, 0] + b[top + ch - 1, 1]) - d.row0
            for which, (used, nbytes) in enumerate(((w1 != w, 3 * d.rows * cw), (h1 != h, 3 * ch * cw), (ow != cw, 3 * ch * ow))):
                if used:
                    d.scratch_off[which] = off
                    off += (nbytes + 15) // 16 * 16
        hc = max((g[6] for g in geo), default=0)
        wc = max((g[7] for g in geo), default=0)
        return descs, off, hc, wc

    @torch.no_grad()
    def __call__(self, images, targets, params=None):
        images = list(images)
        if targets is None or len(targets) != len(images) or (params is not None and len(params) != len(images)):
            raise ValueError("images, targets and params must be lists of the same length")
        for im in images:
            if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.shape[0] == 0 or im.shape[1] == 0:
                raise ValueError("images must be uint8 tensors of shape (H, W, 3)")
        if params is None:
            params = [self.sample(int(im.shape[1]), int(im.shape[0])) for im in images]
        for im, p in zip(images, params):
            _stages(p, int(im.shape[0]), int(im.shape[1]))            # ValueError before anything is uploaded
        imgs = []
        for im in images:
            im = im.to(self.device)
            if im.stride(2) != 1 or im.stride(1) != 3:
                im = im.contiguous()
            imgs.append(im)
        new_targets = self._targets_to_device([transform_target(t, p, im.shape[:2]) for t, p, im in zip(targets, params, images)])
        b = len(imgs)
        descs, scratch_bytes, hc, wc = self.describe(imgs, params)
        out = torch.empty(b, 3, hc, wc, dtype=self.dtype, device=self.device)
        mask = torch.empty(b, hc, wc, dtype=torch.bool, device=self.device)
        if b == 0:
            return NestedTensor(out, mask), new_targets
        scratch = torch.empty(max(scratch_bytes, 16), dtype=torch.uint8, device=self.device)
        host = bytearray(bytes(descs))
        raw = torch.frombuffer(host, dtype=torch.uint8).to(self.device)                   # descriptor array -> device
        with torch.cuda.device(self.device):
            rc = _nat.lib().lwdetr_augment_normalize(C.addressof(descs), raw.data_ptr(), b, self._tables.buf.data_ptr(), self._tables.buf.numel(),
                                                     scratch.data_ptr(), scratch.numel(), self.lut.data_ptr(), out.data_ptr(), mask.data_ptr(),
                                                     hc, wc, _nat.dtype_code(self.dtype), _nat.stream_ptr(self.device))
        _nat.check(rc, "lwdetr_augment_normalize")
        self._keep = (imgs, scratch, raw, descs)      # alive until the next call (the launches are asynchronous)
        return NestedTensor(out, mask), new_targets

    def _targets_to_device(self, targets):
        """One host-to-device copy per field (and dtype) for the whole batch; the per-image tensors are views of it."""
        out = [dict() for _ in targets]
        for key in sorted({k for t in targets for k in t}):
            by_dtype = {}
            for i, t in enumerate(targets):
                if key in t:
                    by_dtype.setdefault((t[key].dtype, tuple(t[key].shape[1:])), []).append(i)
            for idx in by_dtype.values():
                parts = [targets[i][key] for i in idx]
                dev = torch.cat(parts, 0).to(self.device)
                for i, piece in zip(idx, dev.split([int(p.shape[0]) for p in parts], 0)):
                    out[i][key] = piece
        return out


def make_coco_transforms(image_set, dtype=torch.float16, device="cuda", size=640, **recipe):
    """The reference's aspect-preserving recipe (datasets/coco.py:86-120): 'train' -> TrainTransform(square=False); 'val' / 'val_speed' ->
    the inference transform SquareResizeNormalize(size)."""
    if image_set == "train":
        return TrainTransform(dtype=dtype, device=device, square=False, **recipe)
    if image_set in ("val", "val_speed"):
        return SquareResizeNormalize(size, dtype=dtype, device=device)
    raise ValueError(f"unknown {image_set}")


def make_coco_transforms_square_div_64(image_set, dtype=torch.float16, device="cuda", size=640, **recipe):
    """The reference's default recipe (datasets/coco.py:123-160): 'train' -> TrainTransform(square=True); 'val' / 'val_speed' ->
    SquareResizeNormalize(size)."""
    if image_set == "train":
        transform = TrainTransform(dtype=dtype, device=device, square=True, **recipe)
        transform.prebuild()
        return transform
    if image_set in ("val", "val_speed"):
        return SquareResizeNormalize(size, dtype=dtype, device=device)
    raise ValueError(f"unknown {image_set}")
