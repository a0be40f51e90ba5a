"""Writes tests/golden/augment.npz: what the UNMODIFIED reference's training transforms (datasets/transforms.py, datasets/coco.py) make of
small seeded images and annotation lists, on the CPU (needs the reference checkout and Pillow; torchvision is replaced by the stand-ins of
tests/torchvision_pil_shim.py, so the goldens are the reference transforms over real Pillow through these stand-ins):
    python tools/gen_golden_augment.py
Per case the fixture holds data only: the recipe's numbers, the seed, the input image, the annotation list, the reference's uint8 output
(its Compose without the final ToTensor + Normalize), its ConvertCoco target and its full target dict (the Compose with them). The two
cases at the recipes' real default parameters store a sha256 of the uint8 output and a strided subsample instead, and their input is
tests/augment_ref.synth_image. Once, the reference's ToTensor + Normalize of all 256 values per channel pins the lookup table.

A case is (image size, recipe numbers, annotations, a condition on the outcome); the seed is the first one under which the reference's
Compose - built here from the reference's own classes - meets the condition. The conditions name what each case is there for."""
import hashlib
import os
import random
import sys

import numpy as np
import PIL
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import lwdetr_amd  # noqa: E402,F401
import augment_ref as A  # noqa: E402
import torchvision_pil_shim  # noqa: E402
from lwdetr_amd.augment import sample_train_params  # noqa: E402  (only to read a seed's outcome for the conditions)

T, ref_coco = torchvision_pil_shim.install()
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def ref_compose(square, scales, resize_sizes, crop_range, max_size, normalize):
    """The reference's train recipe (datasets/coco.py:95-107 / :135-147) from its own classes, with the recipe's numbers as arguments."""
    last = (lambda: T.SquareResize(list(scales))) if square else (lambda: T.RandomResize(list(scales), max_size=max_size))
    steps = [T.RandomHorizontalFlip(),
             T.RandomSelect(last(), T.Compose([T.RandomResize(list(resize_sizes)), T.RandomSizeCrop(*crop_range), last()]))]
    if normalize:
        steps.append(T.Compose([T.ToTensor(), T.Normalize(MEAN, STD)]))
    return T.Compose(steps)


def run_reference(image, annotations, image_id, seed, recipe):
    pil = Image.fromarray(image)
    _, converted = ref_coco.ConvertCoco()(pil, {"image_id": image_id, "annotations": annotations})
    random.seed(seed)
    torch.manual_seed(seed)
    out_pil, _ = ref_compose(normalize=False, **recipe)(pil, converted)
    random.seed(seed)
    torch.manual_seed(seed)
    out_t, target = ref_compose(normalize=True, **recipe)(pil, converted)
    out = np.asarray(out_pil)
    assert tuple(out_t.shape[1:]) == out.shape[:2]
    return out, converted, target


def boxes_grid(h, w, crowd=True):
    """A few boxes over the image (COCO xywh, float areas), one past the border, one degenerate, one crowd, one without iscrowd."""
    anns = []
    for k, (fx, fy, fw, fh) in enumerate([(0.02, 0.03, 0.2, 0.25), (0.4, 0.35, 0.3, 0.3), (0.7, 0.6, 0.5, 0.5), (0.1, 0.7, 0.15, 0.2),
                                          (0.8, 0.05, 0.12, 0.3), (0.45, 0.02, 0.1, 0.1)]):
        bw, bh = round(fw * w, 2), round(fh * h, 2)
        obj = {"bbox": [round(fx * w, 2), round(fy * h, 2), bw, bh], "category_id": 1 + 7 * k, "area": round(bw * bh * 0.8, 3), "iscrowd": 0}
        if k == 3:
            del obj["iscrowd"]
        anns.append(obj)
    anns.append({"bbox": [5.0, 5.0, 0.0, 4.0], "category_id": 3, "area": 0.0, "iscrowd": 0})            # no width: ConvertCoco drops it
    if crowd:
        anns.append({"bbox": [1.0, 1.0, 10.0, 10.0], "category_id": 5, "area": 100.0, "iscrowd": 1})
    return anns


SMALL = dict(square=True, scales=(48, 56, 64, 72, 80, 88, 96), resize_sizes=(40, 50, 60), crop_range=(38, 60), max_size=None)


def small(**kw):
    return dict(SMALL, **kw)


def b1(p):
    return p.resize1 is None


def b2(p):
    return p.resize1 is not None


# (name, (H, W), recipe, annotations, condition(params, source (h, w), n boxes in, n boxes out[, n boxes clipped to zero width]))
CASES = [
    ("flip_odd_width_branch1", (50, 63), small(), "grid", lambda p, s, ni, no: b1(p) and p.flip),
    ("noflip_odd_width_branch1", (50, 63), small(), "grid", lambda p, s, ni, no: b1(p) and not p.flip),
    ("branch2_stage1_upscale", (30, 41), small(), "grid", lambda p, s, ni, no: b2(p) and p.resize1[0] > s[0] and p.flip),
    ("branch2_stage1_downscale_3x", (131, 150), small(resize_sizes=(40,)), "grid", lambda p, s, ni, no: b2(p) and not p.flip),
    ("branch2_stage1_identity_left_odd", (50, 67), small(resize_sizes=(50,)), "grid",
     lambda p, s, ni, no: b2(p) and p.resize1 == s and p.crop[1] % 4 in (1, 3) and p.crop[0] > 0),
    ("branch2_stage1_identity_flip", (50, 67), small(resize_sizes=(50,)), "grid",
     lambda p, s, ni, no: b2(p) and p.resize1 == s and p.flip and p.crop[1] % 4 == 2),
    ("crop_at_origin", (60, 75), small(), "grid", lambda p, s, ni, no: b2(p) and p.crop[:2] == (0, 0) and p.crop[2:] != p.resize1),
    ("crop_at_far_corner", (60, 75), small(), "grid",
     lambda p, s, ni, no: b2(p) and p.crop[0] == p.resize1[0] - p.crop[2] > 0 and p.crop[1] == p.resize1[1] - p.crop[3] > 0),
    ("crop_is_full_image_no_randint", (45, 58), small(resize_sizes=(40,), crop_range=(40, 60)), "grid",
     lambda p, s, ni, no: b2(p) and p.crop == (0, 0) + p.resize1),
    ("cw_equals_ow_flip", (70, 90), small(scales=(48,)), "grid",
     lambda p, s, ni, no: b2(p) and p.flip and p.crop[3] == 48 and p.crop[2] != 48),
    ("ch_equals_oh", (70, 90), small(scales=(48,)), "grid", lambda p, s, ni, no: b2(p) and p.crop[2] == 48 and p.crop[3] != 48),
    ("stage2_nothing_to_do", (70, 90), small(scales=(48,), resize_sizes=(50, 60), crop_range=(48, 48)), "grid", lambda p, s, ni, no: b2(p) and p.flip),
    ("branch1_width_equals_scale_flip", (51, 64), small(scales=(64,)), "grid", lambda p, s, ni, no: b1(p) and p.flip),
    ("branch1_height_equals_scale", (64, 51), small(scales=(64,)), "none", lambda p, s, ni, no: b1(p) and not p.flip),
    ("residues_cw0_ow1", (66, 81), small(scales=(61,)), "grid", lambda p, s, ni, no: b2(p) and p.crop[3] % 4 == 0),
    ("residues_cw1_ow2", (66, 81), small(scales=(62,)), "grid", lambda p, s, ni, no: b2(p) and p.crop[3] % 4 == 1 and p.flip),
    ("residues_cw2_ow3", (66, 81), small(scales=(63,)), "grid", lambda p, s, ni, no: b2(p) and p.crop[3] % 4 == 2),
    ("residues_cw3_ow0", (66, 81), small(scales=(64,)), "grid", lambda p, s, ni, no: b2(p) and p.crop[3] % 4 == 3 and p.flip),
    ("crop_removes_all_boxes", (80, 100), small(), "corner", lambda p, s, ni, no: b2(p) and ni > 0 and no == 0),
    ("crop_clips_a_box_to_zero_width", (80, 100), small(), "grid", lambda p, s, ni, no, zw=1: b2(p) and 0 < no < ni and zw > 0),
    ("no_annotations", (57, 49), small(), "none", lambda p, s, ni, no: b2(p)),
    ("aspect_branch1_max_size_binds", (40, 121), small(square=False, scales=(64,), max_size=80), "grid", lambda p, s, ni, no: b1(p)),
    ("aspect_branch2_flip", (90, 61), small(square=False, scales=(48, 64, 72), max_size=100), "grid", lambda p, s, ni, no: b2(p) and p.flip),
]
DEFAULTS = [
    ("default_square_branch2", (480, 640), dict(square=True, scales=(448, 512, 576, 640, 704, 768, 832, 896), resize_sizes=(400, 500, 600),
                                                crop_range=(384, 600), max_size=None), "grid", lambda p, s, ni, no: b2(p) and p.flip),
    ("default_aspect_branch2", (427, 640), dict(square=False, scales=(480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800),
                                                resize_sizes=(400, 500, 600), crop_range=(384, 600), max_size=1333), "grid",
     lambda p, s, ni, no: b2(p) and not p.flip),
]


def annotations_for(kind, h, w):
    if kind == "none":
        return []
    if kind == "corner":             # one small box in a corner: most crops leave nothing of it
        return [{"bbox": [0.5, 0.5, 3.0, 2.5], "category_id": 17, "area": 6.1, "iscrowd": 0}]
    return boxes_grid(h, w)


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    specs = [(c, False) for c in CASES] + [(c, True) for c in DEFAULTS]
    for i, ((name, (h, w), recipe, kind, cond), big) in enumerate(specs):
        image = A.synth_image(h, w, 100 + i)
        anns = annotations_for(kind, h, w)
        for seed in range(20000):
            random.seed(seed)
            torch.manual_seed(seed)
            p = sample_train_params(w, h, **recipe)
            if not cond(p, (h, w), 1, 0) and not cond(p, (h, w), 2, 1) and not cond(p, (h, w), 1, 1):
                continue                     # the geometry already rules this seed out
            pix, converted, target = run_reference(image, anns, 1000 + i, seed, recipe)
            assert pix.shape[:2] == tuple(p.out_size), (name, seed, pix.shape, p)
            extra = (A.clipped_to_zero_width(converted["boxes"], p, (h, w)),) if name == "crop_clips_a_box_to_zero_width" else ()
            if cond(p, (h, w), int(converted["boxes"].shape[0]), int(target["boxes"].shape[0]), *extra):
                break
        else:
            raise RuntimeError(f"no seed meets the condition of case {name}")
        pre = f"c{i}_"
        out[pre + "name"], out[pre + "seed"], out[pre + "image_id"] = np.array(name), np.array(seed), np.array(1000 + i)
        out[pre + "square"] = np.array(recipe["square"])
        out[pre + "scales"] = np.array(recipe["scales"], np.int64)
        out[pre + "resize_sizes"] = np.array(recipe["resize_sizes"], np.int64)
        out[pre + "crop_range"] = np.array(recipe["crop_range"], np.int64)
        out[pre + "max_size"] = np.array(recipe["max_size"] or 0)
        if big:
            out[pre + "image_synth"] = np.array([h, w, 100 + i])
        else:
            out[pre + "image"], out[pre + "out"] = image, pix
        out[pre + "ann_bbox"] = np.array([a["bbox"] for a in anns], np.float64).reshape(-1, 4)
        out[pre + "ann_category"] = np.array([a["category_id"] for a in anns], np.int64)
        out[pre + "ann_area"] = np.array([a["area"] for a in anns], np.float64)
        out[pre + "ann_iscrowd"] = np.array([a.get("iscrowd", -1) for a in anns], np.int64)
        out[pre + "out_shape"] = np.array(pix.shape[:2])
        out[pre + "out_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(pix).tobytes()).hexdigest())
        out[pre + "out_sub"] = np.ascontiguousarray(pix[::A.SUB[0], ::A.SUB[1]])
        for k in A.TARGET_KEYS:
            out[pre + "cv_" + k] = converted[k].numpy()
            out[pre + "tg_" + k] = target[k].numpy()
        print(f"{i:2d} {name:36s} seed {seed:5d} {p} boxes {converted['boxes'].shape[0]} -> {target['boxes'].shape[0]}")
    out["num_cases"] = np.array(len(specs))
    # the lookup table: the reference's ToTensor + Normalize of every byte value in every channel
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    lut, _ = T.Compose([T.ToTensor(), T.Normalize(MEAN, STD)])(Image.fromarray(ramp), None)
    out["lut"] = lut.reshape(3, 256).numpy()
    path = os.path.join(ROOT, "tests", "golden", "augment.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
