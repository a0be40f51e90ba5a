"""Inputs shared by tests/test_cocoeval_host.py and tests/test_gpu_cocoeval.py: the hand-derived cases and the seeded generated set.
No test in here; the expected numbers of the hand-derived cases are literals in the tests themselves."""
import numpy as np

SEED = 20240917
CAT_IDS = [1, 3, 7, 8, 90]            # sparse ids; 7 has ground truths and no detections, 8 detections and no ground truth at all
IMG_IDS = [11, 5, 42, 7, 19, 23, 3, 99]      # 99 is in the ground truth and never updated; 3 takes the 130 same-category detections
K = 40
K_BIG = 130
AP1 = 1.0 / (1.0 + 2.220446049250313e-16)     # precision of "one true positive, no false positive": tp / (fp + tp + eps) = 0.9999999999999998


def ann(ann_id, image_id, cat, box, area=None, iscrowd=0, **extra):
    d = {"id": ann_id, "image_id": image_id, "category_id": cat, "bbox": [float(v) for v in box],
         "area": float(box[2] * box[3] if area is None else area), "iscrowd": iscrowd}
    d.update(extra)
    return d


def dataset(images, cats, anns):
    return {"images": [{"id": i} for i in images], "categories": [{"id": c} for c in cats], "annotations": anns}


def pack(dets, k=None):
    """[(score, label, x0, y0, x1, y1), ...] per image -> (B, k, 6) f32, padded with label -1 (no category)."""
    k = max(len(d) for d in dets) if k is None else k
    out = np.zeros((len(dets), k, 6), dtype=np.float32)
    out[:, :, 1] = -1
    for b, d in enumerate(dets):
        if len(d):
            out[b, :len(d)] = np.asarray(d, dtype=np.float32)
    return out


# --------------------------------------------------------------------------------------------------------------- hand-derived cases
def hand_cases():
    """name -> (dataset, image ids, packed detections). The derivations and the expected numbers are in the tests."""
    cases = {}
    ds = dataset([1], [1, 2], [ann(1, 1, 1, [10, 10, 20, 20]), ann(2, 1, 2, [50, 50, 50, 50])])
    cases["perfect"] = (ds, [1], pack([[(.9, 1, 10, 10, 30, 30), (.8, 2, 50, 50, 100, 100)]]))
    ds = dataset([1], [1], [ann(1, 1, 1, [0, 0, 10, 20])])
    cases["second_is_tp_at_50"] = (ds, [1], pack([[(.9, 1, 100, 100, 110, 110), (.8, 1, 0, 0, 10, 10)]]))
    ds = dataset([1], [1], [ann(1, 1, 1, [0, 0, 100, 100], iscrowd=1), ann(2, 1, 1, [200, 200, 50, 50])])
    cases["crowd_absorbs_three"] = (ds, [1], pack([[(.9, 1, 10, 10, 30, 30), (.8, 1, 40, 40, 60, 60), (.7, 1, 50, 50, 90, 90),
                                                    (.6, 1, 200, 200, 250, 250)]]))
    ds = dataset([1], [1], [ann(1, 1, 1, [0, 0, 32, 32])])
    cases["area_1024"] = (ds, [1], pack([[(.9, 1, 0, 0, 32, 32)]]))
    return cases


# --------------------------------------------------------------------------------------------------------------- generated set
def _traps(image_id, next_id):
    """Ground truths and detections that put the listed traps into one image (category 1 / 3 / 90), integer coordinates so that the
    IoUs in question are exact."""
    a, d = [], []
    nid = lambda: next_id.append(0) or (1000 * image_id + len(next_id))
    # an IoU exactly equal to a threshold: [100,100,10,10] against [100,100,10,20] = 100 / 200 = 0.5
    a.append(ann(nid(), image_id, 1, [100, 100, 10, 20]))
    d.append((.75, 1, 100, 100, 110, 110))
    # two gts with equal IoU (100 / 140) to one detection: the later gt takes it, a second identical detection the earlier one
    a.append(ann(nid(), image_id, 3, [200, 200, 12, 10]))
    a.append(ann(nid(), image_id, 3, [204, 200, 12, 10]))
    d.append((.75, 3, 202, 200, 214, 210))
    d.append((.5, 3, 202, 200, 214, 210))
    # a non-ignored match followed by an ignored (crowd) gt that overlaps the same detection: the break
    a.append(ann(nid(), image_id, 90, [300, 300, 40, 40]))
    a.append(ann(nid(), image_id, 90, [290, 290, 80, 80], iscrowd=1))
    d.append((.875, 90, 300, 300, 340, 340))
    d.append((.25, 90, 310, 310, 360, 360))                    # only the crowd is left for this one
    # area exactly 1024; the 'ignore' key has no effect
    a.append(ann(nid(), image_id, 1, [400, 100, 32, 32], ignore=1))
    d.append((.625, 1, 400, 100, 432, 132))
    # zero-area and inverted boxes
    d.append((.5, 1, 50, 50, 50, 60))
    d.append((.5, 1, 70, 70, 60, 60))
    d.append((.375, 3, 205, 205, 205, 205))
    # labels outside the category list
    d.append((.9, 2, 100, 100, 110, 120))
    d.append((.9, 1000, 100, 100, 110, 120))
    d.append((.9, -1, 100, 100, 110, 120))
    d.append((.9, 50, 100, 100, 110, 120))
    return a, d


def generated():
    """Returns dict(dataset, batches=[(image ids, packed)], evaluated=[(image ids, packed)] without the duplicate update)."""
    rng = np.random.RandomState(SEED)
    anns, counter = [], []
    per_image = {}
    for n, img in enumerate(IMG_IDS):
        a, d = (_traps(img, counter) if n in (0, 3) else ([], []))
        for _ in range(rng.randint(3, 9)):                     # random ground truths of all sizes, some crowds
            cat = [1, 3, 90, 7][rng.randint(4)]
            side = [12, 30, 60, 150][rng.randint(4)]
            x, y = rng.randint(0, 500, size=2) + 500
            w, h = side + rng.randint(0, 8), side + rng.randint(0, 8)
            a.append(ann(1000 * img + 500 + len(a), img, cat, [x, y, w, h], iscrowd=int(rng.rand() < .15)))
        if n == 6:                                              # 130 detections of one category over a handful of gts
            for j in range(K_BIG):
                g = a[rng.randint(len(a))]["bbox"]
                jit = rng.randint(-6, 7, size=4)
                d.append((rng.randint(1, 16) / 16., 1, g[0] + jit[0], g[1] + jit[1], g[0] + g[2] + jit[2], g[1] + g[3] + jit[3]))
            a = [dict(x, category_id=1) if x["category_id"] == 3 else x for x in a]
        else:
            while len(d) < K:
                cat = [1, 3, 90, 8][rng.randint(4)]
                score = rng.randint(1, 16) / 16.                # many equal scores, inside an image and across images
                if rng.rand() < .6 and a:
                    g = a[rng.randint(len(a))]["bbox"]
                    jit = rng.randint(-5, 6, size=4)
                    d.append((score, cat, g[0] + jit[0], g[1] + jit[1], g[0] + g[2] + jit[2], g[1] + g[3] + jit[3]))
                else:
                    x, y = rng.randint(0, 900, size=2)
                    d.append((score, cat, x, y, x + rng.randint(1, 200), y + rng.randint(1, 200)))
        anns.extend(a)
        per_image[img] = d
    ds = dataset(IMG_IDS, CAT_IDS, anns)
    first = [IMG_IDS[0], IMG_IDS[1], IMG_IDS[2]]
    second = [IMG_IDS[3], IMG_IDS[4], IMG_IDS[5]]
    big = [IMG_IDS[6]]
    dup = [IMG_IDS[1]]                                          # a second update of image 5 with other detections: the first one wins
    evaluated = [(first, pack([per_image[i] for i in first], K)), (second, pack([per_image[i] for i in second], K)),
                 (big, pack([per_image[i] for i in big], K_BIG))]
    batches = evaluated + [(dup, pack([per_image[IMG_IDS[2]]], K))]
    return {"dataset": ds, "batches": batches, "evaluated": evaluated}


def oracle_run(ref_module, ds, batches):
    """The oracle over ``batches`` [(image ids, packed)]: returns (CocoEvalRef after accumulate + summarize, per-slot table)."""
    ref = ref_module.CocoEvalRef(ds)
    results, ids = [], []
    for image_ids, packed in batches:
        results.extend(ref_module.results_from_packed(image_ids, packed))
        ids.extend(image_ids)
    ref.evaluate(results, ids)
    ref.accumulate()
    ref.summarize()
    return ref, ref.detection_table(len(results))


def carry_set(n_images=40, per_image=75, seed=7):
    """One category, n_images x per_image (= 3 000) detections: the curves kernel's chunk carry."""
    rng = np.random.RandomState(seed)
    imgs = list(range(1, n_images + 1))
    anns, dets = [], []
    for i in imgs:
        gts = []
        for j in range(6):
            x, y = rng.randint(0, 600, size=2)
            w, h = rng.randint(10, 120, size=2)
            gts.append([x, y, w, h])
            anns.append(ann(100 * i + j, i, 1, [x, y, w, h], iscrowd=int(j == 5)))
        d = []
        for j in range(per_image):
            g = gts[rng.randint(6)]
            jit = rng.randint(-8, 9, size=4)
            d.append((rng.randint(1, 1000) / 1000., 1, g[0] + jit[0], g[1] + jit[1], g[0] + g[2] + jit[2], g[1] + g[3] + jit[3]))
        dets.append(d)
    return dataset(imgs, [1], anns), imgs, pack(dets, per_image)
