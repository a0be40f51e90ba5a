"""Times the native COCO box evaluator (csrc/cocoeval.hip through lwdetr_amd.CocoEvaluator) at COCO val2017 scale on synthetic data, beside
the forward + PostProcess step of the same process:

    python tools/cocoeval_time.py [--images 5000] [--cats 80] [--k 300] [--batch 32] [--size small] [--dtype fp16] [--n 3] [--no-model]
  * synthetic ground truth (about 7 annotations per image, 1.5 % crowds, areas over all three ranges) and detections (K per image: jittered
    copies of the image's ground truths under high scores, random boxes under low ones), seeded;
  * update_packed per batch: HIP events around every call (median, max) and the host clock around the whole loop ending in a synchronise;
  * synchronize_between_processes + accumulate (the two sorts, npig, the curves kernel, the copy of the result arrays): host clock ending in
    the copy;
  * once, the graph replay time of forward + PostProcess at the same batch, times the number of batches.
Every figure is reported --n times (the spread). No host baseline exists in a standalone checkout: absolute times only.
Written for profiles/r9a_cocoeval.txt."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def synth_coco(n_images, n_cats, k, seed=0):
    """(dataset dict, image ids, (n_images, k, 6) f32 records)"""
    rng = np.random.RandomState(seed)
    cat_ids = [c for c in range(1, 10 * n_cats) if c % 9 != 3][:n_cats]         # sparse ids, as COCO's 80 of 1..90
    img_ids = (np.arange(n_images) * 7 + 139).tolist()
    anns, packed = [], np.zeros((n_images, k, 6), np.float32)
    for b, img in enumerate(img_ids):
        n = min(int(rng.poisson(7)), 60)
        side = np.exp(rng.uniform(np.log(8), np.log(400), size=(n, 2)))
        xy = rng.uniform(0, 640 - 8, size=(n, 2))
        wh = np.minimum(side, 640 - xy)
        cats = rng.randint(0, n_cats, size=n)
        for j in range(n):
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": cat_ids[cats[j]], "bbox": [*xy[j].tolist(), *wh[j].tolist()],
                         "area": float(wh[j, 0] * wh[j, 1] * rng.uniform(.4, 1.)), "iscrowd": int(rng.rand() < .015)})
        m = min(3 * n, k)
        src = rng.randint(0, n, size=m) if n else np.zeros(0, int)
        jit = rng.normal(0, .08, size=(m, 4)) * np.tile(wh[src], 2) if n else np.zeros((0, 4))
        packed[b, :m, 2:4] = xy[src] + jit[:, :2] if n else 0
        packed[b, :m, 4:6] = xy[src] + wh[src] + jit[:, 2:] if n else 0
        packed[b, :m, 1] = np.asarray(cat_ids)[cats[src]] if n else 0
        r0 = rng.uniform(0, 600, size=(k - m, 2))
        packed[b, m:, 2:4] = r0
        packed[b, m:, 4:6] = r0 + np.exp(rng.uniform(np.log(4), np.log(300), size=(k - m, 2)))
        packed[b, m:, 1] = np.asarray(cat_ids)[rng.randint(0, n_cats, size=k - m)]
        packed[b, :, 0] = np.sort(np.concatenate([rng.uniform(.2, 1., size=m), rng.uniform(0, .3, size=k - m)]))[::-1]
    ds = {"images": [{"id": i} for i in img_ids], "categories": [{"id": c} for c in cat_ids], "annotations": anns}
    return ds, img_ids, packed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--cats", type=int, default=80)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", default="small")
    ap.add_argument("--res", type=int, default=640)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    import torch
    import lwdetr_amd
    from lwdetr_amd import _native
    assert torch.cuda.is_available(), "cocoeval_time.py measures on a ROCm device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    _native.lib()
    t0 = time.perf_counter()
    ds, img_ids, packed = synth_coco(a.images, a.cats, a.k)
    gt = lwdetr_amd.CocoGroundTruth(ds)
    print(f"synthetic set: {a.images} images, {a.cats} categories, {len(ds['annotations'])} annotations ({len(ds['annotations']) / a.images:.2f} / image, "
          f"largest (image, category) group {gt.max_group}), K = {a.k}; generated and packed on the host in {time.perf_counter() - t0:.2f} s", flush=True)
    recs = torch.from_numpy(packed).to(dev)
    batches = [(img_ids[i:i + a.batch], recs[i:i + a.batch].contiguous()) for i in range(0, a.images, a.batch)]
    gt.tables(dev)
    warm = lwdetr_amd.CocoEvaluator(gt, ("bbox",))                              # warm-up of every shape the timed window uses
    for ids, r in batches[:2] + batches[-1:]:
        warm.update_packed(ids, r)
    warm.accumulate()
    torch.cuda.synchronize(dev)
    stats = None
    for rep in range(a.n):
        ev = lwdetr_amd.CocoEvaluator(gt, ("bbox",))
        marks = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in batches]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for (ids, r), (e0, e1) in zip(batches, marks):
            e0.record()
            ev.update_packed(ids, r)
            e1.record()
        torch.cuda.synchronize(dev)
        t_update = (time.perf_counter() - t0) * 1e3
        per = [e0.elapsed_time(e1) for e0, e1 in marks]
        full = [p for p, (ids, _) in zip(per, batches) if len(ids) == a.batch]
        t0 = time.perf_counter()
        ev.synchronize_between_processes()
        torch.cuda.synchronize(dev)
        t_sync = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ev.accumulate()
        t_acc = (time.perf_counter() - t0) * 1e3
        st = ev.coco_eval["bbox"].stats
        assert stats is None or np.array_equal(stats, st), "two runs differ"
        stats = st
        print(f"run {rep}: update_packed x {len(batches)} batches of {a.batch}: device events per call p50 {median(full):.4f} ms max {max(full):.4f} ms "
              f"sum {sum(per):.2f} ms; host clock over the loop, synchronised {t_update:.2f} ms | synchronize_between_processes (one process: "
              f"compaction + de-duplication) {t_sync:.2f} ms | accumulate (2 sorts, npig, curves, copy of the arrays, stats) {t_acc:.2f} ms | "
              f"kept detections {ev.sorted_store.cat.numel()}", flush=True)
    print("stats " + " ".join(f"{v:.4f}" for v in stats), flush=True)
    ev.summarize()

    if not a.no_model:
        from lwdetr_amd.synth import synth_images, synth_state_dict
        T = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
        model, _, post = lwdetr_amd.build_model(lwdetr_amd.get_args(a.size))
        model.load_state_dict(synth_state_dict(model.state_dict(), seed=0))
        model = model.to(dev).to(T).eval()
        images = synth_images(a.batch, a.res, a.res, seed=1234).to(dev).to(T)
        sizes = torch.tensor([[480.0, 640.0]] * a.batch, device=dev)
        graphed = model.capture(images, postprocess=post["bbox"], target_sizes=sizes)
        lat = []
        for i in range(220):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            graphed(images)
            torch.cuda.synchronize(dev)
            if i >= 20:
                lat.append((time.perf_counter() - t0) * 1e3)
        nb = len(batches)
        print(f"forward + PostProcess {a.size} B={a.batch} {a.res} {a.dtype}, one graph: p50 {median(lat):.4f} ms per batch, x {nb} batches = "
              f"{median(lat) * nb:.1f} ms for {a.images} images", flush=True)


if __name__ == "__main__":
    main()
