"""Time of the training-time input transform (measurement tool): a batch of 32 COCO-like uint8 images (about 640 x 480, mixed orientations)
through the default square recipe (lwdetr_amd.augment.make_coco_transforms_square_div_64('train')) with sampled parameters, fp16 output.
Beside it, on the same images and the same machine: the same transform through Pillow + torch on ONE host core (the operations the
reference's dataloader workers run per image, then the collate's padding), and the inference transform SquareResizeNormalize(640).

    python tools/augment_time.py [--out FILE] [--sets 8] [--reps 5]

The first figure cycles `sets` fixed, seeded parameter draws (each run once as warm-up), so every coefficient table is cached: it is the
floor of a call, not what training sees. The "fresh draws" figures sample new parameters inside every timed call, as training does, with the
factory's prebuilt stage-2 tables and without them, and count the tables built inside the timed calls. Every figure is a host clock around
one call that ends in a device synchronise, reported as the median; the call includes the host work of the transform (box arithmetic,
descriptors, table and target uploads). Algorithmic bytes are computed from the shapes of the passes each image needs."""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lwdetr_amd.augment import convert_coco, make_coco_transforms_square_div_64  # noqa: E402
from lwdetr_amd.preprocess import IMAGENET_MEAN, IMAGENET_STD, SquareResizeNormalize  # noqa: E402

SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (375, 500), (500, 375), (480, 640), (426, 640)]


def pillow_batch(arrays, params, dtype):
    """The reference's per-image work over Pillow (hflip, resize, crop, resize, ToTensor, Normalize) and the collate's padding."""
    mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
    outs = []
    for a, p in zip(arrays, params):
        img = Image.fromarray(a)
        if p.flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        if p.resize1 is not None:
            img = img.resize((p.resize1[1], p.resize1[0]), Image.BILINEAR)
            top, left, ch, cw = p.crop
            img = img.crop((left, top, left + cw, top + ch))
        img = img.resize((p.out_size[1], p.out_size[0]), Image.BILINEAR)
        t = torch.from_numpy(np.array(img, np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        outs.append(t.sub_(mean).div_(std))
    hc, wc = max(t.shape[1] for t in outs), max(t.shape[2] for t in outs)
    batch = torch.zeros(len(outs), 3, hc, wc)
    mask = torch.ones(len(outs), hc, wc, dtype=torch.bool)
    for t, b, m in zip(outs, batch, mask):
        b[:, :t.shape[1], :t.shape[2]].copy_(t)
        m[:t.shape[1], :t.shape[2]] = False
    return batch.to(dtype), mask


def traffic(descs, n, hc, wc, elt):
    """Algorithmic bytes of one batch: what each needed pass reads and writes once (taps overlap in cache), + the full canvas and mask."""
    total = 0
    for d in list(descs)[:n]:
        h1p, v1p, h2p, v2p = d.w1 != d.width, d.h1 != d.height, d.ow != d.cw, d.oh != d.ch
        rows = d.rows if v1p else d.ch
        if h1p:
            total += 3 * rows * d.width + 3 * rows * d.cw
        if v1p:
            total += 3 * rows * d.cw + 3 * d.ch * d.cw
        if h2p:
            total += 3 * d.ch * d.cw + 3 * d.ch * d.ow
        total += 3 * d.ch * d.ow
    return total + n * hc * wc * (3 * elt + 1)


def timed(fn, sets, reps):
    for s in range(sets):
        fn(s)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        for s in range(sets):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(s)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--fresh", type=int, default=80)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_time.py needs a ROCm device: a time taken elsewhere says nothing")
    dev, dtype, b = torch.device("cuda:0"), torch.float16, args.batch
    gen = torch.Generator().manual_seed(0)
    host = [torch.randint(0, 256, SIZES[i % len(SIZES)] + (3,), dtype=torch.uint8, generator=gen) for i in range(b)]
    frames = [h.to(dev) for h in host]
    arrays = [h.numpy() for h in host]
    targets = [convert_coco([{"bbox": [10.0 + k, 20.0, 100.0, 80.0 + k], "category_id": 1 + k, "area": 4000.0, "iscrowd": 0} for k in range(7)],
                            h.shape[1], h.shape[0], i) for i, h in enumerate(host)]
    tf = make_coco_transforms_square_div_64("train", dtype=dtype, device=dev)
    random.seed(0)
    torch.manual_seed(0)
    psets = [[tf.sample(h.shape[1], h.shape[0]) for h in host] for _ in range(args.sets)]
    sq = SquareResizeNormalize(640, dtype=dtype, device=dev)
    lines = [f"augment_time: batch {b}, sizes {sorted(set(SIZES))}, default square recipe, fp16, {args.sets} parameter sets x {args.reps} timed calls each",
             f"device: {torch.cuda.get_device_name(0)}; host cores visible to this process: {len(os.sched_getaffinity(0))} (OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})"]
    gpu = timed(lambda s: tf(frames, targets, psets[s]), args.sets, args.reps)
    byts = []
    for ps in psets:
        descs, _, hc, wc = tf.describe(frames, ps)
        byts.append(traffic(descs, b, hc, wc, 2))
    mb = statistics.median(byts) / 1e6
    lines.append(f"TrainTransform (4-pass HIP, device-resident inputs), {args.sets} FIXED parameter sets cycled - every table cached: median {gpu[0]:.3f} ms / batch (min {gpu[1]:.3f}, max {gpu[2]:.3f}) = "
                 f"{b / gpu[0] * 1e3:.0f} img/s; algorithmic bytes median {mb:.1f} MB / batch -> {mb / gpu[0]:.1f} GB/s over the whole call")
    # fresh draws, as training makes them: every call samples its own parameters, so every call meets length pairs it has not seen. With the
    # factory's transform the square recipe's stage-2 tables were built once at construction (prebuild) and only stage-1 pairs (image
    # side -> resized side) are built inside calls, until the dataset's sides have been met; without prebuild every new pair is built in a call.
    from lwdetr_amd.augment import TrainTransform
    for label, make in (("factory transform (stage-2 tables prebuilt)", lambda: make_coco_transforms_square_div_64("train", dtype=dtype, device=dev)),
                        ("TrainTransform without prebuild", lambda: TrainTransform(dtype=dtype, device=dev))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fresh = make()
        torch.cuda.synchronize()
        t_make = (time.perf_counter() - t0) * 1e3
        n_pre = len(fresh._tables.entries)
        random.seed(1)
        torch.manual_seed(1)
        fresh(frames, targets)                                   # code objects and allocator only; its draws are not repeated below
        ts, built = [], []
        for _ in range(args.fresh):
            before = len(fresh._tables.entries)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fresh(frames, targets)                               # params=None: drawn inside the call
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            built.append(len(fresh._tables.entries) - before)
        q = max(args.fresh // 4, 1)
        lines.append(f"fresh draws every call, {label}: construction {t_make:.0f} ms ({n_pre} tables, {fresh._tables.length * 4 / 1e6:.1f} MB after the run); "
                     f"{args.fresh} calls: median {statistics.median(ts):.3f} ms / batch (min {min(ts):.3f}, max {max(ts):.3f}); first {q} calls median "
                     f"{statistics.median(ts[:q]):.3f} ms with {statistics.mean(built[:q]):.1f} tables built per call, last {q} calls median "
                     f"{statistics.median(ts[-q:]):.3f} ms with {statistics.mean(built[-q:]):.1f}")
    # where the call's time goes: the four launches alone (device events around 20 enqueues of one prepared batch, per parameter set),
    # and the host's box arithmetic + target upload alone
    from lwdetr_amd import _native
    from lwdetr_amd.augment import transform_target
    import ctypes
    kern = []
    for ps in psets:
        descs, sbytes, hc, wc = tf.describe(frames, ps)
        scratch = torch.empty(max(sbytes, 16), dtype=torch.uint8, device=dev)
        raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
        out = torch.empty(b, 3, hc, wc, dtype=dtype, device=dev)
        mask = torch.empty(b, hc, wc, dtype=torch.bool, device=dev)
        call = lambda: _native.check(_native.lib().lwdetr_augment_normalize(
            ctypes.addressof(descs), raw.data_ptr(), b, tf._tables.buf.data_ptr(), tf._tables.buf.numel(), scratch.data_ptr(), scratch.numel(),
            tf.lut.data_ptr(), out.data_ptr(), mask.data_ptr(), hc, wc, _native.dtype_code(dtype), _native.stream_ptr(dev)), "lwdetr_augment_normalize")
        call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            call()
        e1.record()
        torch.cuda.synchronize()
        kern.append(e0.elapsed_time(e1) / 20)
    km = statistics.median(kern)
    lines.append(f"  of which the launches alone (device events, 20 enqueues of a prepared batch): median {km:.3f} ms / batch (min {min(kern):.3f}, max "
                 f"{max(kern):.3f}) -> {mb / km:.1f} GB/s algorithmic ({mb / km / 8000:.1%} of 8 TB/s)")
    hs = []
    for _ in range(args.reps):
        for ps in psets:
            t0 = time.perf_counter()
            tf._targets_to_device([transform_target(t, p, h.shape[:2]) for t, p, h in zip(targets, ps, host)])
            torch.cuda.synchronize()
            hs.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"  of which the host's box arithmetic for 32 targets (7 boxes each) + their upload: median {statistics.median(hs):.3f} ms / batch")
    inf = timed(lambda s: sq(frames), args.sets, args.reps)
    mb_inf = sum(3 * h.shape[0] * h.shape[1] + (0 if h.shape[1] == 640 else 6 * h.shape[0] * 640) + 3 * 640 * 640 * 2 for h in host) / 1e6
    lines.append(f"SquareResizeNormalize(640) (2-pass HIP, same images): median {inf[0]:.3f} ms / batch (min {inf[1]:.3f}, max {inf[2]:.3f}); "
                 f"algorithmic bytes {mb_inf:.1f} MB / batch -> {mb_inf / inf[0]:.1f} GB/s over the whole call")
    lines.append(f"ratio TrainTransform / SquareResizeNormalize: time {gpu[0] / inf[0]:.2f}x, bytes {mb / mb_inf:.2f}x")
    torch.set_num_threads(1)
    cpu = []
    for _ in range(2):
        for s in range(min(args.sets, 4)):
            t0 = time.perf_counter()
            ref = pillow_batch(arrays, psets[s], dtype)
            cpu.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"Pillow {Image.__version__} + torch on ONE host core (torch.set_num_threads(1); {len(os.sched_getaffinity(0))} visible), same images and parameters: median "
                 f"{statistics.median(cpu):.1f} ms / batch (min {min(cpu):.1f}, max {max(cpu):.1f}) = {statistics.median(cpu) / gpu[0]:.0f}x the HIP call")
    nt, _ = tf(frames, targets, psets[min(args.sets, 4) - 1])
    same = torch.equal(nt.tensors.cpu(), ref[0]) and torch.equal(nt.mask.cpu(), ref[1])
    lines.append(f"last Pillow batch equals the HIP batch bit for bit: {same}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
