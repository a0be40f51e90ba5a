"""Forward + backward time and peak memory of one training step's model part (4 images of 640 x 640, group_detr = 13), two ways on one device
in one process and one build: ``differentiable_forward(fused=None)`` (the fused attention, LayerNorm2d, two-stage, sine-embed and deformable
attention operators) and ``differentiable_forward(fused=False)`` (the same assembly with every one of them in its torch formulation). Sizes:
small and large, in f32 and under bf16 autocast.
    python tools/train_model_time.py [--reps 10] [--warmup 3] [--sizes small,large] > profiles/r17a_train_model.txt
The two ways are interleaved round by round (one forward + backward each per round, device events around it); the table gives the median and
the minimum in milliseconds, and the peak of torch.cuda.max_memory_allocated() over one forward + backward above what the parameters, their
gradients and the images hold. The loss is the sum of every output tensor times a fixed random cotangent."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lwdetr_amd  # noqa: E402
from lwdetr_amd.models.train_forward import differentiable_forward  # noqa: E402
from lwdetr_amd.synth import synth_images, synth_state_dict  # noqa: E402


def flat(out):
    t = [out["pred_logits"], out["pred_boxes"], out["enc_outputs"]["pred_logits"], out["enc_outputs"]["pred_boxes"]]
    for a in out["aux_outputs"]:
        t += [a["pred_logits"], a["pred_boxes"]]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="small,large")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--res", type=int, default=640)
    a = ap.parse_args()
    dev = torch.device("cuda")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {a.batch} images of {a.res} x {a.res}, group_detr = 13; model forward + "
          f"backward, {a.reps} interleaved rounds after {a.warmup} warm-up rounds")
    print("# size   compute | ms median (min): fused=None | fused=False || peak MiB above parameters, gradients and images: fused=None | fused=False")
    for size in a.sizes.split(","):
        args = lwdetr_amd.get_args(size)
        model, _, _ = lwdetr_amd.build_model(args)
        model.load_state_dict(synth_state_dict(model.state_dict(), seed=0))
        model = model.to(dev).train()
        images = synth_images(a.batch, a.res, a.res, seed=7).to(dev)
        cots = None
        for autocast in (False, True):
            def one(fused):
                with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
                    out = flat(differentiable_forward(model, images, fused=fused))
                nonlocal cots
                if cots is None or cots[0].dtype != out[0].dtype:
                    g = torch.Generator(device=dev).manual_seed(1)
                    cots = [torch.randn(t.shape, generator=g, device=dev, dtype=torch.float32).to(t.dtype) for t in out]
                torch.autograd.backward(out, cots)

            ways = [("fused", None), ("torch", False)]
            times, peaks = {n: [] for n, _ in ways}, {}
            for n, fused in ways:
                one(fused)                                                  # first call: allocator pools, library algorithm choice, gradients allocated
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                one(fused)
                torch.cuda.synchronize()
                peaks[n] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            for r in range(a.warmup + a.reps):
                for n, fused in ways:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    one(fused)
                    e1.record()
                    e1.synchronize()
                    if r >= a.warmup:
                        times[n].append(e0.elapsed_time(e1))
            cell = lambda n: f"{statistics.median(times[n]):8.2f} ({min(times[n]):8.2f})"
            print(f"{size:>6} {'bf16 autocast' if autocast else 'f32':>13} | {cell('fused')} | {cell('torch')} || {peaks['fused']:9.1f} | {peaks['torch']:9.1f}",
                  flush=True)
        del model, images


if __name__ == "__main__":
    main()
