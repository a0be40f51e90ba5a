"""Forward + backward time and peak memory of the deformable cross-attention core of a 4-image training step - from the outputs of the
sampling_offsets / attention_weights / value_proj Linears to the core's output and back - two ways on one device in one process:
FusedMSDeformAttnFunction (csrc/msda_train.hip) and the path there was before it, the reference's location / softmax arithmetic in torch +
MSDeformAttnFunction (float32 only: that operator has no 16-bit backward). Shapes: B = 4 at the small model's training shape (3900 queries,
16 heads x 16, one 40 x 40 level, 2 points) and at the large model's (24 heads x 16, 80 x 80 + 20 x 20, 4 points), f32 and bf16.
    python tools/msda_train_time.py [--reps 30] [--warmup 5] > profiles/r14a_msda_train.txt
The two are interleaved round by round (one forward + backward each per round, timed with events); the table gives medians and minima in
microseconds, the fused forward alone, and the peak of torch.cuda.max_memory_allocated() over one forward + backward above what the inputs
hold (the fused path's backward workspace, 20 bytes per sample and kept between calls, is part of its peak)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lwdetr_amd.ops import FusedMSDeformAttnFunction  # noqa: E402
from lwdetr_amd.ops import deform_train  # noqa: E402

SHAPES = [("small", 4, 3900, 16, 16, [(40, 40)], 2), ("large", 4, 3900, 24, 16, [(80, 80), (20, 20)], 4)]


def fused(value, shapes, lsi, off, lg, ref, P):
    return FusedMSDeformAttnFunction.apply(value, shapes, lsi, off, lg, ref)


def torch_path(value, shapes, lsi, off, lg, ref, P):
    return deform_train.torch_formulation(value, shapes, lsi, off, lg, ref, None, P)


def one(fn, ops, t, backward=True):
    for x in ops["leaves"]:
        x.grad = None
    out = fn(ops["value"], ops["shapes"], ops["lsi"], ops["off"], ops["lg"], ops["ref"], ops["P"])
    if backward:
        out.backward(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; forward + backward, {a.reps} interleaved rounds after {a.warmup} warm-up rounds")
    print("# dtype  model     Q   M   D  L  P | us median (min): fused fwd+bwd | fused fwd alone | torch + MSDeformAttnFunction fwd+bwd || peak MiB above inputs: fused | torch")
    for dtype in (torch.float32, torch.bfloat16):
        for name, B, Q, M, D, levels, P in SHAPES:
            torch.manual_seed(0)
            L, S = len(levels), sum(h * w for h, w in levels)
            shapes = torch.tensor(levels, dtype=torch.int64, device=dev)
            lsi = torch.cat((shapes.new_zeros(1), (shapes[:, 0] * shapes[:, 1]).cumsum(0)[:-1]))
            value = torch.randn(B, S, M, D, device=dev, dtype=dtype, requires_grad=True)
            off = (torch.randn(B, Q, M * L * P * 2, device=dev) * P).to(dtype).requires_grad_(True)
            lg = torch.randn(B, Q, M * L * P, device=dev, dtype=dtype, requires_grad=True)
            ref = torch.cat((torch.rand(B, Q, 1, 2, device=dev), torch.rand(B, Q, 1, 2, device=dev) * 0.3 + 0.05), -1).expand(B, Q, L, 4).contiguous()
            ref.requires_grad_(True)
            t = torch.randn(B, Q, M * D, device=dev, dtype=dtype)
            ops = dict(value=value, shapes=shapes, lsi=lsi, off=off, lg=lg, ref=ref, P=P, leaves=[value, off, lg, ref])
            ways = [("fused", fused, True), ("fused_fwd", fused, False)] + ([("torch", torch_path, True)] if dtype == torch.float32 else [])
            times, peaks = {n: [] for n, _, _ in ways}, {}
            for n, fn, bwd in ways:
                if not bwd:
                    continue
                one(fn, ops, t)                                         # first call: allocator pools and the cached workspace
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                one(fn, ops, t)
                torch.cuda.synchronize()
                peaks[n] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            ws = sum(w.numel() * 4 for w in deform_train._WORKSPACES.values()) / 2 ** 20
            for r in range(a.warmup + a.reps):
                for n, fn, bwd in ways:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if bwd:
                        one(fn, ops, t)
                    else:
                        with torch.no_grad():
                            one(fn, ops, t, backward=False)
                    e1.record()
                    e1.synchronize()
                    if r >= a.warmup:
                        times[n].append(e0.elapsed_time(e1) * 1e3)
            cell = lambda n: f"{statistics.median(times[n]):9.1f} ({min(times[n]):9.1f})" if times.get(n) else "       n/a            "
            mem = lambda n: f"{peaks[n]:8.1f}" if n in peaks else "     n/a"
            print(f"{str(dtype).split('.')[-1]:>8} {name:>6} {Q:5d} {M:3d} {D:3d} {L:2d} {P:2d} | {cell('fused')} | {cell('fused_fwd')} | {cell('torch')} || "
                  f"{mem('fused')} (+ {ws:.1f} cached workspace) | {mem('torch')}", flush=True)
            deform_train._WORKSPACES.clear()


if __name__ == "__main__":
    main()
