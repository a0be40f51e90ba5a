"""Forward + backward time and peak memory of the ViT attention core of a 4-image training step, three ways on one device in one process:
FusedAttentionFunction (csrc/attention_train.hip), the reference formulation (scores materialised, torch autograd) and
F.scaled_dot_product_attention. Shapes: the windowed block (64 sequences x 12 heads, N = 100 / 196) and the global block (4 x 12,
N = 1600 / 3136) at the head sizes of vit_tiny / small / base, f32 and bf16.
    python tools/attn_train_time.py [--reps 30] [--warmup 5] > profiles/r13a_attn_train.txt
The three are interleaved round by round (one forward + backward each per round, timed with events); the table gives medians and minima in
microseconds and the peak of torch.cuda.max_memory_allocated() over one forward + backward above what the inputs hold."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lwdetr_amd.ops import FusedAttentionFunction  # noqa: E402

SHAPES = [(64, 100, 16), (64, 100, 32), (64, 100, 64), (64, 196, 16), (4, 1600, 16), (4, 1600, 32), (4, 1600, 64), (4, 3136, 16)]
HEADS = 12


def fused(qkv, scale):
    return FusedAttentionFunction.apply(qkv, scale)


def formulation(qkv, scale):
    B, N, _, H, D = qkv.shape
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    w = ((q * scale) @ k.transpose(-2, -1)).softmax(dim=-1)
    return (w @ v).transpose(1, 2).reshape(B, N, H * D)


def sdpa(qkv, scale):
    B, N, _, H, D = qkv.shape
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    return F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(B, N, H * D)


def one(fn, qkv, scale, t):
    qkv.grad = None
    fn(qkv, scale).backward(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; forward + backward, {a.reps} interleaved rounds after {a.warmup} warm-up rounds")
    print("# dtype  seqs heads     N  hd | us median (min): fused | formulation | sdpa || peak MiB above inputs: fused | formulation | sdpa")
    ways = [("fused", fused), ("formulation", formulation), ("sdpa", sdpa)]
    for dtype in (torch.float32, torch.bfloat16):
        for B, N, D in SHAPES:
            torch.manual_seed(0)
            qkv = torch.randn(B, N, 3, HEADS, D, device=dev, dtype=dtype, requires_grad=True)
            t = torch.randn(B, N, HEADS * D, device=dev, dtype=dtype)
            scale = D ** -0.5
            times, peaks, alive = {}, {}, []
            for name, fn in ways:
                try:
                    qkv.grad = None
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    one(fn, qkv, scale, t)
                    torch.cuda.synchronize()
                    peaks[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                    alive.append((name, fn))
                    times[name] = []
                except Exception as e:                                  # a backend that does not take this dtype / shape
                    print(f"# {name} refused {dtype} N={N} hd={D}: {type(e).__name__}: {str(e)[:100]}")
            for r in range(a.warmup + a.reps):
                for name, fn in alive:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    one(fn, qkv, scale, t)
                    e1.record()
                    e1.synchronize()
                    if r >= a.warmup:
                        times[name].append(e0.elapsed_time(e1) * 1e3)

            def cell(name):
                return f"{statistics.median(times[name]):9.1f} ({min(times[name]):9.1f})" if name in times else "       n/a            "

            def mem(name):
                return f"{peaks[name]:8.1f}" if name in peaks else "     n/a"
            print(f"{str(dtype).split('.')[-1]:>8} {B:5d} {HEADS:5d} {N:5d} {D:3d} | " + " | ".join(cell(n) for n, _ in ways) + " || "
                  + " | ".join(mem(n) for n, _ in ways), flush=True)


if __name__ == "__main__":
    main()
