"""Forward + backward time and peak memory of the two-stage query selection of a training step, two ways on one device in one process:
``two_stage_select`` (csrc/two_stage_train.hip + the heads on the selected rows) and the reference's per-group loop over all rows written in
torch (``reference_loop`` below - it lives here, not in the code under test). Shapes: small (B = 4, S = 1600, d = 256) and large (B = 4,
S = 6800, d = 384) with G = 13 groups of nq = 300 queries and 91 classes, plus the shape of the memory test (B = 1, S = 6800, d = 384), in
f32 and bf16.
    python tools/two_stage_time.py [--reps 20] [--warmup 3] > profiles/r15a_two_stage_train.txt
The two are interleaved round by round (one forward + backward each per round, timed with events); the table gives medians and minima in
microseconds, the scoring launch alone (events around the one launch) with its rate as a fraction of the MFMA peak of its input type
(157.3 TFLOP/s float32, 2516.6 TFLOP/s bfloat16: 2 B S G d (d + ncls) FLOP), and the peak of torch.cuda.max_memory_allocated() over one forward
+ backward above what the inputs and parameters hold."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lwdetr_amd.ops import two_stage as T  # noqa: E402

SHAPES = [("small", 4, [(40, 40)], 256), ("large", 4, [(80, 85)], 384), ("memtest", 1, [(80, 85)], 384)]
G, NQ, NCLS = 13, 300, 91
PEAK = {torch.float32: 157.3e12, torch.bfloat16: 2516.6e12}


class BoxHead(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, 4)])

    def forward(self, x):
        return self.layers[2](F.relu(self.layers[1](F.relu(self.layers[0](x)))))


class Heads(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.enc_output = nn.ModuleList([nn.Linear(d, d) for _ in range(G)])
        self.enc_output_norm = nn.ModuleList([nn.LayerNorm(d) for _ in range(G)])
        self.enc_out_class_embed = nn.ModuleList([nn.Linear(d, NCLS) for _ in range(G)])
        self.enc_out_bbox_embed = nn.ModuleList([BoxHead(d) for _ in range(G)])


def reference_loop(memory, valid, props, m):
    """transformer.py:230-264 with bbox_reparam, over all rows, under autograd."""
    x = memory * valid.unsqueeze(-1).to(memory.dtype)
    props = props.to(memory.dtype)
    d = memory.shape[-1]
    mts, bts = [], []
    for g in range(G):
        y = m.enc_output_norm[g](m.enc_output[g](x))
        cls = m.enc_out_class_embed[g](y)
        delta = m.enc_out_bbox_embed[g](y)
        coord = torch.cat([delta[..., :2] * props[..., 2:] + props[..., :2], delta[..., 2:].exp() * props[..., 2:]], -1)
        idx = torch.topk(cls.max(-1)[0], NQ, dim=1)[1]
        bts.append(torch.gather(coord, 1, idx.unsqueeze(-1).repeat(1, 1, 4)))
        mts.append(torch.gather(y, 1, idx.unsqueeze(-1).repeat(1, 1, d)))
    return torch.cat(mts, 1), torch.cat(bts, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; G = {G}, nq = {NQ}, ncls = {NCLS}; forward + backward, {a.reps} interleaved "
          f"rounds after {a.warmup} warm-up rounds")
    print("# dtype   shape  B     S   d | us median (min): operator fwd+bwd | reference loop fwd+bwd | scoring launch alone (fraction of MFMA peak) "
          "|| peak MiB above inputs: operator | reference loop")
    for dtype in (torch.float32, torch.bfloat16):
        for name, B, levels, d in SHAPES:
            torch.manual_seed(0)
            S = sum(h * w for h, w in levels)
            m = Heads(d).to(dev).to(dtype)
            memory = torch.randn(B, S, d, device=dev, dtype=dtype, requires_grad=True)
            props, valid = T.proposals(B, levels, None, dev, unsigmoid=False)
            tm, tb = torch.randn(B, G * NQ, d, device=dev, dtype=dtype), torch.randn(B, G * NQ, 4, device=dev, dtype=dtype)
            stacked = [torch.stack([getattr(mod[g], at).detach() for g in range(G)]) for mod, at in
                       ((m.enc_output, "weight"), (m.enc_output, "bias"), (m.enc_output_norm, "weight"), (m.enc_output_norm, "bias"),
                        (m.enc_out_class_embed, "weight"), (m.enc_out_class_embed, "bias"))]

            def operator():
                _, mts, bts = T.two_stage_select(memory, None, levels, m.enc_output, m.enc_output_norm, m.enc_out_class_embed,
                                                 m.enc_out_bbox_embed, NQ, G, True)
                return mts, bts

            def loop():
                return reference_loop(memory, valid, props, m)

            def one(fn):
                for p in m.parameters():
                    p.grad = None
                memory.grad = None
                mts, bts = fn()
                torch.autograd.backward([mts, bts], [tm, tb])

            ways = [("operator", operator), ("loop", loop)]
            times, peaks = {n: [] for n, _ in ways}, {}
            times["scores"] = []
            for n, fn in ways:
                one(fn)                                                     # first call: allocator pools
                for p in m.parameters():
                    p.grad = None
                memory.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                mts, bts = fn()
                torch.autograd.backward([mts, bts], [tm, tb])
                del mts, bts
                torch.cuda.synchronize()
                peaks[n] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            for r in range(a.warmup + a.reps):
                for n, fn in ways:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    one(fn)
                    e1.record()
                    e1.synchronize()
                    if r >= a.warmup:
                        times[n].append(e0.elapsed_time(e1) * 1e3)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                T.two_stage_scores(memory, valid, *stacked)
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    times["scores"].append(e0.elapsed_time(e1) * 1e3)
            cell = lambda n: f"{statistics.median(times[n]):9.1f} ({min(times[n]):9.1f})"
            flop = 2.0 * B * S * G * d * (d + NCLS)
            frac = flop / (statistics.median(times["scores"]) * 1e-6) / PEAK[dtype]
            print(f"{str(dtype).split('.')[-1]:>8} {name:>7} {B:2d} {S:5d} {d:3d} | {cell('operator')} | {cell('loop')} | {cell('scores')} ({frac:6.1%}) || "
                  f"{peaks['operator']:8.1f} | {peaks['loop']:8.1f}", flush=True)


if __name__ == "__main__":
    main()
