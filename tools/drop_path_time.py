"""Time and peak memory of the drop-path residual, fused (``drop_path_residual``, csrc/drop_path.hip) against the torch formulation
(``drop_path_residual_torch``), on one device in one process and one build.
    python tools/drop_path_time.py [--reps 20] [--warmup 5] [--inner 50] [--model-reps 10] > profiles/r18a_drop_path.txt
Operator rows: forward + backward of ONE residual at the shape of a 4-image 640 x 640 step - 64 windows of 100 tokens - for C = 192, 384 and 768,
in f32 (x, y, gamma f32) and in the form bf16 autocast hands over (x and gamma f32, y bf16); x, y and gamma all want a gradient, keep
probability 0.9. The two ways alternate round by round; a round is ``--inner`` forward + backward passes between two device events (one pass
is a few microseconds of device work), and the table gives the median and the minimum per pass in microseconds, and the peak of
torch.cuda.max_memory_allocated() over one pass (``torch.autograd.grad``: the output, what autograd keeps, the gradients) above the inputs.
Model rows: the ``large`` model's forward + backward (4 images of 640 x 640, group_detr = 13) built with drop_path = 0.1, ``fused=None`` against
``fused=False`` (every fused operator in its torch formulation), and ``fused=None`` with the rate set to 0 by ``update_drop_path`` - the
configuration of profiles/r17a_train_model.txt - and ``fused=None`` with the residual alone left to its torch formulation (the dispatch's
``drop_path_supports`` answering no), which is the comparison that decides the dispatch; alternated in the same way, one pass per event pair,
milliseconds.
``--ways fused`` / ``--ways torch`` with ``--no-model`` runs one way alone, for a kernel trace of its own (the operator rows are bound by the
host's launch rate: the device time per pass is the sum of the trace's kernel times over the passes):
    rocprofv3 --kernel-trace --stats -d DIR -o fused --output-format csv -- python tools/drop_path_time.py --no-model --ways fused --reps 4 --warmup 1 --inner 10
    (the same with torch), then, without a device,
    python tools/drop_path_time.py --kernel-stats DIR/fused_kernel_stats.csv DIR2/torch_kernel_stats.csv --reps 4 --warmup 1 --inner 10
prints per way the kernels launched once per pass or more, their mean time, and the sum per pass."""
import argparse
import csv
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lwdetr_amd  # noqa: E402
from lwdetr_amd.models import train_forward as TF  # noqa: E402
from lwdetr_amd.models.train_forward import differentiable_forward  # noqa: E402
from lwdetr_amd.ops import drop_path_keep, drop_path_residual, drop_path_residual_torch  # noqa: E402
from lwdetr_amd.synth import synth_images, synth_state_dict  # noqa: E402

GROUPS, ROWS = 64, 100


def timed(ways, reps, warmup, inner):
    """ways: [(name, callable)] -> {name: [time of one call in ms]}; the ways alternate round by round."""
    times = {n: [] for n, _ in ways}
    for r in range(warmup + reps):
        for n, fn in ways:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[n].append(e0.elapsed_time(e1) / inner)
    return times


def peak_of(fn):
    fn()                                                            # first call: allocator pools, gradients allocated
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def operator_rows(a, dev):
    print("# one residual, forward + backward, 64 windows x 100 tokens; us per pass median (min): fused | torch || peak MiB above the "
          "inputs: fused | torch")
    for c in a.channels:
        for dy in (torch.float32, torch.bfloat16):
            g = torch.Generator(device=dev).manual_seed(c)
            x = torch.randn(GROUPS, ROWS, c, generator=g, device=dev).requires_grad_()
            y = torch.randn(GROUPS, ROWS, c, generator=g, device=dev).to(dy).requires_grad_()
            gamma = torch.full((c,), 0.1, device=dev).requires_grad_()
            cot = torch.randn(GROUPS, ROWS, c, generator=g, device=dev)
            keep = drop_path_keep(x, GROUPS, 0.1)

            def one(fn):
                torch.autograd.grad(fn(x, y, gamma, keep, 0.1), (x, y, gamma), cot)

            ways = [("fused", lambda: one(drop_path_residual)), ("torch", lambda: one(drop_path_residual_torch))]
            ways = [w for w in ways if w[0] in a.ways]
            peaks = {n: peak_of(fn) for n, fn in ways}
            t = timed(ways, a.reps, a.warmup, a.inner)
            peaks, t = {"fused": 0.0, "torch": 0.0, **peaks}, {"fused": [0.0], "torch": [0.0], **t}
            cell = lambda n: f"{1e3 * statistics.median(t[n]):8.1f} ({1e3 * min(t[n]):8.1f})"
            name = "f32" if dy == torch.float32 else "f32 + bf16"
            print(f" C = {c:4d} {name:>10} | {cell('fused')} | {cell('torch')} || {peaks['fused']:7.2f} | {peaks['torch']:7.2f}   "
                  f"(kept {int(keep.sum())} of {GROUPS})", flush=True)


def flat(out):
    t = [out["pred_logits"], out["pred_boxes"], out["enc_outputs"]["pred_logits"], out["enc_outputs"]["pred_boxes"]]
    for aux in out["aux_outputs"]:
        t += [aux["pred_logits"], aux["pred_boxes"]]
    return t


def model_rows(a, dev):
    print("# large, 4 images of 640 x 640, group_detr = 13, built with drop_path = 0.1; model forward + backward; ms median (min): fused=None | "
          "fused=False | fused=None at rate 0 | fused=None, the residual in torch || peak MiB above parameters, gradients and images, in the same "
          "order")
    args = lwdetr_amd.get_args("large")
    args.drop_path = 0.1
    depth = args.vit_encoder_num_layers
    model, _, _ = lwdetr_amd.build_model(args)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=0))
    model = model.to(dev).train()
    images = synth_images(4, 640, 640, seed=7).to(dev)
    for autocast in (False, True):
        cots = None

        def one(fused, rate, residual_fused=True):
            nonlocal cots
            model.update_drop_path(rate, depth)
            supports = TF.DP.drop_path_supports
            if not residual_fused:
                TF.DP.drop_path_supports = lambda *args: False
            try:
                with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
                    out = flat(differentiable_forward(model, images, fused=fused))
            finally:
                TF.DP.drop_path_supports = supports
            if cots is None:
                g = torch.Generator(device=dev).manual_seed(1)
                cots = [torch.randn(t.shape, generator=g, device=dev, dtype=torch.float32).to(t.dtype) for t in out]
            torch.autograd.backward(out, cots)

        ways = [("fused", lambda: one(None, 0.1)), ("torch", lambda: one(False, 0.1)), ("rate0", lambda: one(None, 0.0)),
                ("residual", lambda: one(None, 0.1, residual_fused=False))]
        peaks = {n: peak_of(fn) for n, fn in ways}
        t = timed(ways, a.model_reps, 3, 1)
        cell = lambda n: f"{statistics.median(t[n]):8.2f} ({min(t[n]):8.2f})"
        print(f" large {'bf16 autocast' if autocast else 'f32':>13} | {cell('fused')} | {cell('torch')} | {cell('rate0')} | {cell('residual')} || "
              f"{peaks['fused']:9.1f} | {peaks['torch']:9.1f} | {peaks['rate0']:9.1f} | {peaks['residual']:9.1f}", flush=True)


def kernel_stats_rows(a):
    """The device time of a pass from rocprofv3 kernel statistics of one-way runs: kernels with fewer launches than passes are set-up."""
    passes = len(a.channels) * 2 * (2 + (a.warmup + a.reps) * a.inner)
    print(f"# device time per pass from kernel traces of one-way runs ({passes} passes: {len(a.channels)} channel counts x 2 dtype forms x "
          f"(2 + ({a.warmup} + {a.reps}) x {a.inner})), mean over the six rows; kernels launched at least once per pass")
    for path in a.kernel_stats:
        total = 0
        for r in csv.DictReader(open(path)):
            calls, ns = int(r["Calls"]), int(r["TotalDurationNs"])
            if calls < passes // 2:
                continue
            total += ns
            name = r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
            print(f"   {os.path.basename(path):>24} | {calls / passes:5.2f} launches per pass | {ns / calls / 1e3:7.2f} us mean | {name[:72]}")
        print(f"   {os.path.basename(path):>24} | device time per pass {total / passes / 1e3:7.2f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--model-reps", type=int, default=10)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--ways", default="fused,torch")
    ap.add_argument("--channels", default="192,384,768")
    ap.add_argument("--kernel-stats", nargs="+", default=None)
    a = ap.parse_args()
    a.ways, a.channels = a.ways.split(","), [int(c) for c in a.channels.split(",")]
    if a.kernel_stats:
        return kernel_stats_rows(a)
    dev = torch.device("cuda")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {a.reps} interleaved rounds after {a.warmup} warm-up rounds, {a.inner} "
          f"passes per round (operator rows); {a.model_reps} rounds after 3 (model rows)")
    operator_rows(a, dev)
    if not a.no_model:
        model_rows(a, dev)


if __name__ == "__main__":
    main()
