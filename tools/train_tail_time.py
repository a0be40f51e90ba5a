"""Times the tail of one training step - gradient clip, AdamW over one group per parameter, model EMA - on the real parameter sets of the tiny,
small and large models with random gradients, on the GPU, for
  native    : lwdetr_amd.train.NativeAdamW(max_norm=0.1, ema=ModelEma) - three launches, and the ema.update() call that finds its work done;
  reference : torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW at its defaults over the same groups + the reference's ModelEma.update loop.
Per size and side: host time of the calls (a host clock around the calls, no synchronise inside), stream time (device events around the same
calls: for a launch-bound sequence this is what the device waits, not what it computes), launches per step (native: the library's counter;
reference: kernels seen by torch.profiler in one step). For the native kernels beside that: time per launch from events around a train of
back-to-back launches, and the bytes the algorithm moves over that time against the 6.3 TB/s copy figure. The two sides alternate inside one
process, several rounds; medians and the spread over rounds are printed.
    python tools/train_tail_time.py [--sizes tiny small large] [--out profiles/r11a_train_tail.txt]"""
import argparse
import copy
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lwdetr_amd  # noqa: E402
from lwdetr_amd import _native, train as T  # noqa: E402

ARGS = dict(lr=1e-4, lr_encoder=1.5e-4, lr_vit_layer_decay=0.8, lr_component_decay=0.7, weight_decay=1e-4)
COPY_BW = 6.3e12
MAX_NORM, DECAY = 0.1, 0.9997


def timed(fn, iters):
    """(host seconds per call, stream seconds per call) of fn over `iters` calls: the queue is empty at the start and drained at the end."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = time.perf_counter() - t0
    b.record()
    torch.cuda.synchronize()
    return host / iters, a.elapsed_time(b) * 1e-3 / iters


def reference_ema_update(shadow, model, decay):
    with torch.no_grad():
        for ev, mv in zip(shadow.state_dict().values(), model.state_dict().values()):
            ev.copy_(decay * ev + (1. - decay) * mv)


def kernel_count(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n if n > 0 else None
    except Exception as exc:                                         # the count is then reported as not measured
        print(f"  (torch.profiler unavailable: {type(exc).__name__}: {exc})")
        return None


def one_size(size, iters, rounds, emit):
    args = lwdetr_amd.get_args(size)
    for k, v in ARGS.items():
        setattr(args, k, v)
    model, _, _ = lwdetr_amd.build_model(args)
    model = model.to("cuda")
    ref_model = copy.deepcopy(model)
    gen = torch.Generator(device="cuda").manual_seed(3)
    for m in (model, ref_model):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=gen, device="cuda") * 1e-3
    nparam, nelem, nsd = sum(1 for _ in model.parameters()), sum(p.numel() for p in model.parameters()), len(model.state_dict())
    small = sum(1 for p in model.parameters() if p.numel() <= 1024)
    # native
    ema = T.ModelEma(model, decay=DECAY)
    opt = T.NativeAdamW(T.get_param_dict(args, model), lr=args.lr, weight_decay=args.weight_decay, max_norm=MAX_NORM, ema=ema)

    def native():
        opt.step()
        ema.update(model)
    # reference
    ref_params = [p for p in ref_model.parameters()]
    ref_opt = torch.optim.AdamW(T.get_param_dict(args, ref_model), lr=args.lr, weight_decay=args.weight_decay)
    shadow = copy.deepcopy(ref_model).eval()

    def reference():
        torch.nn.utils.clip_grad_norm_(ref_params, MAX_NORM)
        ref_opt.step()
        reference_ema_update(shadow, ref_model, DECAY)
    for _ in range(3):
        native()
        reference()
    res = {"native": [], "reference": []}
    for _ in range(rounds):
        res["native"].append(timed(native, iters))
        res["reference"].append(timed(reference, max(1, iters // 4)))
    before = _native.mt_launch_counts()
    native()
    after = _native.mt_launch_counts()
    n_native = sum(after[k] - before[k] for k in after)
    emit(f"== {size}: {nparam} parameters ({small} of them <= 1024 elements), {nelem / 1e6:.2f} M elements, {nsd} state-dict entries, "
         f"{opt._tables.nchunks} chunks")
    for side in ("native", "reference"):
        host, stream = [h for h, _ in res[side]], [s for _, s in res[side]]
        emit(f"  {side:9s}: host {statistics.median(host) * 1e3:8.3f} ms (min {min(host) * 1e3:.3f} max {max(host) * 1e3:.3f})   "
             f"stream {statistics.median(stream) * 1e3:8.3f} ms (min {min(stream) * 1e3:.3f} max {max(stream) * 1e3:.3f})")
    emit(f"  native launches per step (the library's counter): {n_native}, and one 30 KB host-to-device copy of the tensor table")
    hn, sn = statistics.median(h for h, _ in res["native"]), statistics.median(s for _, s in res["native"])
    hr, sr = statistics.median(h for h, _ in res["reference"]), statistics.median(s for _, s in res["reference"])
    emit(f"  reference / native: host {hr / hn:.1f} x, stream {sr / sn:.1f} x")
    # the native kernels alone: a train of back-to-back launches on tables that are already uploaded
    tb = opt._tables
    hyper = T._hyper(0.9, 0.999, 1e-8, DECAY)
    rec = tb.rec
    n_par = len(opt._params())
    par_elems = int(rec["numel"][:n_par].sum())
    ema_par = int(rec["numel"][:n_par][rec["ema"][:n_par] != 0].sum())
    extra = int(rec["numel"][n_par:][rec["kind"][n_par:] == _native.MT_EMA_F32].sum())
    step_bytes = par_elems * 28 + ema_par * 8 + extra * 12                   # p, m, v read + written, g read; ema read + written; buffers x, e, e
    trains = {"mt_sumsq + mt_norm_finish": (lambda: tb.norm(MAX_NORM), par_elems * 4),
              "mt_step (ADAMW | EMA)": (lambda: tb.step(hyper, _native.MT_ADAMW | _native.MT_EMA, True), step_bytes)}
    for name, (fn, nbytes) in trains.items():
        fn()
        ts = [timed(fn, 50)[1] for _ in range(rounds)]
        t = statistics.median(ts)
        emit(f"  {name:27s}: {t * 1e6:8.1f} us per launch (min {min(ts) * 1e6:.1f} max {max(ts) * 1e6:.1f}), {nbytes / 1e6:.1f} MB -> "
             f"{nbytes / t / 1e12:.2f} TB/s = {100 * nbytes / t / COPY_BW:.0f} % of the 6.3 TB/s copy figure")
    return reference


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["tiny", "small", "large"])
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11a_train_tail.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_tail_time.py measures on the GPU; there is nothing to report without one")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()

    def emit(s):
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    emit(f"training-step tail, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; max_norm {MAX_NORM}, EMA decay {DECAY}, "
         f"{a.iters} calls per window, {a.rounds} rounds, sides alternating")
    refs = [(size, one_size(size, a.iters, a.rounds, emit)) for size in a.sizes]
    emit("== reference launches per step (kernels torch.profiler sees in one clip + AdamW + EMA-loop step, copies and memsets left out)")
    for size, reference in refs:
        n = kernel_count(reference)
        emit(f"  {size}: {n if n is not None else 'not measured'}")


if __name__ == "__main__":
    main()
