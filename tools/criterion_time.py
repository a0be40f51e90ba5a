"""Times the native evaluation criterion (the four launches of csrc/match.hip) beside the forward + PostProcess step of the same process:

    python tools/criterion_time.py [--size small] [--batch 32] [--dtype fp16] [--targets 7,40,100] [--n 200] [--no-model]
Per target count (every image gets that many synthetic targets; B x 300 queries x 91 classes, final + two aux + enc, outputs in --dtype):
  * HIP events around each of the four entries, median over --n calls (the phase split),
  * one captured graph of the whole criterion call, median of --n replays after warm-up (as tools/lat_bs1.py measures),
  * the solver's shortest-path step counts per (layer, image) problem,
and, once, the graph replay time of forward + PostProcess at the same batch. Written for profiles/r8a_criterion.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="small")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=640)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--targets", default="7,40,100")
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    import torch
    import lwdetr_amd
    import lwdetr_amd.models
    import criterion_ref as R
    from lwdetr_amd import _native
    from lwdetr_amd.models import criterion as NC
    from lwdetr_amd.synth import synth_images, synth_state_dict
    T = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    dev = torch.device("cuda:0")
    b, nq, ncls, nl = a.batch, 300, 91, 4
    layers = [(lg.to(dev).to(T), bx.to(dev).to(T)) for lg, bx in R.synth_outputs(nl, b, nq, ncls, 300)]
    outputs = R.as_outputs(layers)
    args = lwdetr_amd.get_args(a.size)
    args.native_criterion = True
    model, crit, post = lwdetr_amd.build_model(args)
    lib = _native.lib()

    def event_ms(fns):
        """median milliseconds of each fn of `fns` (run back to back on the current stream) over a.n rounds"""
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(a.n)]
        for r in range(a.n + 10):
            e = ev[max(r - 10, 0)]
            e[0].record()
            for k, fn in enumerate(fns):
                fn()
                e[k + 1].record()
        torch.cuda.synchronize(dev)
        return [median([e[k].elapsed_time(e[k + 1]) for e in ev]) for k in range(len(fns))]

    for t in [int(x) for x in a.targets.split(",")]:
        targets = [{k: v.to(dev) for k, v in tg.items()} for tg in R.synth_targets((t,) * b, ncls, 300)]
        m = crit.matcher
        loss = crit(outputs, targets)                                # warm-up: workspaces, offsets
        torch.cuda.synchronize(dev)
        steps = m.steps().flatten().tolist()
        assert not m.status().any() and all(torch.isfinite(v).item() for v in loss.values())
        arr, keep = NC._layer_array(layers, True)
        packed = NC._Packed(targets, dev, nq, m._offsets)
        ws = m._workspace(dev, nl, b, nq, ncls, packed.sum_t)
        out = torch.empty(nl, 5, dtype=torch.float32, device=dev)
        st, dt = _native.stream_ptr(dev), _native.dtype_code(T)
        lp, bp, op = packed.labels.data_ptr(), packed.boxes.data_ptr(), packed.offsets.data_ptr()
        four = [
            lambda: _native.check(lib.lwdetr_match_cost(arr, nl, b, nq, ncls, lp, bp, op, packed.counts_c, 2.0, 5.0, 2.0, 0.25, ws.cost.data_ptr(), dt, st), "cost"),
            lambda: _native.check(lib.lwdetr_match_assign(ws.cost.data_ptr(), op, packed.counts_c, nl, b, nq, ws.idx_q.data_ptr(), ws.idx_t.data_ptr(),
                                                          ws.status.data_ptr(), ws.steps.data_ptr(), st), "assign"),
            lambda: _native.check(lib.lwdetr_criterion_partials(arr, nl, b, nq, ncls, lp, bp, op, packed.counts_c, ws.idx_q.data_ptr(), ws.idx_t.data_ptr(),
                                                                0, 0.25, ws.partials.data_ptr(), dt, st), "partials"),
            lambda: _native.check(lib.lwdetr_criterion_finish(ws.partials.data_ptr(), arr, op, packed.counts_c, nl, b, nq, 0, float(max(packed.sum_t, 1)),
                                                              out.data_ptr(), st), "finish"),
        ]
        phase = event_ms(four)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            crit(outputs, targets)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            crit(outputs, targets)
        lat = []
        for i in range(a.n + 20):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            graph.replay()
            torch.cuda.synchronize(dev)
            if i >= 20:
                lat.append((time.perf_counter() - t0) * 1e3)
        print(f"criterion B={b} nq={nq} C={ncls} layers={nl} {a.dtype} T={t}/image: events cost {phase[0]:.4f} assign {phase[1]:.4f} partials {phase[2]:.4f} "
              f"finish {phase[3]:.4f} sum {sum(phase):.4f} ms | one graph (packing included) p50 {median(lat):.4f} ms | solver steps per problem "
              f"min {min(steps)} median {median(steps)} max {max(steps)} (bound {t * (t + 1) // 2})", flush=True)
        del graph

    if not a.no_model:
        model.load_state_dict(synth_state_dict(model.state_dict(), seed=0))
        model = model.to(dev).to(T).eval()
        images = synth_images(b, a.res, a.res, seed=1234).to(dev).to(T)
        sizes = torch.tensor([[480.0, 640.0]] * b, device=dev)
        graphed = model.capture(images, postprocess=post["bbox"], target_sizes=sizes)
        lat = []
        for i in range(a.n + 20):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            graphed(images)
            torch.cuda.synchronize(dev)
            if i >= 20:
                lat.append((time.perf_counter() - t0) * 1e3)
        print(f"forward + PostProcess {a.size} B={b} {a.res} {a.dtype}, one graph: p50 {median(lat):.4f} ms", flush=True)


if __name__ == "__main__":
    main()
