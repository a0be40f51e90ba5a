"""Does the wide-class encoder chain (LWDETR_CHAIN_WIDE_CLS=1, 96 < classes <= 384) pay? (tuning tool; profiles/r7d_enc_chain_wide_cls.txt is its output)

For a 366-class model (dataset_file="o365") on one launch chain:
  * the time of the one lwdetr_enc_chain launch against the sum of the launches it replaces in the plan without the switch (cv2 GEMM + LayerNorm where the
    chain takes them in front, value-projection GEMMs, enc_output GEMM + LayerNorm, class GEMM, row maximum), each launch timed alone with HIP events,
    median of 20 back-to-back repetitions (as tools/op_times.py: weights and rows are L2-warm from the repetition before);
  * the step time (whole forward, events around `steps` forwards) of the two plans, alternated round by round in ONE process, with the spread of rounds;
  * the chain launch of the 91-class model of the same size, for scale.

    python tools/enc_chain_wide_times.py --sizes small large --batch 16 --res 640 --out profiles/r7d_enc_chain_wide_cls.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["small", "large"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=640)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import lwdetr_amd
    from lwdetr_amd import _native, kernels as K
    from lwdetr_amd.models import lwdetr as L
    from lwdetr_amd.synth import synth_images, synth_state_dict
    assert torch.cuda.is_available(), "needs a ROCm device"
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[a.dtype]
    dev = torch.device("cuda:0")
    L.set_streams(1)                       # one launch chain
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def build(size, dataset, switch):
        os.environ["LWDETR_CHAIN_WIDE_CLS"] = switch       # read when the plan is built
        model, _, _ = lwdetr_amd.build_model(lwdetr_amd.get_args(size, dataset_file=dataset))
        model.load_state_dict(synth_state_dict(model.state_dict(), seed=0))
        model = model.to(dev).to(dt).eval()
        for _ in range(3):
            model(x)
        torch.cuda.synchronize()
        return model, model._plan(a.batch, a.res, a.res)

    def op_us(op, stream):
        ts = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            op(stream)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ts)

    def step_ms(model):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            model(x)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def describe(op):
        if isinstance(op, K.GemmOp):
            return f"GemmOp M={op.desc.M} N={op.desc.N} K={op.desc.K}"
        return f"RawOp {op.name}" if isinstance(op, K.RawOp) else type(op).__name__

    say(f"# tools/enc_chain_wide_times.py --sizes {' '.join(a.sizes)} --batch {a.batch} --res {a.res} --dtype {a.dtype} --rounds {a.rounds} --steps {a.steps}")
    say(f"# {torch.cuda.get_device_name(0)}, one launch chain (set_streams(1)), synthetic weights, per-launch times: median of 20 back-to-back repetitions")
    x = synth_images(a.batch, a.res, a.res, seed=1).to(dev).to(dt)
    stream = _native.stream_ptr(dev)
    for size in a.sizes:
        say()
        say(f"== {size} / o365 (366 classes), batch {a.batch}, {a.res} x {a.res}, {a.dtype}")
        m_on, p_on = build(size, "o365", "1")
        m_off, p_off = build(size, "o365", "0")
        assert p_on.use_chain and not p_off.use_chain and p_on.ldc_enc == 384, (p_on.use_chain, p_off.use_chain, p_on.ldc_enc)
        chain = [op for op in p_on.ops_enc if isinstance(op, K.EncChainOp)]
        assert len(chain) == 1 and len(p_on.ops_enc) == 1
        t_chain = op_us(chain[0], stream)
        say(f"wide chain launch (rows {p_on.B * p_on.S}, d {p_on.d}, cv2 in front: {p_on.chain_front is not None}): {t_chain:8.1f} us")
        nfront = len(p_off.ops_backbone) - len(p_on.ops_backbone)      # the projector's cv2 GEMM + LayerNorm, where the chain takes them
        assert nfront == (2 if p_on.chain_front is not None else 0), nfront
        replaced = list(p_off.ops_backbone[len(p_off.ops_backbone) - nfront:]) + list(p_off.ops_enc) + [p_off.op_rowmax]
        t_rep = 0.0
        for op in replaced:
            t = op_us(op, stream)
            t_rep += t
            say(f"    replaced launch {t:8.1f} us  {describe(op)}")
        say(f"sum of the {len(replaced)} launches it replaces: {t_rep:8.1f} us   (chain / sum = {t_chain / t_rep:.2f})")
        on, off = [], []
        for _ in range(a.rounds):
            on.append(step_ms(m_on))
            off.append(step_ms(m_off))
        for name, v in (("switch on ", on), ("switch off", off)):
            say(f"step time {name}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}  ({a.rounds} alternated rounds of {a.steps} steps)")
        diff = [f - n for n, f in zip(on, off)]
        say(f"off - on per round: median {statistics.median(diff) * 1e3:+.1f} us, min {min(diff) * 1e3:+.1f}, max {max(diff) * 1e3:+.1f}")
        del m_on, m_off, p_on, p_off
        m91, p91 = build(size, "coco", "0")
        c91 = [op for op in p91.ops_enc if isinstance(op, K.EncChainOp)]
        assert len(c91) == 1 and p91.ldc_enc == 96
        say(f"for scale, the chain launch of the 91-class model (3 class tiles): {op_us(c91[0], stream):8.1f} us")
        del m91, p91
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
