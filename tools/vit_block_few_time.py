"""Per-launch time of lwdetr_vit_block_few (projection + MLP + the next block's norm1 / QKV, one launch) on synthetic operands: HIP events, the median
of 30 single launches (each followed by a synchronise) and the mean of 200 launches issued back to back.

    python tools/vit_block_few_time.py [--dtype fp32|fp16|bf16] [--c 192|384] [--rows 1600:1600,3200:1600,6400:1600,12000:400]
rows are M:Tp pairs; --c 384 (12 heads of 32, 16-bit only) times vit_block_few384_kernel. LWDETR_HIP_LIB selects a tuning build of the library (e.g. one compiled with TUNE=-DMLP_SMALL_F32_NB=6). The seven launches an fp32
plan runs per block without LWDETR_VIT_BLOCK_FEW_F32 are timed by tools/op_times.py --dtype fp32."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--c", type=int, default=192, choices=[192, 384])
    ap.add_argument("--rows", default="1600:1600,3200:1600,6400:1600,12000:400")
    a = ap.parse_args()
    import torch
    from lwdetr_amd import _native, kernels as K
    T = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    dev = torch.device("cuda:0")
    c, heads, hd = a.c, 12, a.c // 12
    if c == 384 and a.dtype == "fp32":
        sys.exit("lwdetr_vit_block_few has no float32 form at C = 384")
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(dev)
    w1, b1, w2, b2 = rnd(4 * c, c, scale=c ** -0.5), rnd(4 * c) * 0.1, rnd(c, 4 * c, scale=(4 * c) ** -0.5), rnd(c) * 0.1
    lw, lb, g1, g2 = rnd(c) * 0.2 + 1, rnd(c) * 0.1, rnd(c) * 0.3, rnd(c) * 0.3
    wp, bp, wqkv, qb, vb = rnd(c, c, scale=c ** -0.5), rnd(c) * 0.1, rnd(3 * c, c, scale=c ** -0.5), rnd(c) * 0.1, rnd(c) * 0.1
    w1p, b1p, w2p = K.pack_mlp_weights(w1, b1, w2, lw, lb, T, proj=True)
    wq, bq = K.pack_qkv_weights(wqkv, qb, vb, lw, lb, T)
    w1F, wpF, wqF = K.pack_frag16(w1p), K.pack_frag16(wp.to(T).contiguous()), K.pack_frag16(wq)
    print(f"library {_native.LIB_PATH}  device {torch.cuda.get_device_name(0)}  dtype {a.dtype}  C {c}")
    for pair in a.rows.split(","):
        m, tp = (int(v) for v in pair.split(":"))
        nb = m // tp
        x, att = rnd(m, c).to(T), rnd(m, c).to(T)
        taps = torch.zeros(m, 2 * c, dtype=T, device=dev)
        q, k = torch.zeros(nb, heads, tp, hd, dtype=T, device=dev), torch.zeros(nb, heads, tp, hd, dtype=T, device=dev)
        vt = torch.zeros(nb, heads, hd, tp, dtype=T, device=dev)
        x0 = x.clone()
        op = K.MlpFusedOp(x, w1F, b1p, w2p, b2, g2, m, c, 1e-6, out2=taps[:, c:], ld2=2 * c, att=att, wp=wpF, bp=bp, gamma1=g1, wqkv=wqF, bqkv=bq, q=q, k=k,
                          vt=vt, qscale=0.25, heads=heads, hd=hd, Tp=tp)
        op._fn = _native.lib().lwdetr_vit_block_few
        st = _native.stream_ptr(dev)
        ev = lambda: torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            x.copy_(x0)                                              # the launch updates x in place: keep the values of a residual stream
            op(st)
        torch.cuda.synchronize()
        single = []
        for _ in range(30):
            x.copy_(x0)
            torch.cuda.synchronize()
            e0, e1 = ev(), ev()
            e0.record()
            op(st)
            e1.record()
            torch.cuda.synchronize()
            single.append(e0.elapsed_time(e1) * 1e3)
        single.sort()
        x.copy_(x0)                                                  # 200 in-place updates in a row: LayerNorm keeps every step's addend bounded
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(200):
            op(st)
        e1.record()
        torch.cuda.synchronize()
        print(f"M {m:6d} Tp {tp:5d}: single launch median {single[15]:7.1f} us (min {single[0]:.1f})   200 back to back {e0.elapsed_time(e1) * 1e3 / 200:7.1f} us per launch",
              flush=True)


if __name__ == "__main__":
    main()
