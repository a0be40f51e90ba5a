"""Sanitizer run of the host forms of the training-step tail, outside Python: builds csrc/optim.hip + tools/train_tail_host_check.cpp into one
stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and runs it on the edge set of
tests/train_tail_ref.py (every tensor an exact-size heap block, two of them one element into their block): the fused step (norm, clip, AdamW,
EMA), AdamW alone, the stand-alone clip, EMA alone, EMA_SET, and a step with NaN / inf gradients. The fused step's output is compared with the
fp64 restatement under the tests' bound. Needs hipcc, no GPU.
    python tools/train_tail_sanitize.py [--keep DIR]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PARAM, EMA_F32, EMA_I64 = 0, 1, 2
SCALE_GRADS, ADAMW, EMA, EMA_SET = 1, 2, 4, 8


def run(exe, work, tag, env, flags, clip, tensors, max_norm, betas, eps, decay):
    """tensors: [dict(kind, skip, misalign, scal=(decay_mul, neg_step_size, bc2_sqrt), arrays=[...])] -> (norm_clip, [arrays after the call])."""
    fin, fout = os.path.join(work, f"in_{tag}.bin"), os.path.join(work, f"out_{tag}.bin")
    with open(fin, "wb") as f:
        np.asarray([len(tensors), flags, clip, 1], np.int32).tofile(f)
        np.asarray([max_norm, 1 - betas[0], betas[1], 1 - betas[1], eps, decay, 1. - decay], np.float64).astype(np.float32).tofile(f)
        for t in tensors:
            np.asarray([t["arrays"][0].size, t["kind"], t["skip"], t["misalign"]], np.int32).tofile(f)
            np.asarray(t["scal"], np.float64).astype(np.float32).tofile(f)
        for t in tensors:
            for a in t["arrays"]:
                np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([exe, fin, fout], env=env, capture_output=True, text=True, timeout=600)
    print(tag, r.stdout.strip(), r.stderr.strip()[-4000:])
    if r.returncode != 0:
        raise SystemExit(f"sanitizer run failed with exit code {r.returncode}")
    raw, pos = open(fout, "rb").read(), 16
    out = []
    for t in tensors:
        got = []
        for a in t["arrays"]:
            got.append(np.frombuffer(raw, dtype=a.dtype, count=a.size, offset=pos))
            pos += a.nbytes
        out.append(got)
    assert pos == len(raw)
    return np.frombuffer(raw, dtype=np.float32, count=4), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="build and run in this directory and leave the files there")
    a = ap.parse_args()
    import torch
    import train_tail_ref as R
    work = a.keep or tempfile.mkdtemp(prefix="train_tail_san_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "train_tail_host_check")
    cmd = [os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-slp-vectorize", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "lw-detr_amd", "csrc", "optim.hip"), "-x", "hip",
           os.path.join(ROOT, "tools", "train_tail_host_check.cpp"), "-fsanitize=address,undefined", "-o", exe]
    print(" ".join(cmd))
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    case = R.make_case()
    r64, r32 = R.references(R.MAX_NORM, True)
    b1, b2 = R.BETAS

    def tensors(grads):
        ts = []
        for i, p in enumerate(case["params"]):
            g = grads[i]
            lr, wd = R.lr_of(i), R.wd_of(i)
            z = np.zeros(p.numel(), np.float32)
            ts.append(dict(kind=PARAM, skip=int(g is None), misalign=int(i in R.VIEWS), scal=(1 - lr * wd, -(lr / (1 - b1)), (1 - b2) ** 0.5),
                           arrays=[p.numpy().copy(), z.copy() if g is None else g.numpy().copy(), z.copy(), z.copy(), p.numpy().copy()]))
        ts.append(dict(kind=EMA_I64, skip=0, misalign=0, scal=(1, 0, 1), arrays=[case["bufs"][0][0].numpy().reshape(1).copy(),
                                                                                 case["buf0"][0].numpy().reshape(1).copy()]))
        for j in (1, 2):
            ts.append(dict(kind=EMA_F32, skip=0, misalign=j - 1, scal=(1, 0, 1), arrays=[case["bufs"][0][j].numpy().copy(), case["buf0"][j].numpy().copy()]))
        return ts
    common = dict(max_norm=R.MAX_NORM, betas=R.BETAS, eps=R.EPS, decay=R.DECAY)
    nc, out = run(exe, work, "fused", env, ADAMW | EMA, 1, tensors(case["grads"][0]), **common)
    assert abs(nc[0] - r64[0]["norm"]) <= 1e-6 * r64[0]["norm"]
    worst, n = 0.0, len(R.SIZES)
    for i in range(n):
        for k, slot in (("p", 0), ("m", 2), ("v", 3), ("ema", 4)):
            ref64, ref32 = r64[0][k][i], r32[0][k][i]
            if ref64 is None:                                    # the parameter without a gradient: nothing moved but its EMA entry
                assert np.array_equal(out[i][slot], np.zeros_like(out[i][slot]))
                continue
            err, bound = np.abs(out[i][slot].astype(np.float64) - ref64.numpy()).max(), R.tensor_bound(ref64, ref32)
            worst = max(worst, err / bound)
            assert err <= bound, (i, k, err, bound)
        assert np.array_equal(out[i][1], tensors(case["grads"][0])[i]["arrays"][1])            # the gradient is not rewritten
    assert int(out[n][1][0]) == int(r64[0]["ema"][n])
    for j in (1, 2):
        ref64, ref32 = r64[0]["ema"][n + j], r32[0]["ema"][n + j]
        assert np.abs(out[n + j][1].astype(np.float64) - ref64.numpy()).max() <= R.tensor_bound(ref64, ref32)
    run(exe, work, "adamw", env, ADAMW, 0, tensors(case["grads"][2]), **common)
    nc, out = run(exe, work, "scale", env, SCALE_GRADS, 1, tensors(case["grads"][0]), **common)
    for i, g in enumerate(case["grads"][0]):
        if g is not None:
            assert np.abs(out[i][1].astype(np.float64) - r64[0]["grads"][i].numpy()).max() <= R.ulp32(float(r64[0]["grads"][i].abs().max()))
    run(exe, work, "ema", env, EMA, 0, tensors(case["grads"][1]), **common)
    _, out = run(exe, work, "ema_set", env, EMA_SET, 0, tensors(case["grads"][1]), **common)
    assert all(np.array_equal(o[0], o[-1]) for o in out)
    bad = [None if g is None else g.clone() for g in case["grads"][0]]
    bad[11][17], bad[13][2048], bad[0][0] = float("nan"), float("inf"), -float("inf")
    nc, _ = run(exe, work, "nonfinite", env, ADAMW | EMA, 1, tensors(bad), **common)                # the program must return, nothing more is asked
    assert np.isnan(nc[0]) and np.isnan(nc[1])
    print(f"train_tail sanitizer run: clean (address, undefined); fused step worst error / bound = {worst:.3f}")


if __name__ == "__main__":
    main()
