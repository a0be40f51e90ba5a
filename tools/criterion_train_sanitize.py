"""Sanitizer run of the host forms of the training criterion, outside Python: builds csrc/match.hip + csrc/match_train.hip +
tools/criterion_train_host_check.cpp into one stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer on the host side, and
runs it - the grouped solve (lwdetr_match_assign_host per column slice) and lwdetr_criterion_grad_host - on single images of the fixture
batches of tests/criterion_train_ref.py in all four loss forms, plus a batch with NaN / inf costs, logits and boxes. What it writes for the
clean inputs is compared with the fixture's pairs and the fp64 restatement's gradients (the host test's bound). Needs hipcc, no GPU.
    python tools/criterion_train_sanitize.py [--keep DIR]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [("h7", 0, None), ("h91", 0, None), ("g3", 0, None), ("g3", 2, None), ("g3", 3, None), ("c366", 2, None), ("g13", 2, ("focal", "possup"))]


def run(exe, work, tag, env, nq, c, t, g, form, alpha, num_boxes, grad_out, logits, boxes, labels, tboxes, cost_tm):
    fin, fout = os.path.join(work, f"in_{tag}.bin"), os.path.join(work, f"out_{tag}.bin")
    with open(fin, "wb") as f:
        np.asarray([nq, c, t, g, form], np.int32).tofile(f)
        np.asarray([alpha, num_boxes, *grad_out], np.float32).tofile(f)
        for arr, dt in ((logits, np.float32), (boxes, np.float32), (labels, np.int64), (tboxes, np.float32), (cost_tm, np.float32)):
            np.ascontiguousarray(arr, dt).tofile(f)
    r = subprocess.run([exe, fin, fout], env=env, capture_output=True, text=True, timeout=600)
    print(tag, r.stdout.strip(), r.stderr.strip()[-4000:])
    if r.returncode != 0:
        raise SystemExit(f"sanitizer run failed with exit code {r.returncode}")
    raw, pos, out = open(fout, "rb").read(), 0, []
    for n, dt in ((g * t, np.int64), (g * t, np.int64), (g, np.int32), (g, np.int32), (nq * c, np.float32), (nq * 4, np.float32)):
        out.append(np.frombuffer(raw, dtype=dt, count=n, offset=pos))
        pos += n * np.dtype(dt).itemsize
    assert pos == len(raw)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="build and run in this directory and leave the files there")
    a = ap.parse_args()
    import criterion_ref as R
    import criterion_train_ref as TR
    work = a.keep or tempfile.mkdtemp(prefix="criterion_train_san_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "criterion_train_host_check")
    csrc = os.path.join(ROOT, "lw-detr_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-slp-vectorize",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
           os.path.join(csrc, "match.hip"), os.path.join(csrc, "match_train.hip"), "-x", "hip",
           os.path.join(ROOT, "tools", "criterion_train_host_check.cpp"), "-fsanitize=address,undefined", "-o", exe]
    print(" ".join(cmd))
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    fx = np.load(os.path.join(ROOT, "tests", "golden", "criterion_train.npz"), allow_pickle=False)
    worst = 0.0
    for name, b, forms in CASES:
        s = TR.BATCHES[name]
        layers, targets = TR.batch_inputs(name, int(fx[name + ".seed"]), "f32")
        keys = [str(k) for k in fx[name + ".keys"]]
        w = TR.loss_weights(keys)
        iq, it = fx[f"{name}.f32.idx_q"], fx[f"{name}.f32.idx_t"]
        idx, pos = [], 0
        for _ in range(s["layers"]):
            lay = []
            for t in s["counts"]:
                lay.append((iq[pos:pos + t * s["G"]], it[pos:pos + t * s["G"]]))
                pos += t * s["G"]
            idx.append(lay)
        lg, bx = layers[0]
        tg = targets[b]
        t = len(tg["labels"])
        cost = R.cost_matrix(lg[b], bx[b], tg["labels"], tg["boxes"], **R.COST_W).numpy().astype(np.float32)
        num_boxes = max(float(sum(s["counts"]) * s["G"]), 1.0)
        grad_out = [w["loss_ce"], 0.0, w["loss_bbox"], w["loss_giou"], 0.0]
        for form in forms or TR.FORMS:
            _, ref, _ = TR.gradients(layers, targets, form, s["G"], w, indices=idx)
            got = run(exe, work, f"{name}_{b}_{form}", env, s["nq"], s["C"], t, s["G"], TR.FORMS.index(form), R.FOCAL_ALPHA, num_boxes, grad_out,
                      lg[b].numpy(), bx[b].numpy(), tg["labels"].numpy(), tg["boxes"].numpy(), cost.T)
            assert np.array_equal(got[0], idx[0][b][0]) and np.array_equal(got[1], idx[0][b][1]) and not got[2].any(), (name, b, form)
            gdist, gmax = fx[f"{name}.f32.{form}.gdist"][0], fx[f"{name}.f32.{form}.gmax"][0]
            for k, (g, r) in enumerate(((got[4].reshape(s["nq"], s["C"]), ref[0][0][b].numpy()), (got[5].reshape(s["nq"], 4), ref[0][1][b].numpy()))):
                err, bound = np.abs(g.astype(np.float64) - r).max(), 4.0 * gdist[k] + 1e-6 * gmax[k]
                worst = max(worst, err / bound)
                assert err <= bound, (name, b, form, k, err, bound)
    # non-finite inputs: a NaN solver row, inf entries, a NaN logit row, an inf box, a negative width - the program must return, nothing more is asked
    layers, targets = TR.batch_inputs("g3", int(fx["g3.seed"]), "f32")
    lg, bx, tg = layers[0][0][3].numpy().copy(), layers[0][1][3].numpy().copy(), targets[3]
    cost = R.cost_matrix(layers[0][0][3], layers[0][1][3], tg["labels"], tg["boxes"], **R.COST_W).numpy().astype(np.float32).T.copy()
    cost[4, :] = np.nan
    cost[9, ::3] = np.inf
    cost[11, 40:] = -np.inf
    lg[5, :], lg[50, 2] = np.nan, np.inf
    bx[7, :], bx[8, 2], bx[60, 0] = np.inf, -1.0, np.nan
    for form in TR.FORMS:
        got = run(exe, work, f"nonfinite_{form}", env, 111, 7, 37, 3, TR.FORMS.index(form), R.FOCAL_ALPHA, 135.0, [1.0, 0.0, 1.0, 1.0, 0.0], lg, bx,
                  tg["labels"].numpy(), tg["boxes"].numpy(), cost)
        assert got[2].all()                                      # every group saw the NaN row
        q, t = got[0].reshape(3, 37), got[1].reshape(3, 37)
        assert all(np.array_equal(q[g], np.arange(37 * g, 37 * g + 37)) and sorted(t[g].tolist()) == list(range(37)) for g in range(3))
    print(f"criterion_train sanitizer run: clean (address, undefined); pairs equal the fixture, worst gradient error / bound = {worst:.3f}")


if __name__ == "__main__":
    main()
