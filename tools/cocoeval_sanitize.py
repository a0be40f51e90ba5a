"""Sanitizer run of the host form of the COCO matching kernel, outside Python: builds csrc/cocoeval.hip + tools/cocoeval_host_check.cpp
into one stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer on the host side, runs it on every batch of the
generated set of tests/cocoeval_cases.py (plus one batch with NaN / inf records), and compares what it wrote with the oracle
(tests/cocoeval_ref.py). Needs hipcc, no GPU.   python tools/cocoeval_sanitize.py [--keep DIR]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="build and run in this directory and leave the files there")
    a = ap.parse_args()
    import cocoeval_cases as CS
    import cocoeval_ref as R
    from lwdetr_amd import coco_eval as CE
    work = a.keep or tempfile.mkdtemp(prefix="cocoeval_san_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "cocoeval_host_check")
    cmd = [os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fno-slp-vectorize", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "lw-detr_amd", "csrc", "cocoeval.hip"), "-x", "hip", os.path.join(ROOT, "tools", "cocoeval_host_check.cpp"),
           "-fsanitize=address,undefined", "-o", exe]
    print(" ".join(cmd))
    subprocess.check_call(cmd)
    g = CS.generated()
    gt = CE.CocoGroundTruth(g["dataset"])
    nan_ids, nan_packed = g["evaluated"][0][0], g["evaluated"][0][1].copy()
    nan_packed[0, 0, 2:] = np.nan
    nan_packed[0, 1, 4] = np.inf
    nan_packed[0, 2, 0] = np.nan
    runs = [g["evaluated"], [(nan_ids, nan_packed)]]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for batches in runs:
        _, (cat, rank, matched, ignored) = CS.oracle_run(R, g["dataset"], batches)
        got = [[] for _ in range(5)]
        for n, (ids, packed) in enumerate(batches):
            rows = gt.rows_of(ids)
            B, K = packed.shape[:2]
            fin, fout = os.path.join(work, f"in{n}.bin"), os.path.join(work, f"out{n}.bin")
            with open(fin, "wb") as f:
                np.asarray([len(gt.img_ids), len(gt.cat_ids), len(gt.cat_lut), len(gt.area), gt.max_group, B, K], np.int32).tofile(f)
                for arr in (gt.grp_off, gt.box, gt.area, gt.cat, gt.cat_lut, rows, np.ascontiguousarray(packed, np.float32),
                            np.ascontiguousarray(CE.IOU_THRS, np.float64), gt.crowd):
                    arr.tofile(f)
            r = subprocess.run([exe, fin, fout], env=env, capture_output=True, text=True, timeout=300)
            print(r.stdout.strip(), r.stderr.strip()[-4000:])
            if r.returncode != 0:
                raise SystemExit(f"sanitizer run failed with exit code {r.returncode}")
            raw = open(fout, "rb").read()
            n_el, pos = B * K, 0
            for j, dt in enumerate((np.int32, np.float32, np.int32, np.int64, np.int64)):
                got[j].append(np.frombuffer(raw, dtype=dt, count=n_el, offset=pos))
                pos += n_el * np.dtype(dt).itemsize
        got = [np.concatenate(x) for x in got]
        assert np.array_equal(got[0], cat) and np.array_equal(got[2], rank) and np.array_equal(got[3], matched) and np.array_equal(got[4], ignored)
    print("cocoeval sanitizer run: clean (address, undefined), outputs equal the oracle")


if __name__ == "__main__":
    main()
