"""Register / LDS / scratch usage of every kernel in an object or in the built shared library (from the code objects' metadata notes; needs no GPU):
    python tools/kernel_regs.py lw-detr_amd/csrc/build/gemm.o [name-filter]
    python tools/kernel_regs.py lw-detr_amd/liblwdetr_hip.so gemm_few_kernel
``kernel_table(path)`` returns the same as a list of dicts (tests/test_gemm_few_f32_host.py).
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
INT_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def _demangle(text):
    try:
        return subprocess.run(["c++filt"], input=text, capture_output=True, text=True, check=True).stdout
    except (OSError, subprocess.CalledProcessError):
        return text


def kernel_table(obj, arch="gfx950"):
    """One dict per kernel of ``obj`` (a .o, or a .so that holds one offload bundle per translation unit): ``symbol`` (mangled), ``name`` (demangled
    where c++filt can), and the integer fields of INT_KEYS."""
    rows = []
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "a.fatbin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), data)]
        for n, (lo, hi) in enumerate(zip(starts, starts[1:] + [len(data)])):
            part, co = os.path.join(td, f"b{n}.fatbin"), os.path.join(td, f"b{n}.co")
            with open(part, "wb") as f:
                f.write(data[lo:hi])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}", f"--input={part}",
                            f"--output={co}", "--unbundle"], check=True)
            if not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
            cur = {}
            for ln in notes.splitlines():
                m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)", ln)
                if not m:
                    continue
                k, v = m.group(1), m.group(2).strip().strip("'")
                if k == "agpr_count" and cur.get("name"):           # first key of the next kernel's entry
                    rows.append(cur)
                    cur = {}
                cur[k] = v
            if cur.get("name"):
                rows.append(cur)
    names = _demangle("\n".join(r["name"] for r in rows)).splitlines() if rows else []
    out = []
    for r, nm in zip(rows, names):
        e = {"symbol": r["name"], "name": nm}
        for k in INT_KEYS:
            e[k] = int(r[k]) if str(r.get(k, "")).lstrip("-").isdigit() else None
        out.append(e)
    return out


def main(obj, flt=""):
    q = lambda v: "?" if v is None else v
    for r in kernel_table(obj):
        if flt and flt not in r["name"] and flt not in r["symbol"]:
            continue
        print(f"vgpr {q(r['vgpr_count']):>4} agpr {q(r['agpr_count']):>4} sgpr {q(r['sgpr_count']):>4} spill {q(r['vgpr_spill_count']):>4} "
              f"scratch {q(r['private_segment_fixed_size']):>5} lds {q(r['group_segment_fixed_size']):>6}  {r['name'][:150]}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
