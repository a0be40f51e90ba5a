"""CPU: the COCO evaluator's entries are exported by the built library and the ctypes mirror of lwdetr_coco_gt has the compiler's layout."""
import ctypes
import os
import re
import subprocess

import pytest

from helpers import ROOT


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from lwdetr_amd import _native
    return _native


def test_cocoeval_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "lwdetr_hip.h")).read()
    declared = set(re.findall(r"\b(lwdetr_cocoeval_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"lwdetr_cocoeval_match", "lwdetr_cocoeval_match_host", "lwdetr_cocoeval_npig", "lwdetr_cocoeval_curves"}
    raw = ctypes.CDLL(built.LIB_PATH)
    for sym in sorted(declared):
        assert hasattr(raw, sym), f"{sym} declared in include/lwdetr_hip.h but not exported"
        fn = getattr(built.lib(), sym)
        assert fn.restype is ctypes.c_int and fn.argtypes, sym
    assert len(built.lib().lwdetr_cocoeval_match.argtypes) == 12 and len(built.lib().lwdetr_cocoeval_match_host.argtypes) == 11
    assert len(built.lib().lwdetr_cocoeval_npig.argtypes) == 5 and len(built.lib().lwdetr_cocoeval_curves.argtypes) == 13


def test_coco_gt_mirror_has_the_compilers_layout(built, tmp_path):
    fields = ["grp_off", "box", "area", "crowd", "cat", "cat_lut", "n_images", "n_cats", "lut_size", "n_ann", "max_group", "reserved"]
    assert [f[0] for f in built.CocoGt._fields_] == fields
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lwdetr_hip.h"\nint main(){printf("%zu", sizeof(lwdetr_coco_gt));\n' + \
          "".join(f'printf(" %zu", offsetof(lwdetr_coco_gt, {f}));\n' for f in fields) + \
          'printf(" %d %d %d %d\\n", LWDETR_COCOEVAL_MAX_DETS, LWDETR_COCOEVAL_MAX_GROUP, LWDETR_COCOEVAL_MAX_CATS, LWDETR_COCOEVAL_KEEP);return 0;}\n'
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got[0] == ctypes.sizeof(built.CocoGt)
    assert got[1:1 + len(fields)] == [getattr(built.CocoGt, f).offset for f in fields]
    assert got[1 + len(fields):] == [built.COCOEVAL_MAX_DETS, built.COCOEVAL_MAX_GROUP, built.COCOEVAL_MAX_CATS, built.COCOEVAL_KEEP]
