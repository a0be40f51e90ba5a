"""CPU: the multi-tensor entries of the training-step tail are exported by the built library and bound, and the ctypes / numpy mirrors of
lwdetr_mt_tensor, lwdetr_mt_chunk and lwdetr_mt_hyper have the compiler's layout."""
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


def test_mt_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "lwdetr_hip.h")).read()
    declared = set(re.findall(r"\b(lwdetr_mt_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"lwdetr_mt_check", "lwdetr_mt_sumsq", "lwdetr_mt_norm_finish", "lwdetr_mt_step", "lwdetr_mt_norm_host", "lwdetr_mt_step_host",
                        "lwdetr_mt_launch_counts", "lwdetr_mt_launch_name"}
    raw = ctypes.CDLL(built.LIB_PATH)
    for sym in sorted(declared):
        assert hasattr(raw, sym), f"{sym} declared in include/lwdetr_hip.h but not exported"
        fn = getattr(built.lib(), sym)
        assert fn.argtypes, sym
        assert fn.restype is (ctypes.c_char_p if sym == "lwdetr_mt_launch_name" else ctypes.c_int), sym
    nargs = {"lwdetr_mt_check": 4, "lwdetr_mt_sumsq": 6, "lwdetr_mt_norm_finish": 5, "lwdetr_mt_step": 8, "lwdetr_mt_norm_host": 6, "lwdetr_mt_step_host": 7}
    for sym, n in nargs.items():
        assert len(getattr(built.lib(), sym).argtypes) == n, sym
    assert built.lib().lwdetr_mt_norm_finish.argtypes[2] is ctypes.c_double and built.lib().lwdetr_mt_norm_host.argtypes[4] is ctypes.c_double
    assert list(built.mt_launch_counts()) == ["mt_sumsq", "mt_norm_finish", "mt_step"]


def test_mt_mirrors_have_the_compilers_layout(built, tmp_path):
    from lwdetr_amd import train
    structs = {"lwdetr_mt_tensor": (built.MtTensor, train._TENSOR_DT), "lwdetr_mt_chunk": (built.MtChunk, train._CHUNK_DT),
               "lwdetr_mt_hyper": (built.MtHyper, None)}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lwdetr_hip.h"\nint main(){\n'
    for name, (cls, _) in structs.items():
        src += f'printf("%zu", sizeof({name}));\n' + "".join(f'printf(" %zu", offsetof({name}, {f[0]}));\n' for f in cls._fields_) + 'printf("\\n");\n'
    src += ('printf("%d %d %d %d %u %u %u %u\\n", LWDETR_MT_CHUNK, LWDETR_MT_PARAM, LWDETR_MT_EMA_F32, LWDETR_MT_EMA_I64, LWDETR_MT_SCALE_GRADS, '
            'LWDETR_MT_ADAMW, LWDETR_MT_EMA, LWDETR_MT_EMA_SET);return 0;}\n')
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    lines = [[int(x) for x in ln.split()] for ln in subprocess.check_output([str(tmp_path / "s")]).decode().splitlines()]
    for ln, (name, (cls, dt)) in zip(lines, structs.items()):
        assert ln[0] == ctypes.sizeof(cls), name
        assert ln[1:] == [getattr(cls, f[0]).offset for f in cls._fields_], name
        if dt is not None:                                        # the numpy record the Python layer fills
            assert dt.itemsize == ln[0] and [dt.fields[f[0]][1] for f in cls._fields_] == ln[1:], name
            assert list(dt.names) == [f[0] for f in cls._fields_]
    assert lines[3] == [built.MT_CHUNK, built.MT_PARAM, built.MT_EMA_F32, built.MT_EMA_I64, built.MT_SCALE_GRADS, built.MT_ADAMW, built.MT_EMA,
                        built.MT_EMA_SET]
