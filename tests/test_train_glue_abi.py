"""CPU: the argument checks of csrc/train_glue.hip answer before anything is launched (no device is touched), the workspace formula, and the
launch-form record's names."""
import ctypes as C

import pytest

from lwdetr_amd import _native as N


@pytest.fixture(scope="module")
def lib():
    return N.lib()          # raises when the library has not been built


def _buf(nbytes=4096):
    b = (C.c_char * nbytes)()
    return b, C.addressof(b) + (-C.addressof(b)) % 16


def test_ln2d_refusals(lib):
    keep, p = _buf()
    ok = dict(B=1, C=4, HW=6, eps=1e-6, tokens=0, dtype=N.DT_F32)

    def fwd(x=p, w=p, b=p, y=p, mean=p, rstd=p, **kw):
        a = dict(ok, **kw)
        return lib.lwdetr_ln2d_forward(x, w, b, y, mean, rstd, a["B"], a["C"], a["HW"], a["eps"], a["tokens"], a["dtype"], None)

    assert fwd(dtype=N.DT_F64) == N.ERR_UNSUPPORTED and fwd(dtype=7) == N.ERR_UNSUPPORTED
    for bad in (dict(C=0), dict(C=1025), dict(B=0), dict(B=65536), dict(HW=0), dict(eps=-1.0), dict(x=None), dict(y=None), dict(mean=None),
                dict(w=p + 2), dict(x=p + 1, dtype=N.DT_F16)):
        assert fwd(**bad) == N.ERR_BAD_ARG, bad

    def bwd(ws=p, ws_floats=48, dx=p, **kw):
        a = dict(ok, **kw)
        return lib.lwdetr_ln2d_backward(p, p, p, p, p, dx, p, p, ws, ws_floats, a["B"], a["C"], a["HW"], a["tokens"], a["dtype"], None)

    assert lib.lwdetr_ln2d_workspace_floats(1, 4, 6) == 8 and lib.lwdetr_ln2d_workspace_floats(3, 384, 65) == 3 * 2 * 2 * 384
    assert lib.lwdetr_ln2d_workspace_floats(0, 4, 6) == 0
    assert bwd(ws_floats=7) == N.ERR_BAD_ARG and bwd(ws=None) == N.ERR_BAD_ARG and bwd(dx=None) == N.ERR_BAD_ARG
    assert bwd(dtype=N.DT_F64) == N.ERR_UNSUPPORTED and bwd(C=2000) == N.ERR_BAD_ARG
    del keep


def test_sine_embed_refusals(lib):
    keep, p = _buf()
    fwd = lambda boxes=p, ld=4, hi=p, lo=p, out=p, rows=3, dim=128, dtype=N.DT_F32: lib.lwdetr_sine_embed_forward(boxes, ld, hi, lo, out, rows, dim,
                                                                                                               dtype, None)
    bwd = lambda go=p, gb=p, rows=3, dim=128, dtype=N.DT_F32: lib.lwdetr_sine_embed_backward(p, 4, p, p, go, gb, rows, dim, dtype, None)
    assert fwd(dtype=N.DT_F64) == N.ERR_UNSUPPORTED and bwd(dtype=N.DT_F64) == N.ERR_UNSUPPORTED
    for bad in (dict(dim=7), dict(dim=0), dict(dim=258), dict(ld=3), dict(rows=-1), dict(boxes=None), dict(hi=None), dict(lo=None), dict(out=None)):
        assert fwd(**bad) == N.ERR_BAD_ARG, bad
    assert bwd(go=None) == N.ERR_BAD_ARG and bwd(gb=None) == N.ERR_BAD_ARG and bwd(dim=5) == N.ERR_BAD_ARG
    assert fwd(rows=0) == 0 and bwd(rows=0) == 0          # nothing to do, nothing launched
    del keep


def test_launch_form_names(lib):
    names = set(N.train_glue_path_counts())
    want = {f"ln2d_{d}_{lay}_{t}" for d in ("fwd", "bwd") for lay in ("nchw", "tok") for t in ("f32", "f16", "bf16")}
    want |= {f"sine_{d}_{t}" for d in ("fwd", "bwd") for t in ("f32", "f16", "bf16")}
    assert names == want
    assert lib.lwdetr_train_glue_path_name(-1) is None and lib.lwdetr_train_glue_path_name(len(want)) is None
