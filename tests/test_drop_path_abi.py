"""CPU: the argument checks of csrc/drop_path.hip through lwdetr_drop_path_check (no device is touched), that the launch entries give the same
answers for refused calls and for rows == 0, the workspace formula, and the launch-form record's names."""
import ctypes as C

import pytest

from lwdetr_amd import _native as N

PAIRS = ((N.DT_F32, N.DT_F32), (N.DT_F16, N.DT_F16), (N.DT_BF16, N.DT_BF16), (N.DT_F32, N.DT_F16), (N.DT_F32, N.DT_BF16))


@pytest.fixture(scope="module")
def lib():
    return N.lib()          # raises when the library has not been built


def _buf(nbytes=4096):
    b = (C.c_char * nbytes)()
    return b, C.addressof(b) + (-C.addressof(b)) % 16


def _calls(lib, p):
    ok = dict(a=p, lda=8, y=p, ldy=8, gamma=p, scale=p, b=p, ldb=8, gg=p, ws=p, ws_floats=4096, rows=12, C=8, rpg=4, dx=N.DT_F32, dy=N.DT_F32)

    def check(backward, **kw):
        a = dict(ok, **kw)
        if not backward:
            a.update(gg=None, ws=None, ws_floats=0)
        return lib.lwdetr_drop_path_check(backward, a["a"], a["lda"], a["y"], a["ldy"], a["gamma"], a["scale"], a["b"], a["ldb"], a["gg"], a["ws"],
                                          a["ws_floats"], a["rows"], a["C"], a["rpg"], a["dx"], a["dy"])

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.lwdetr_drop_path_forward(a["a"], a["lda"], a["y"], a["ldy"], a["gamma"], a["scale"], a["b"], a["ldb"], a["rows"], a["C"], a["rpg"],
                                            a["dx"], a["dy"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.lwdetr_drop_path_backward(a["a"], a["lda"], a["y"], a["ldy"], a["gamma"], a["scale"], a["b"], a["ldb"], a["gg"], a["ws"],
                                             a["ws_floats"], a["rows"], a["C"], a["rpg"], a["dx"], a["dy"], None)

    return check, fwd, bwd


def test_accepted_calls(lib):
    keep, p = _buf()
    check, _, _ = _calls(lib, p)
    for dx, dy in PAIRS:
        assert check(0, dx=dx, dy=dy) == 0 and check(1, dx=dx, dy=dy) == 0, (dx, dy)
    assert check(0, gamma=None) == 0 and check(1, gamma=None, gg=None, ws=None, y=None) == 0       # the plain x + drop_path(y) form
    assert check(1, gg=None, ws=None, y=None) == 0 and check(1, b=None) == 0                      # one of the two gradients only
    assert check(0, C=2048, lda=2048, ldy=2048, ldb=2048, rows=0) == 0 and check(0, C=1, rows=3, rpg=1) == 0
    assert check(0, lda=9, ldy=24, ldb=11) == 0                                                    # own leading dimensions, any above C
    del keep


def test_refusals(lib):
    keep, p = _buf()
    check, fwd, bwd = _calls(lib, p)
    unsupported = [dict(dx=N.DT_F16, dy=N.DT_F32), dict(dx=N.DT_BF16, dy=N.DT_F16), dict(dx=N.DT_F16, dy=N.DT_BF16), dict(dx=N.DT_F64, dy=N.DT_F64),
                   dict(dx=N.DT_F32, dy=N.DT_F64), dict(dx=7, dy=7), dict(dx=-1, dy=0), dict(C=2049, lda=4096, ldy=4096, ldb=4096)]
    for bad in unsupported:
        assert check(0, **bad) == N.ERR_UNSUPPORTED and check(1, **bad) == N.ERR_UNSUPPORTED, bad
        assert fwd(**bad) == N.ERR_UNSUPPORTED and bwd(**bad) == N.ERR_UNSUPPORTED, bad
    both = [dict(a=None), dict(scale=None), dict(lda=7), dict(ldb=7), dict(rows=-1), dict(C=0), dict(C=-3), dict(rpg=0), dict(rpg=-4), dict(rpg=5),
            dict(rows=13), dict(a=p + 2), dict(b=p + 2), dict(gamma=p + 2), dict(scale=p + 1), dict(a=p + 1, dx=N.DT_F16, dy=N.DT_F16),
            dict(y=p + 1, dx=N.DT_F32, dy=N.DT_BF16), dict(y=p + 2), dict(ldy=7)]
    for bad in both:
        assert check(0, **bad) == N.ERR_BAD_ARG and check(1, **bad) == N.ERR_BAD_ARG, bad
        assert fwd(**bad) == N.ERR_BAD_ARG and bwd(**bad) == N.ERR_BAD_ARG, bad
    for bad in (dict(y=None), dict(b=None)):
        assert check(0, **bad) == N.ERR_BAD_ARG and fwd(**bad) == N.ERR_BAD_ARG, bad
    need = lib.lwdetr_drop_path_workspace_floats(12, 8)
    backward_only = [dict(ws_floats=need - 1), dict(ws=None), dict(y=None), dict(gamma=None), dict(b=None, gg=None), dict(ws=p + 2), dict(gg=p + 2)]
    for bad in backward_only:
        assert check(1, **bad) == N.ERR_BAD_ARG and bwd(**bad) == N.ERR_BAD_ARG, bad
    assert check(1, ws_floats=need) == 0
    # nothing to do, nothing launched
    assert fwd(rows=0) == 0 and bwd(rows=0) == 0
    del keep


def test_workspace_floats(lib):
    f = lib.lwdetr_drop_path_workspace_floats
    assert f(0, 8) == 0 and f(-1, 8) == 0 and f(5, 0) == 0
    assert f(1, 8) >= 8
    for c in (1, 20, 192, 2048):
        got = [f(r, c) for r in (1, 2, 15, 16, 17, 100, 3300, 6400, 6401, 1 << 20)]
        assert all(a <= b for a, b in zip(got, got[1:])), (c, got)
        assert all(g % c == 0 for g in got), (c, got)      # whole rows of per-channel partials


def test_launch_form_names(lib):
    names = list(N.drop_path_path_counts())
    pairs = ("f32_f32", "f16_f16", "bf16_bf16", "f32_f16", "f32_bf16")
    assert names == [f"dp_fwd_{p}" for p in pairs] + [f"dp_bwd_{p}" for p in pairs]
    assert lib.lwdetr_drop_path_path_name(-1) is None and lib.lwdetr_drop_path_path_name(len(names)) is None
    # the train_glue record keeps its own name set
    assert not any(n.startswith("dp_") for n in N.train_glue_path_counts())
