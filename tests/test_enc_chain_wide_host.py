"""CPU: the host side of the wide-class form of lwdetr_enc_chain (96 < ncls <= 384, lw-detr_amd/csrc/chain.hip + chain_enc_body.h).

(1) kernels.pack_enc_chain for 97 / 366 / 384 classes walked lane by lane as the kernel walks it with 12 class tiles
    (tests/enc_chain_wide_sim.py) equals the dense float64 chain; pad columns are zero, the row maximum runs over columns < ncls.
(2) Stream / vector sizes equal the class-count helpers of the C ABI; the two older helpers return what they always returned.
(3) What the C entry refuses before any launch (lwdetr_enc_chain_check: the entry's own argument checks, no device call).
(4) kernels.enc_chain_supported against LWDETR_CHAIN_WIDE_CLS and LWDETR_CHAIN."""
import ctypes as C

import numpy as np
import pytest
import torch

import lwdetr_amd  # noqa: F401
from lwdetr_amd import kernels as K
from enc_chain_wide_sim import simulate_enc_wave_cols

FORMS = [(256, 640), (256, 0), (384, 0)]


def _ln(x, g, b, eps):
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def _pieces(d, k5, nl, cols):
    return ((d // 32) * (k5 // 64) if k5 else 0) + (nl * (d // 32) + d // 32 + cols // 32) * (d // 64) + 2


def _vec_floats(d, k5, cols):
    return ((3 * d if k5 else 0) + 3 * d + cols + 6 * d + 1023) // 1024 * 1024


# ---------------------------------------------------------------------------------------------------------------- (1) lane-level walk
@pytest.mark.parametrize("ncls", [97, 366, 384])
@pytest.mark.parametrize("d,k5", FORMS)
def test_wide_stream_walk_equals_dense(d, k5, ncls):
    nl = 3 if d == 256 else 2
    g = torch.Generator().manual_seed(d + k5 + ncls)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()      # f32-representable: the packer keeps f32 masters
    w_enc, b_enc, g_enc, be_enc = r(d, d) / 16, r(d), (1 + 0.125 * r(d)).float().double(), 0.125 * r(d)
    w_cls, b_cls = r(ncls, d) / 16, r(ncls)
    w_val, b_val = r(nl * d, d) / 16, r(nl * d)
    cv2 = ((r(d, k5) / 32).float().double(), r(d), (1 + 0.125 * r(d)).float().double(), 0.125 * r(d)) if k5 else None
    stream, vec = K.pack_enc_chain(d, torch.float64, w_enc, b_enc, g_enc, be_enc, w_cls, b_cls, w_val, b_val, cv2=cv2)
    cols = K.enc_chain_class_cols(ncls)
    assert cols == 384
    pieces = _pieces(d, k5, nl, cols)
    assert stream.numel() == pieces * 2048
    assert vec.numel() == _vec_floats(d, k5, cols)
    x = r(32, k5 or d).numpy()
    rowvalid = (torch.rand(32, generator=g) > 0.3).numpy().astype(np.float64)
    notpad = (torch.rand(32, generator=g) > 0.2).numpy().astype(np.float64)
    eps_p, eps_e = 1e-6, 1e-5
    sim = simulate_enc_wave_cols(stream.double().numpy(), vec.double().numpy(), x, rowvalid, notpad, d, k5, nl, ncls, cols, eps_p, eps_e)
    assert sim["fragments_consumed"] == (pieces - 2) * 4                          # all but the two zero pieces of the read-ahead
    assert np.abs(stream.double().numpy()[-2 * 2048:]).max() == 0
    n = lambda t: t.double().numpy()
    if k5:
        z = x @ n(cv2[0]).T + n(cv2[1])
        mem = _ln(z / (1 + np.exp(-z)), n(cv2[2]), n(cv2[3]), eps_p)
        np.testing.assert_allclose(sim["memory"], mem, rtol=0, atol=1e-9)
    else:
        mem = x
    vals = (mem @ n(w_val).T + n(b_val)) * notpad[:, None]
    np.testing.assert_allclose(sim["values"], vals.reshape(32, nl, d).transpose(1, 0, 2), rtol=0, atol=1e-9)
    om = _ln((mem * rowvalid[:, None]) @ n(w_enc).T + n(b_enc), n(g_enc), n(be_enc), eps_e)
    np.testing.assert_allclose(sim["om"], om, rtol=0, atol=1e-9)
    cls = om @ n(w_cls).T + n(b_cls)
    np.testing.assert_allclose(sim["cls"][:, :ncls], cls, rtol=0, atol=1e-9)
    if ncls < cols:
        assert np.abs(sim["cls"][:, ncls:]).max() == 0
    np.testing.assert_allclose(sim["cls_max"], cls.max(1), rtol=0, atol=1e-9)


def test_narrow_packing_is_unchanged_by_the_class_columns():
    """Up to 96 classes the class block is 96 rows, as ever: the stream and the vector of a 91-class model have the sizes of the older helpers'
    formulas, and 96 classes still take the narrow layout."""
    d, nl = 256, 3
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g)
    for ncls in (1, 91, 96):
        stream, vec = K.pack_enc_chain(d, torch.float16, r(d, d), r(d), r(d), r(d), r(ncls, d), r(ncls), r(nl * d, d), r(nl * d))
        assert K.enc_chain_class_cols(ncls) == 96
        assert stream.numel() == _pieces(d, 0, nl, 96) * 2048 == 142 * 2048 and vec.numel() == 3072
    with pytest.raises(ValueError):
        K.enc_chain_class_cols(385)
    with pytest.raises(ValueError):
        K.enc_chain_class_cols(0)


# ---------------------------------------------------------------------------------------------------------------- (2) the C size helpers
def _lib():
    from lwdetr_amd import _native
    assert _native.is_built(), f"{_native.LIB_PATH} is not built"
    return _native.lib()


def test_size_helpers_by_class_count_and_the_older_ones():
    lib = _lib()
    # the older helpers: literal values of (k5 ? 3 D : 0) + 3 D + 96 + 6 D floats rounded up to 4 KB, and of
    # (k5 ? D / 32 * k5 / 64 : 0) + (nl * D / 32 + D / 32 + 3) * D / 64 + 2 pieces
    assert [lib.lwdetr_enc_chain_vec_floats(d, k5) for d, k5 in FORMS] == [4096, 3072, 4096]
    assert [lib.lwdetr_enc_chain_pieces(d, k5, 3) for d, k5 in FORMS] == [222, 142, 308]
    assert [lib.lwdetr_enc_chain_pieces(d, k5, 2) for d, k5 in FORMS] == [190, 110, 236]
    assert lib.lwdetr_enc_chain_pieces(256, 0, 6) == 238
    assert [lib.lwdetr_enc_chain_class_cols(n) for n in (1, 91, 96, 97, 366, 384)] == [96, 96, 96, 384, 384, 384]
    assert lib.lwdetr_enc_chain_class_cols(0) < 0 and lib.lwdetr_enc_chain_class_cols(-5) < 0 and lib.lwdetr_enc_chain_class_cols(385) < 0
    for d, k5 in FORMS:
        for nl in (1, 2, 3, 6):
            for ncls in (1, 91, 96):          # the narrow layout: the older helpers' values
                assert lib.lwdetr_enc_chain_pieces_cls(d, k5, nl, ncls) == lib.lwdetr_enc_chain_pieces(d, k5, nl)
                assert lib.lwdetr_enc_chain_vec_floats_cls(d, k5, ncls) == lib.lwdetr_enc_chain_vec_floats(d, k5)
            for ncls in (97, 366, 384):       # 9 more class tiles of D / 64 pieces each; 288 more bias floats, inside the same 4 KB multiple
                assert lib.lwdetr_enc_chain_pieces_cls(d, k5, nl, ncls) == lib.lwdetr_enc_chain_pieces(d, k5, nl) + 9 * (d // 64) == _pieces(d, k5, nl, 384)
                assert lib.lwdetr_enc_chain_vec_floats_cls(d, k5, ncls) == lib.lwdetr_enc_chain_vec_floats(d, k5) == _vec_floats(d, k5, 384)
        assert lib.lwdetr_enc_chain_pieces_cls(d, k5, 3, 385) < 0 and lib.lwdetr_enc_chain_vec_floats_cls(d, k5, 0) < 0
    assert [lib.lwdetr_enc_chain_pieces_cls(d, k5, 3, 366) for d, k5 in FORMS] == [258, 178, 362]


@pytest.mark.parametrize("ncls", [91, 366])
@pytest.mark.parametrize("d,k5", FORMS)
def test_packed_sizes_equal_the_helpers(d, k5, ncls):
    lib = _lib()
    nl = 3
    z = torch.zeros
    cv2 = (z(d, k5), z(d), z(d), z(d)) if k5 else None
    stream, vec = K.pack_enc_chain(d, torch.float16, z(d, d), z(d), z(d), z(d), z(ncls, d), z(ncls), z(nl * d, d), z(nl * d), cv2=cv2)
    assert stream.numel() * 2 == lib.lwdetr_enc_chain_pieces_cls(d, k5, nl, ncls) * 4096
    assert vec.numel() == lib.lwdetr_enc_chain_vec_floats_cls(d, k5, ncls)


# ---------------------------------------------------------------------------------------------------------------- (3) refusals before any launch
BAD_ARG, UNSUPPORTED = -1, -2
# `values` is a HOST array that the checks read (six dummy device pointers, 16-byte aligned), unlike every other pointer argument
_VALUES = (C.c_void_p * 6)(*[0x50000 + 0x1000 * i for i in range(6)])


def _args(**kw):
    """Arguments lwdetr_enc_chain takes (dummy pointers, every one 16-byte aligned; nothing is dereferenced before the checks are through):
    D = 256 without cv2, 3 layers, one image of 100 tokens, 91 classes in rows of 96."""
    a = dict(inp=0x10000, ld_in=256, k5=0, memory=None, om=0x20000, cls=0x30000, ld_cls=96, cls_max=0x40000, values=_VALUES, nl=3,
             rowvalid=0x60000, notpad=0x70000, wstream=0x80000, vec=0x90000, M=100, D=256, npix=100, S=100, lsi=0, total_rows=100,
             ncls=91, dtype=1)
    a.update(kw)
    return a


def _check(**kw):
    a = _args(**kw)
    order = ("inp", "ld_in", "k5", "memory", "om", "cls", "ld_cls", "cls_max", "values", "nl", "rowvalid", "notpad", "wstream", "vec", "M", "D",
             "npix", "S", "lsi", "total_rows", "ncls", "dtype")
    lib = _lib()
    rc = lib.lwdetr_enc_chain_check(*[a[k] for k in order])
    if rc != 0:
        # the entry itself answers the same, and returns before it touches the device or any of the (dummy) pointers
        head = [a[k] for k in order[:-1]]
        assert lib.lwdetr_enc_chain(*head, C.c_float(1e-6), C.c_float(1e-5), a["dtype"], None) == rc
    return rc


def test_the_entry_refuses_bad_class_counts_and_strides_before_any_launch():
    assert _check(ncls=385, ld_cls=392) == BAD_ARG
    assert _check(ncls=366, ld_cls=96) == BAD_ARG                  # the wide form needs rows of 384 columns ...
    assert _check(ncls=366, ld_cls=368) == BAD_ARG                 # ... not ceil8(ncls)
    assert _check(ncls=97, ld_cls=376) == BAD_ARG
    assert _check(ncls=366, ld_cls=388) == BAD_ARG                 # 16-byte stores: ld_cls % 8
    assert _check(ncls=0) == BAD_ARG
    assert _check(ncls=-1) == BAD_ARG
    # accepted (the checks are through; a launch would follow)
    assert _check(ncls=96, ld_cls=96) == 0
    assert _check(ncls=91, ld_cls=96) == 0
    assert _check(ncls=91, ld_cls=104) == 0
    assert _check(ncls=97, ld_cls=384) == 0
    assert _check(ncls=366, ld_cls=384) == 0
    assert _check(ncls=384, ld_cls=392) == 0
    assert _check(ncls=366, ld_cls=384, D=384, ld_in=384, dtype=2) == 0
    assert _check(ncls=366, ld_cls=384, k5=640, ld_in=640, memory=0xA0000) == 0


def test_the_entry_keeps_its_older_refusals_in_the_wide_form():
    w = dict(ncls=366, ld_cls=384)
    assert _check(**w, nl=0) == BAD_ARG and _check(**w, nl=7) == BAD_ARG
    assert _check(**w, ld_in=260) == BAD_ARG
    assert _check(**w, S=99) == BAD_ARG and _check(**w, lsi=-1) == BAD_ARG and _check(**w, npix=0) == BAD_ARG
    assert _check(**w, k5=640, ld_in=640) == BAD_ARG               # cv2 in front without a `memory` to write
    assert _check(**w, cls=0x30008) == BAD_ARG
    assert _check(**w, om=None) == BAD_ARG
    assert _check(**w, D=192, ld_in=192) == UNSUPPORTED
    assert _check(**w, D=384, ld_in=640, k5=640, memory=0xA0000) == UNSUPPORTED
    assert _check(**w, dtype=0) == UNSUPPORTED
    # the 2 GB range of the buffer descriptors is taken with the real row stride: 2.7 M rows of 384 class columns fit, 2.8 M do not
    # (with 96 columns the D = 256 tensors set the limit: 4.19 M rows)
    assert _check(**w, total_rows=2_790_000) == 0
    assert _check(**w, total_rows=2_800_000) == UNSUPPORTED
    assert _check(total_rows=2_800_000) == 0
    assert _check(total_rows=4_200_000) == UNSUPPORTED
    assert _check(**w, M=0, nl=0) == 0                             # no rows: nothing to do, as ever


# ---------------------------------------------------------------------------------------------------------------- (4) the plan switch
def test_enc_chain_supported_takes_wide_class_counts_only_behind_its_switch(monkeypatch):
    F16, BF16 = torch.float16, torch.bfloat16
    monkeypatch.delenv("LWDETR_CHAIN", raising=False)
    monkeypatch.delenv("LWDETR_CHAIN_WIDE_CLS", raising=False)
    big, few = 4 * K.CHAIN_MIN_ROWS, K.CHAIN_MIN_ROWS - 1
    wide, narrow = (97, 366, 384), (1, 91, 96)
    for sw in (None, "0", ""):                                     # the default: off
        if sw is not None:
            monkeypatch.setenv("LWDETR_CHAIN_WIDE_CLS", sw)
        for d, k5 in FORMS:
            for n in wide:
                assert not K.enc_chain_supported(d, F16, k5=k5, ncls=n) and not K.enc_chain_supported(d, BF16, k5=k5, ncls=n, rows=big)
            for n in narrow:
                assert K.enc_chain_supported(d, F16, k5=k5, ncls=n) and K.enc_chain_supported(d, BF16, k5=k5, ncls=n, rows=big)
    monkeypatch.setenv("LWDETR_CHAIN", "1")
    assert not K.enc_chain_supported(256, F16, ncls=366, rows=big)  # forcing the chains on does not widen them
    assert K.enc_chain_supported(256, F16, ncls=91, rows=few)
    monkeypatch.setenv("LWDETR_CHAIN_WIDE_CLS", "1")
    monkeypatch.delenv("LWDETR_CHAIN")
    for d, k5 in FORMS:
        for n in wide + narrow:
            assert K.enc_chain_supported(d, F16, k5=k5, ncls=n) and K.enc_chain_supported(d, BF16, k5=k5, ncls=n)
            assert K.enc_chain_supported(d, F16, k5=k5, ncls=n, rows=big) and not K.enc_chain_supported(d, F16, k5=k5, ncls=n, rows=few)
        assert not K.enc_chain_supported(d, F16, k5=k5, ncls=385) and not K.enc_chain_supported(d, F16, k5=k5, ncls=1024, rows=big)
    assert not K.enc_chain_supported(256, torch.float32, ncls=366) and not K.enc_chain_supported(384, F16, k5=640, ncls=366)
    assert not K.enc_chain_supported(256, F16, ncls=366, nl=7)
    monkeypatch.setenv("LWDETR_CHAIN", "1")
    assert K.enc_chain_supported(256, F16, ncls=366, rows=few) and K.enc_chain_supported(384, BF16, ncls=97, rows=few)
    monkeypatch.setenv("LWDETR_CHAIN", "0")
    assert not K.enc_chain_supported(256, F16, ncls=366, rows=big) and not K.enc_chain_supported(256, F16, ncls=91, rows=big)
    assert K.enc_chain_supported(256, F16, ncls=366)               # (without rows: "is there a kernel", not the plan's choice)


def test_no_enc_chain_kernel_uses_scratch():
    """All twelve kernels (six narrow, six wide) of the built library: no scratch, no spills; the wide ones are there under a name that the
    barrier checks of tests/test_isa_guard.py pick up."""
    import os
    import sys
    from lwdetr_amd import _native
    _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_regs.kernel_table(_native.LIB_PATH) if "enc_chain_kernel" in r["symbol"]]
    assert len(rows) == 12 and sum("enc_chain_kernel_wide" in r["symbol"] for r in rows) == 6, [r["symbol"] for r in rows]
    for r in rows:
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
