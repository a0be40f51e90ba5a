"""CPU: what lwdetr_row_chain and lwdetr_enc_chain (lw-detr_amd/csrc/chain.hip) refuse before any launch, through the C ABI with dummy pointers.
Every refusal sits in front of the first device call, so nothing here touches a GPU; of the pointers only the host array `values` is read.

The four argument sets that used to be accepted although the kernels cannot honour them:
  * lwdetr_row_chain: ld_in < k_in, ld_res < D, ld_q < D (rows overlap, the last rows' loads fall behind the buffer bound and read zeros);
  * lwdetr_enc_chain_check: ld_in < (k5 ? k5 : D);
  * lwdetr_enc_chain_check: the largest memory row of the launch, ((M - 1) / npix) S + lsi + (M - 1) % npix, against total_rows
    (rowvalid / notpad / cls_max are plain pointer accesses at that row);
  * lwdetr_enc_chain_check: values[i] null or misaligned (the entry always refused it; the check now reads the host array and answers the same).
lwdetr_row_chain checks the rules on in / res / qpos in FRONT of its M == 0 return (they refuse whatever M is) and the per-stage rules after it
(with M == 0 they are not looked at): both sides are asserted below. tests/test_gpu_chain_fp64.py runs the same calls with the launch-form
record watched: no counter moves."""
import ctypes as C

import lwdetr_amd  # noqa: F401
from lwdetr_amd import _native

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
F32, F16, BF16 = 0, 1, 2
FULL, SIDE = _native.CHAIN_FULL, _native.CHAIN_SIDE
RES, RELU, LN, STORE, ADDQ = _native.CHAIN_RES, _native.CHAIN_RELU, _native.CHAIN_LN, _native.CHAIN_STORE, _native.CHAIN_ADDQ
_VALUES = (C.c_void_p * 6)(*[0x50000 + 0x1000 * i for i in range(6)])       # a host array of six aligned dummy device pointers


def _lib():
    assert _native.is_built(), f"{_native.LIB_PATH} is not built"
    return _native.lib()


def test_the_record_names_24_forms_by_rule():
    names = list(_native.chain_path_counts())
    want = ([f"enc_{t}_{f}_{w}" for t in ("f16", "bf16") for f in ("d256_pf1", "d256_pf0", "d384_pf0") for w in ("narrow", "wide")]
            + [f"row_{t}_d256_{f}" for t in ("f16", "bf16") for f in ("k512", "res0_q0", "res1_q0", "res1_q1")]
            + [f"split_{t}_d{d}" for t in ("f16", "bf16") for d in (256, 384)])
    assert names == want and len(set(names)) == 24
    lib = _lib()
    assert lib.lwdetr_chain_path_counts(None, 0) == 24 and lib.lwdetr_chain_path_name(24) is None and lib.lwdetr_chain_path_name(-1) is None
    buf = (C.c_long * 30)(*[-7] * 30)
    assert lib.lwdetr_chain_path_counts(buf, 30) == 24 and list(buf[24:]) == [-7] * 6 and all(v >= 0 for v in buf[:24])


# ---------------------------------------------------------------------------------------------------------------- lwdetr_row_chain
def row(stages, *, D=256, k_in=None, M=100, ld_in=None, res=None, ld_res=0, qpos=None, ld_q=0, inp=0x10000, wstream=0x80000, vec=0x90000, dtype=F16):
    """rc of lwdetr_row_chain for a description with dummy pointers; stages: (kind, n, flags, out, ldo)."""
    d = _native.ChainDesc()
    k_in = D if k_in is None else k_in
    d.inp, d.ld_in, d.k_in = inp, k_in if ld_in is None else ld_in, k_in
    d.res, d.ld_res, d.qpos, d.ld_q = res, ld_res, qpos, ld_q
    d.wstream, d.vec, d.M, d.D, d.nst = wstream, vec, M, D, len(stages)
    for i, (kind, n, flags, out, ldo) in enumerate(stages):
        s = d.st[i]
        s.kind, s.n, s.flags, s.eps, s.out, s.ldo = kind, n, flags, 1e-5, out, ldo
    before = _native.chain_path_counts()
    rc = _lib().lwdetr_row_chain(C.byref(d), dtype, None)
    assert _native.chain_path_counts() == before, "a refused request counts nothing"
    return rc


FRONT = [(FULL, 256, RES | LN | STORE | ADDQ, 0xA0000, 256), (SIDE, 96, 0, 0xB0000, 96)]
BACK = [(FULL, 256, RES | LN | STORE, 0xA0000, 256)]
PLAIN = [(FULL, 256, RELU | STORE, 0xA0000, 256)]
R = dict(res=0x20000, ld_res=256)
Q = dict(qpos=0x30000, ld_q=256)


def test_row_chain_refuses_strides_shorter_than_the_row_whatever_m_is():
    for M in (100, 1, 0):
        assert row(PLAIN, M=M, ld_in=248) == BAD_ARG
        assert row(PLAIN, M=M, k_in=512, ld_in=256) == BAD_ARG
        assert row(BACK, M=M, res=0x20000, ld_res=248) == BAD_ARG
        assert row(BACK, M=M, res=0x20000, ld_res=0) == BAD_ARG
        assert row(FRONT, M=M, **R, qpos=0x30000, ld_q=248) == BAD_ARG
        assert row(PLAIN, M=M, **R, qpos=0x30000, ld_q=128) == BAD_ARG           # given but used by no stage: the kernels load it all the same
        assert row(PLAIN, M=M, res=0x20000, ld_res=128) == BAD_ARG
        assert row(PLAIN, M=M, D=384, ld_in=256) == BAD_ARG
        assert row(PLAIN, M=M, D=384, **R) == BAD_ARG                            # 256 < D = 384
        # the older rules on the same operands sit in the same place
        assert row(PLAIN, M=M, ld_in=260) == BAD_ARG and row(PLAIN, M=M, inp=0x10008) == BAD_ARG
        assert row(BACK, M=M, res=0x20008, ld_res=256) == BAD_ARG and row(FRONT, M=M, **R, qpos=0x30008, ld_q=256) == BAD_ARG
        assert row(BACK, M=M, res=0x20000, ld_res=260) == BAD_ARG
    # the other side of the M == 0 return: valid row operands -> LWDETR_OK, nothing to do; strides LARGER than the row are fine; a stride that belongs to
    # no pointer is not looked at
    assert row(PLAIN, M=0) == OK and row(FRONT, M=0, **R, **Q) == OK and row(PLAIN, M=0, ld_in=264) == OK
    assert row(FRONT, M=0, res=0x20000, ld_res=264, qpos=0x30000, ld_q=512) == OK
    assert row(PLAIN, M=0, ld_res=8, ld_q=8) == OK
    assert row(PLAIN, M=0, k_in=512, ld_in=512) == OK and row(PLAIN, M=0, D=384, ld_in=384) == OK
    assert row(PLAIN, M=-1) == BAD_ARG


def test_row_chain_stage_rules_come_after_the_m0_return():
    side_flag = [(FULL, 256, RELU, None, 0), (SIDE, 4, RELU, 0xB0000, 4)]
    no_out = [(FULL, 256, STORE, None, 256)]
    short_ldo = [(FULL, 256, 0, None, 0), (SIDE, 91, 0, 0xB0000, 88)]
    ldo_mod = [(FULL, 256, STORE, 0xA0000, 260)]
    for prog in (side_flag, no_out, short_ldo, ldo_mod):
        assert row(prog, M=100) == BAD_ARG and row(prog, M=0) == OK
    assert row(FRONT, M=100, **Q) == BAD_ARG and row(FRONT, M=0, **Q) == OK      # qpos without res
    assert row(BACK, M=100) == BAD_ARG                                           # RES without a res pointer
    assert row([(FULL, 256, ADDQ | STORE, 0xA0000, 256)], M=100, **Q) == BAD_ARG


def test_row_chain_unsupported_forms_launch_nothing():
    assert row(PLAIN, dtype=F32) == UNSUPPORTED and row([(FULL, 384, RELU | STORE, 0xA0000, 384)], D=384, dtype=F32) == UNSUPPORTED
    assert row(PLAIN, k_in=512, ld_in=512, dtype=F32) == UNSUPPORTED
    assert row(PLAIN, D=384, k_in=768, ld_in=768) == UNSUPPORTED
    assert row(PLAIN, k_in=512, ld_in=512, **R) == UNSUPPORTED and row(PLAIN, k_in=512, ld_in=512, **R, **Q) == UNSUPPORTED
    assert row([(SIDE, 4, 0, 0xB0000, 4)], k_in=512, ld_in=512) == UNSUPPORTED
    assert row([(FULL, 256, LN, None, 0)] * 6) == UNSUPPORTED                    # 6 x 3 x 256 floats of vectors: 18 KB > 16 KB
    assert row([(FULL, 256, LN, None, 0)] * 5 + [(FULL, 256, 0, None, 0)], M=0) == OK
    assert row(PLAIN, D=192, ld_in=192) == UNSUPPORTED and row([], M=100) == UNSUPPORTED
    assert row([(SIDE, 0, 0, 0xB0000, 4)]) == UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- lwdetr_enc_chain
ORDER = ("inp", "ld_in", "k5", "memory", "om", "cls", "ld_cls", "cls_max", "values", "nl", "rowvalid", "notpad", "wstream", "vec", "M", "D",
         "npix", "S", "lsi", "total_rows", "ncls", "dtype")


def enc(**kw):
    """rc of lwdetr_enc_chain_check; where it refuses, the entry itself must answer the same (it returns before any device call)."""
    a = dict(inp=0x10000, ld_in=256, k5=0, memory=None, om=0x20000, cls=0x30000, ld_cls=96, cls_max=0x40000, values=_VALUES, nl=3,
             rowvalid=0x60000, notpad=0x70000, wstream=0x80000, vec=0x90000, M=100, D=256, npix=100, S=100, lsi=0, total_rows=100,
             ncls=91, dtype=F16)
    a.update(kw)
    lib = _lib()
    rc = lib.lwdetr_enc_chain_check(*[a[k] for k in ORDER])
    if rc != 0:
        before = _native.chain_path_counts()
        assert lib.lwdetr_enc_chain(*[a[k] for k in ORDER[:-1]], C.c_float(1e-6), C.c_float(1e-5), a["dtype"], None) == rc
        assert _native.chain_path_counts() == before
    return rc


def test_enc_chain_refuses_an_input_stride_shorter_than_the_row():
    assert enc(ld_in=248) == BAD_ARG and enc(ld_in=0) == BAD_ARG
    assert enc(D=384, ld_in=256) == BAD_ARG
    assert enc(k5=640, memory=0xA0000, ld_in=256) == BAD_ARG and enc(k5=640, memory=0xA0000, ld_in=632) == BAD_ARG
    assert enc(ld_in=256) == OK and enc(ld_in=264) == OK and enc(D=384, ld_in=384) == OK and enc(k5=640, memory=0xA0000, ld_in=640) == OK
    assert enc(k5=640, memory=0xA0000, ld_in=648) == OK


def test_enc_chain_compares_the_largest_memory_row_with_total_rows():
    # one image: rows lsi .. lsi + M - 1
    assert enc(total_rows=99) == BAD_ARG and enc(total_rows=100) == OK
    assert enc(S=137, lsi=19, total_rows=118) == BAD_ARG and enc(S=137, lsi=19, total_rows=119) == OK
    # three images of 50 pixels in rows of S = 87 at offset 19: the last row is 2 * 87 + 19 + 49 = 242
    g = dict(M=150, npix=50, S=87, lsi=19)
    assert enc(**g, total_rows=242) == BAD_ARG and enc(**g, total_rows=243) == OK and enc(**g, total_rows=3 * 87 + 5) == OK
    # a wave that ends inside image 1: M = 70 -> row 87 + 19 + 19 = 125
    assert enc(M=70, npix=50, S=87, lsi=19, total_rows=125) == BAD_ARG and enc(M=70, npix=50, S=87, lsi=19, total_rows=126) == OK
    # M a multiple of npix + 1: the first row of the next image
    assert enc(M=101, npix=50, S=87, lsi=19, total_rows=2 * 87 + 19) == BAD_ARG and enc(M=101, npix=50, S=87, lsi=19, total_rows=2 * 87 + 20) == OK
    assert enc(M=1, total_rows=0) == BAD_ARG and enc(M=1, total_rows=1) == OK and enc(M=1, lsi=5, total_rows=5) == BAD_ARG
    assert enc(M=0, total_rows=0) == OK                                          # no rows: nothing to do, as ever


def test_enc_chain_check_answers_for_the_values_array_as_the_entry_does():
    """`values` is a host array: lwdetr_enc_chain_check reads its entries [0, nl) once every other rule has passed and answers LWDETR_ERR_BAD_ARG for a
    null or misaligned one, as the entry does (enc() calls the entry too wherever the check refuses). Both read the array guarded: an address that
    cannot be read is BAD_ARG as well, not a fault."""
    def vals(*p):
        return (C.c_void_p * 6)(*p)
    assert enc(values=vals(0x50000, 0x51000, None)) == BAD_ARG
    assert enc(values=vals(0x50000, 0x51008, 0x52000)) == BAD_ARG
    assert enc(values=vals(None), nl=1) == BAD_ARG
    assert enc(values=vals(0x50000, 0x51000, None), nl=2) == OK                  # entries [nl, 6) are not looked at
    assert enc(values=vals(0x50000), nl=1) == OK and enc(values=vals(0x50000, 0x51000, 0x52000, 0x53000, 0x54000, 0x55000), nl=6) == OK
    assert enc(values=vals(0x50000, 0x51000, 0x52000, 0x53000, 0x54000, 0x55008), nl=6) == BAD_ARG
    assert enc(values=None) == BAD_ARG
    # the answer for everything else comes first, as in the entry: an unsupported form with a bad entry is UNSUPPORTED
    assert enc(values=vals(None), nl=1, dtype=F32) == UNSUPPORTED and enc(values=vals(None), nl=1, D=192, ld_in=192) == UNSUPPORTED
    assert enc(values=vals(None), nl=1, ld_in=248) == BAD_ARG
    assert enc(values=vals(None), M=0) == OK                                     # no rows: nothing to do, nothing read
    # an address that is not readable host memory: BAD_ARG from the check and from the entry
    assert enc(values=0x50000) == BAD_ARG and enc(values=8) == BAD_ARG and enc(values=0x50000, dtype=F32) == UNSUPPORTED
    check = lambda values, **kw: _lib().lwdetr_enc_chain_check(0x10000, 256, 0, None, 0x20000, 0x30000, 96, 0x40000, values, kw.get("nl", 3), 0x60000, 0x70000,
                                                               0x80000, 0x90000, kw.get("M", 100), 256, 100, 100, 0, 100, 91, kw.get("dtype", F16))
    assert check(0x50000) == BAD_ARG and check(8) == BAD_ARG
    assert check(0x50000, M=0) == OK and check(0x50000, dtype=F32) == UNSUPPORTED and check(0x50000, nl=7) == BAD_ARG
    assert check(_VALUES) == OK


def test_enc_chain_keeps_its_older_refusals():
    assert enc(nl=0) == BAD_ARG and enc(nl=7) == BAD_ARG and enc(nl=1) == OK and enc(nl=6) == OK
    assert enc(ncls=0) == BAD_ARG and enc(ncls=385, ld_cls=392) == BAD_ARG and enc(ncls=1) == OK and enc(ncls=384, ld_cls=384) == OK
    assert enc(ld_cls=88) == BAD_ARG and enc(ncls=97, ld_cls=96) == BAD_ARG and enc(ld_cls=100) == BAD_ARG and enc(ld_cls=104) == OK
    for name in ("inp", "om", "cls", "wstream", "vec"):
        assert enc(**{name: 0x10008}) == BAD_ARG, name
    assert enc(k5=640, ld_in=640, memory=0xA0008) == BAD_ARG
    assert enc(dtype=F32) == UNSUPPORTED and enc(D=384, k5=640, ld_in=640, memory=0xA0000) == UNSUPPORTED
