"""Every kernel family behind lwdetr_gemm / lwdetr_gemm_few, forced through its own switch, pinned with the launch-path record
(lwdetr_gemm_path_counts, helpers.served_by) and checked ELEMENT BY ELEMENT against float64 arithmetic on the operands as stored.

The bound of one output y against the float64 value y64 of the same epilogue:

    |y - y64| <= 2^-p |y64| + g (c K 2^-24 sum_k |a_k w_k|) + act_slack + (f32 rounding of the epilogue) + floor

p = 11 / 8 / 24 for f16 / bf16 / f32 (half an ulp of the stored result), c = 2 (f32 accumulation of exact 16-bit products in any order,
either rounding mode), g = |scale gamma| times the activation's largest slope, act_slack = the documented error of the kernels' activation
forms (gelu_fast16 2.5e-5; gelu_erf's erf 1.5e-7; the rcpf / __expf SiLU), scaled by |scale gamma|. The residual enters as stored and is added
to the f32 value before the one rounding, so it costs only the f32 rounding of that sum. floor = half the smallest subnormal of the dtype.
Bytes of an output buffer that the launch must not write (guard rows past M, guard columns past n_end inside ldo, rows a HEADS / TOKMAP
layout does not address) must come back bit-identical."""
import math

import pytest
import torch

from helpers import served_by

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NONE, RELU, GELU, SILU = 0, 1, 2, 3
P = {F16: 11, BF16: 8, F32: 24}
FLOOR = {F16: 2.0 ** -25, BF16: 2.0 ** -134, F32: 2.0 ** -150}
U = 2.0 ** -24
C_ACC = 2
SLOPE = {NONE: 1.0, RELU: 1.0, GELU: 1.13, SILU: 1.1}      # max |d act / dz|: GELU 1.129 at z = 2.4, SiLU 1.100 at z = 2.4
WORST = {}                                                 # (family, dtype) -> largest err / bound seen (printed at the end of the module)


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def act64(z, act):
    if act == RELU:
        return z.clamp_min(0)
    if act == GELU:
        return 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))
    if act == SILU:
        return z * torch.sigmoid(z)
    return z


def act_slack(z, act, dtype):
    az = z.abs()
    if act == GELU:
        # 16-bit: gelu_fast16 (fit error 2.5e-5, plus rcpf / exp2f rounding); f32: gelu_erf (Abramowitz-Stegun erf, |error| 1.5e-7)
        return 2.5e-5 + 2.0 ** -21 * az if dtype != F32 else 1.5e-7 * az + 2.0 ** -21 * az
    if act == SILU:
        # z * rcpf(1 + __expf(-z)): exp of a rounded argument (relative error |z| 2^-24 log2 e), exp2 / rcp to a few ulp
        return 2.0 ** -21 * az * (2 + az)
    return torch.zeros_like(z)


def epilogue64(acc, s, *, dtype, K, bias=None, act=NONE, scale=1.0, gamma=None, res=None, rowmask=None, rowmask_after=False):
    """y64 and the element bound of one column segment. acc = A_view W^T and s = |A_view| |W|^T in float64 over (M, n)."""
    acc, s = acc.clone(), s.clone()
    if rowmask is not None and not rowmask_after:
        acc[~rowmask] = 0
        s[~rowmask] = 0
    b = bias.double() if bias is not None else torch.zeros(acc.shape[1], dtype=torch.float64, device=acc.device)
    z = acc + b
    sg = scale * (gamma.double() if gamma is not None else torch.ones_like(b))
    a = act64(z, act) * sg
    y = a + (res.double() if res is not None else 0)
    acc_err = C_ACC * (K + 2) * U * (s + b.abs())
    f32_err = sg.abs() * (SLOPE.get(act, 1.0) * acc_err + act_slack(z, act, dtype)) + 4 * U * (a.abs() + (res.double().abs() if res is not None else 0))
    bnd = 2.0 ** -P[dtype] * y.abs() + (1 + 2.0 ** -P[dtype]) * f32_err + FLOOR[dtype]
    if rowmask is not None and rowmask_after:
        y[~rowmask] = 0
        bnd[~rowmask] = 0
    return y, bnd


def compare(got, exp, bnd):
    """(ok, worst err / bound over the elements with a bound, number of failing elements): bound 0 = must be bit-identical."""
    d = (got.double().flatten() - exp.flatten()).abs()
    bad = ~(d <= bnd.flatten())                 # NaN fails
    pos = bnd.flatten() > 0
    worst = (d[pos] / bnd.flatten()[pos]).max().item() if bool(pos.any()) else 0.0
    return not bool(bad.any()), worst, int(bad.sum())


# ---- output addressing of the modes (flat element index of (m, n - n_begin) in the segment's buffer; -1 = not written)
def index_linear(M, n, ldo, dev):
    return torch.arange(M, device=dev)[:, None] * ldo + torch.arange(n, device=dev)[None, :]


def index_heads(M, n, p0, p1, p2, transposed, dev):
    m = torch.arange(M, device=dev)[:, None]
    nl = torch.arange(n, device=dev)[None, :]
    b, t = m // p0, m % p0
    if transposed:                                              # (B, heads, hd, Tp)
        return (b * p2 * p1 + nl) * p0 + t
    h, dd = nl // p1, nl % p1                                   # (B, heads, Tp, hd)
    return ((b * p2 + h) * p0 + t) * p1 + dd


def index_tokmap(M, n, hp, wp, ldo, obs, oro, dev, deconv_p0=0):
    m = torch.arange(M, device=dev)[:, None]
    nl = torch.arange(n, device=dev)[None, :]
    b, r = m // (hp * wp), m % (hp * wp)
    y, x = r // wp, r % wp
    if not deconv_p0:
        return b * obs + (oro + y * wp + x) * ldo + nl
    q4, co = nl // deconv_p0, nl % deconv_p0                    # out_tok: raster (2 hp, 2 wp)
    return b * obs + (oro + (2 * y + q4 // 2) * (2 * wp) + 2 * x + q4 % 2) * ldo + co


def expected(snapshot, idx, y, bnd):
    exp = snapshot.double().flatten().clone()
    b = torch.zeros_like(exp)
    exp[idx.flatten()] = y.flatten()
    b[idx.flatten()] = bnd.flatten()
    return exp, b


# ---------------------------------------------------------------------------------------------------------------- comparator self-test (CPU)
def _cpu_case(dtype=F16, M=37, n=48, K=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(dtype).double()
    W = (torch.randn(n, K, generator=g) * K ** -0.5).to(dtype).double()
    bias = torch.randn(n, generator=g) + torch.sign(torch.randn(n, generator=g)) * 0.5
    res = torch.randn(M, n, generator=g).to(dtype)
    return A, W, bias, res


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_comparator_flags_each_planted_bug(dtype):
    """The element-wise bound passes the correctly rounded result and flags every one of the planted epilogue / addressing bugs."""
    A, W, bias, res = _cpu_case(dtype)
    M, K, n = A.shape[0], A.shape[1], W.shape[0]
    acc, s = A @ W.t(), A.abs() @ W.abs().t()
    y, bnd = epilogue64(acc, s, dtype=dtype, K=K, bias=bias, res=res)
    ldo = n + 8
    snap = torch.full((M + 2, ldo), 1234.0).to(dtype)
    idx = index_linear(M, n, ldo, "cpu")

    def out_of(yy):
        o = snap.clone().flatten()
        o[idx.flatten()] = yy.to(dtype).flatten()
        return o

    exp, b = expected(snap, idx, y, bnd)
    ok, worst, _ = compare(out_of(y), exp, b)
    assert ok and worst <= 1.0, worst

    def flagged(yy_or_out):
        o = yy_or_out if yy_or_out.dim() == 1 else out_of(yy_or_out)
        return not compare(o, exp, b)[0]

    col = int(torch.argmax(bias.abs()[:16]))                    # one column's bias dropped
    bad = y.clone(); bad[:, col] -= bias[col]
    assert flagged(bad)
    y_nb, _ = epilogue64(acc, s, dtype=dtype, K=K, bias=bias, res=res, act=RELU)   # ReLU in place of the identity
    assert flagged(y_nb)
    bad = y.clone(); bad[:-1] += res[1:].double() - res[:-1].double()              # residual taken from the neighbouring row
    assert flagged(bad)
    o = out_of(y); o[idx[M - 1]] = snap.flatten()[idx[M - 1]]                      # the last (tail) row left stale
    assert flagged(o)
    bad = y.clone(); bad[:, [18, 21]] = bad[:, [21, 18]]                           # two columns swapped inside a 16-column fragment
    assert flagged(bad)
    o = out_of(y); o[M * ldo - 1] = 0.0                                            # a guard column past n_end written
    assert flagged(o)
    # HEADS_T: token and feature index transposed
    p0, p1, p2 = 16, 8, n // 8
    Mh = 2 * p0
    Ah = A[:Mh]
    yh, bh = epilogue64(Ah @ W.t(), Ah.abs() @ W.abs().t(), dtype=dtype, K=K, bias=bias)
    snap_h = torch.full((2 * p2 * p1 * p0 + 16,), 1234.0).to(dtype)
    ih = index_heads(Mh, n, p0, p1, p2, True, "cpu")
    exp_h, b_h = expected(snap_h, ih, yh, bh)
    good = snap_h.clone(); good[ih.flatten()] = yh.to(dtype).flatten()
    assert compare(good, exp_h, b_h)[0]
    t = torch.arange(Mh)[:, None] % p0
    nl = torch.arange(n)[None, :]
    # transposed addressing inside each head: element (t, d) stored at the position of (d, t) (p0 != p1, so the maps differ)
    wrong = ((torch.arange(Mh)[:, None] // p0) * p2 + nl // p1) * p1 * p0 + (t * p1 + nl % p1)
    bad = snap_h.clone(); bad[wrong.flatten()] = yh.to(dtype).flatten()
    assert not compare(bad, exp_h, b_h)[0]


def test_bound_is_not_looser_than_a_few_ulp():
    """The bound stays within a few ulp of the result where the contraction is well conditioned (no cancellation): it cannot hide a wrong bias."""
    A, W, bias, res = _cpu_case(F16, K=256)
    A, W = A.abs(), W.abs()
    y, bnd = epilogue64(A @ W.t(), A.abs() @ W.t(), dtype=F16, K=256, bias=bias.abs())
    assert float((bnd / y.abs()).max()) < 4 * 2.0 ** -11


# ---------------------------------------------------------------------------------------------------------------- GPU launches
def _dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _rand(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(_dev())


def _entry(kind):
    """The entry a case launches through, without GemmOp's automatic few-row routing (a subclass does not take it)."""
    from lwdetr_amd import kernels as K

    class _Gemm(K.GemmOp):
        pass
    return K.GemmFewOp if kind == "few" else _Gemm


def _products(Av, W):
    """float64 A_view W^T and |A_view| |W|^T: on the GPU for large shapes, on the CPU for small ones."""
    big = Av.shape[0] * W.shape[0] * Av.shape[1] > 2e7
    dev = _dev() if big else "cpu"
    a, w = Av.to(dev).double(), W.to(dev).double()
    return (a @ w.t()).to(_dev()), (a.abs() @ w.abs().t()).to(_dev())


def _im2col(x, cin, col0, stride, ho, wo):
    """(B, H, W, ctot) raster tokens -> (B ho wo, 9 cin) float64 rows of the implicit 3x3 / padding 1 view (tap-major, as the kernels read it)."""
    xp = torch.nn.functional.pad(x[..., col0:col0 + cin].double(), (0, 0, 1, 1, 1, 1))
    cols = [xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride, :] for ky in range(3) for kx in range(3)]
    return torch.cat(cols, -1).reshape(-1, 9 * cin)


SENT = 1234.0


def run_case(family, dtype, M, K, segs, *, entry="gemm", a2=False, conv=None, force=None, expect_rc=0, seed=0):
    """Builds the operands and one output buffer (with guards, filled with a sentinel) per segment, forces the path (force(knobs, lib)),
    launches ONCE, asserts the family with served_by and every element of every buffer against float64. segs: dicts with n, mode
    ("lin" / "heads" / "heads_t" / "tokmap" / "deconv"), bias, act, scale, gamma, res (None / "sep" / "inplace"), res_mod, out2,
    rowmask (None / 0 / 1 = rowmask_after), heads = (p0, p1, p2), tok = (hp, wp)."""
    from lwdetr_amd import kernels as kn
    dev = _dev()
    N = sum(s["n"] for s in segs)
    if conv is None:
        A = _rand((M, K), dtype, seed + 1)
        A2 = _rand((M, K), dtype, seed + 2) if a2 else None
        Av = (A.float() + A2.float()).to(dtype) if a2 else A          # the kernels round the operand sum to the dtype before the MFMA
        op_kw = dict(A2=A2)
    else:
        b, hp, wp, cin, stride, col0, ctot = conv
        ho, wo = (hp - 1) // stride + 1, (wp - 1) // stride + 1
        assert M == b * ho * wo and K == 9 * cin
        x = _rand((b, hp, wp, ctot), dtype, seed + 1)
        A, Av = x.reshape(-1, ctot), _im2col(x, cin, col0, stride, ho, wo)
        op_kw = dict(lda=ctot, a_mode=kn.A_CONV3x3, a_tok=kn.tok_layout(False, hp, wp, 0), conv_cin=cin, conv_stride=stride, a_col0=col0,
                     conv_hout=ho, conv_wout=wo)
    W = _rand((N, K), dtype, seed + 3, K ** -0.5)
    acc, s_abs = _products(Av, W)
    cseg, checks, keep, nb = [], [], [], 0
    for i, sp in enumerate(segs):
        n, mode = sp["n"], sp.get("mode", "lin")
        sd = seed + 10 * (i + 1)
        bias = _rand((n,), F32, sd + 1) if sp.get("bias") else None
        gamma = _rand((n,), F32, sd + 2) if sp.get("gamma") else None
        act, scale = sp.get("act", NONE), sp.get("scale", 1.0)
        rm = sp.get("rowmask")
        rowmask = (torch.rand(M, generator=torch.Generator().manual_seed(sd + 3)) < 0.7).to(torch.uint8).to(dev) if rm is not None else None
        kw = dict(bias=bias, act=act, scale=scale, gamma=gamma)
        if rowmask is not None:
            kw.update(rowmask=rowmask, rowmask_after=bool(rm))
        res = None
        if mode == "lin":
            ldo = n + 8
            out = torch.full((M + 3, ldo), SENT, dtype=dtype, device=dev)
            kw.update(ldo=ldo)
            if sp.get("res") == "sep":
                rows = sp.get("res_mod") or M
                ldres = n + 8
                res_t = _rand((rows, ldres), dtype, sd + 4)
                kw.update(res=res_t, ldres=ldres, res_mod=sp.get("res_mod", 0))
                res = res_t[torch.arange(M, device=dev) % rows, :n] if sp.get("res_mod") else res_t[:M, :n]
            elif sp.get("res") == "inplace":
                out[:M, :n] = _rand((M, n), dtype, sd + 4)
                res = out[:M, :n].clone()
                kw.update(res=out, ldres=ldo)
            idx = index_linear(M, n, ldo, dev)
        elif mode in ("heads", "heads_t"):
            p0, p1, p2 = sp["heads"]
            assert p1 * p2 == n
            nb_img = (M + p0 - 1) // p0
            out = torch.full((nb_img * p2 * p1 * p0 + 64,), SENT, dtype=dtype, device=dev)
            kw.update(mode=kn.OUT_HEADS_T if mode == "heads_t" else kn.OUT_HEADS, p0=p0, p1=p1, p2=p2)
            idx = index_heads(M, n, p0, p1, p2, mode == "heads_t", dev)
        else:
            hp, wp = sp["tok"]
            deconv = mode == "deconv"
            co = n // 4 if deconv else n
            ldo = co + 8
            oro = 3
            img_rows = (4 if deconv else 1) * hp * wp + oro + 2
            obs = img_rows * ldo
            nimg = M // (hp * wp)
            out = torch.full((nimg * obs + 64,), SENT, dtype=dtype, device=dev)
            kw.update(mode=kn.OUT_DECONV2x2 if deconv else kn.OUT_TOKMAP, ldo=ldo, in_tok=kn.tok_layout(False, hp, wp, 0),
                      out_tok=kn.tok_layout(False, (2 if deconv else 1) * hp, (2 if deconv else 1) * wp, 0), out_batch_stride=obs,
                      out_row_offset=oro, p0=co if deconv else 0)
            idx = index_tokmap(M, n, hp, wp, ldo, obs, oro, dev, co if deconv else 0)
        out2 = None
        if sp.get("out2"):
            ld2 = n + 16
            out2 = torch.full((M + 2, ld2), SENT, dtype=dtype, device=dev)
            kw.update(out2=out2[:, 8:], ld2=ld2)
        y, bnd = epilogue64(acc[:, nb:nb + n], s_abs[:, nb:nb + n], dtype=dtype, K=K, bias=bias, act=act, scale=scale, gamma=gamma,
                            res=res, rowmask=rowmask.bool() if rowmask is not None else None, rowmask_after=bool(rm))
        cseg.append(kn.seg(out, nb, nb + n, **kw))
        keep.append(kw)                                          # (seg() keeps only its padded vectors: residual, mask, out2 live here)
        checks.append((out, idx, y, bnd, out.clone(), f"segment {i} ({mode})"))
        if out2 is not None:
            checks.append((out2, index_linear(M, n, ld2, dev) + 8, y, bnd, out2.clone(), f"segment {i} out2"))
        nb += n
    Wl = kn.pack_frag16(W) if entry == "few" and N % 16 == 0 else W      # (N % 16 != 0: a refusal case, the weights are never read)
    op = _entry(entry)(A, Wl, M, N, K, cseg, keep=(A, W, keep), splitk=0, **op_kw)
    from lwdetr_amd import _native
    lib = _native.lib()
    if expect_rc:
        before = _native.gemm_path_counts()
        rc = op._fn(op._ref, op.dtype, _native.stream_ptr())
        torch.cuda.synchronize()
        assert rc == expect_rc, (rc, expect_rc)
        assert _native.gemm_path_counts() == before
        for buf, _, _, _, snap, _ in checks:
            assert torch.equal(buf, snap), "a refused launch wrote its output"
        return
    if force is not None:
        force(lib)
    try:
        with served_by(family):
            op()
    finally:
        lib.lwdetr_gemm_tuning(-1)
        lib.lwdetr_gemm_pt_tuning(-1)
    worst = 0.0
    for buf, idx, y, bnd, snap, what in checks:
        exp, b = expected(snap, idx, y, bnd)
        ok, w, nbad = compare(buf, exp, b)
        worst = max(worst, w)
        if not ok:
            d = (buf.double().flatten() - exp).abs()
            i = int(torch.argmax(torch.where(d <= b, torch.zeros_like(d), d / b.clamp_min(1e-300))))
            pytest.fail(f"{family} {dtype} {what}: {nbad} elements out of bound; worst at flat {i} (of {buf.numel()}, row length "
                        f"{buf.shape[-1]}): got {buf.flatten()[i].item()} "
                        f"expected {exp[i].item()} bound {b[i].item()}")
    key = (family, str(dtype).split(".")[-1])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    return worst


def _knobs(**kv):
    def f(lib):
        from lwdetr_amd import _native
        for k, v in kv.items():
            _native.tuning_set(k, v)
    return f


@pytest.fixture(autouse=True)
def _clear_knobs():
    yield
    from lwdetr_amd import _native
    if torch.cuda.is_available():
        for k in ("GEMM_DMA", "GEMM_NST", "GEMM_KB", "GEMM_TILE", "CONV_PATCH", "GEMM_BIG_2WG", "GEMM_FEW_WAVES"):
            _native.tuning_set(k, None)
        _native.lib().lwdetr_gemm_tuning(-1)
        _native.lib().lwdetr_gemm_pt_tuning(-1)


def _big(mode):
    return lambda lib: lib.lwdetr_gemm_tuning(mode)


def _pt(lib):
    lib.lwdetr_gemm_pt_tuning(2)


FULL = dict(bias=True, act=GELU, scale=0.75, gamma=True, res="sep", out2=True)
ROWS = [1, 15, 17, 63, 65, 255, 257, 1000]
D16 = [F16, BF16]


def _segs3(b1, b2, n, **kw):
    return [dict(n=b1, bias=True, **kw), dict(n=b2 - b1, act=RELU, scale=0.5, **kw), dict(n=n - b2, bias=True, act=SILU, **kw)]


# family, dtypes, M, K, segs, extra run_case arguments
CASES = []
for m in ROWS:
    CASES += [("gemm_dma_64x64_d3", D16, m, 64, [dict(n=96, **FULL)], {}),
              ("gemm_kernel_64x64", [F32], m, 64, [dict(n=96, **FULL)], {}),
              ("gemm_few_plain", D16, m, 64, [dict(n=96, **FULL)], dict(entry="few"))]
CASES += [
    # the 64 x 64 ring kernel: depths, 64-deep stages, epilogue features, segments, column tails, the shortest K
    ("gemm_dma_64x64_d3", D16, 300, 32, [dict(n=91, bias=True, act=SILU)], {}),
    ("gemm_dma_64x64_d3", D16, 257, 64, [dict(n=4, bias=True, act=RELU, res="sep")], {}),
    ("gemm_dma_64x64_d3", D16, 300, 96, _segs3(64, 192, 250), {}),
    ("gemm_dma_64x64_d3", D16, 300, 96, _segs3(128, 384, 450, gamma=True), {}),
    ("gemm_dma_64x64_d3", D16, 200, 64, [dict(n=80, bias=True, res="inplace", gamma=True, scale=2.0)], {}),
    ("gemm_dma_64x64_d3", D16, 200, 64, [dict(n=80, bias=True, res="sep", res_mod=37)], {}),
    ("gemm_dma_64x64_d3", D16, 190, 64, [dict(n=72, bias=True, act=RELU, rowmask=0, res="sep")], {}),
    ("gemm_dma_64x64_d3", D16, 190, 64, [dict(n=72, bias=True, act=GELU, rowmask=1, res="sep", out2=True)], {}),
    ("gemm_dma_64x64_d3", D16, 3 * 100, 64, [dict(n=64, mode="heads", heads=(100, 16, 4), bias=True, scale=0.37),
                                             dict(n=64, mode="heads", heads=(100, 16, 4)),
                                             dict(n=64, mode="heads_t", heads=(100, 16, 4), bias=True, act=GELU)], {}),
    ("gemm_dma_64x64_d3", D16, 2 * 7 * 9, 64, [dict(n=40, mode="tokmap", tok=(7, 9), bias=True, act=SILU)], {}),
    ("gemm_dma_64x64_d3", D16, 2 * 7 * 9, 64, [dict(n=4 * 24, mode="deconv", tok=(7, 9), bias=True)], {}),
    ("gemm_dma_64x64_d2", D16, 257, 96, [dict(n=130, **FULL)], dict(force=_knobs(GEMM_NST=2))),
    ("gemm_dma_64x64_d4", D16, 257, 96, [dict(n=130, **FULL)], dict(force=_knobs(GEMM_NST=4))),
    ("gemm_dma_64x64_d3_kb64", D16, 257, 128, [dict(n=130, **FULL)], dict(force=_knobs(GEMM_KB=64))),
    ("gemm_dma_64x64_d3_kb64", D16, 65, 64, _segs3(64, 192, 250), dict(force=_knobs(GEMM_KB=64))),
    # the 128-row ring tiles
    ("gemm_dma_128x64", D16, 257, 64, _segs3(64, 192, 250), dict(force=_knobs(GEMM_TILE=2))),
    ("gemm_dma_128x64", D16, 1000, 32, [dict(n=91, **FULL)], dict(force=_knobs(GEMM_TILE=2))),
    ("gemm_dma_128x128_d3", D16, 257, 64, _segs3(128, 384, 450, res="sep"), dict(force=_knobs(GEMM_TILE=3))),
    ("gemm_dma_128x128_d3", D16, 130, 64, [dict(n=200, **FULL)], dict(force=_knobs(GEMM_TILE=3))),
    ("gemm_dma_128x128_d4", D16, 257, 64, [dict(n=200, **FULL)], dict(force=_knobs(GEMM_TILE=3, GEMM_DMA=4))),
    ("gemm_dma_128x128_d3", D16, 2 * 8 * 10, 9 * 64, [dict(n=130, bias=True, act=SILU, res="sep")], dict(conv=(2, 8, 10, 64, 1, 32, 160),
                                                                                                        force=_knobs(GEMM_TILE=3))),
    # gemm_kernel (no DMA): f32, the A + A2 operand sum, GEMM_DMA = 0
    ("gemm_kernel_64x64", [F32], 300, 32, [dict(n=91, bias=True, act=SILU)], {}),
    ("gemm_kernel_64x64", [F32], 257, 64, _segs3(64, 192, 250), {}),
    ("gemm_kernel_64x64", [F32], 190, 64, [dict(n=72, bias=True, act=RELU, rowmask=0, res="sep")], {}),
    ("gemm_kernel_64x64", [F32], 3 * 100, 64, [dict(n=64, mode="heads", heads=(100, 16, 4), bias=True),
                                               dict(n=64, mode="heads_t", heads=(100, 16, 4), bias=True, act=GELU)], {}),
    ("gemm_kernel_128x64", [F32], 257, 64, [dict(n=130, **FULL)], dict(force=_knobs(GEMM_TILE=2))),
    ("gemm_kernel_64x64", D16, 257, 64, [dict(n=130, **FULL)], dict(a2=True)),
    ("gemm_kernel_64x64", D16, 300, 64, _segs3(64, 192, 250, res="sep"), dict(a2=True)),
    ("gemm_kernel_64x64", D16, 190, 64, [dict(n=72, bias=True, rowmask=1, res="sep")], dict(a2=True)),
    ("gemm_kernel_64x64", D16, 257, 32, [dict(n=91, **FULL)], dict(force=_knobs(GEMM_DMA=0))),
    ("gemm_kernel_128x64", D16, 257, 64, [dict(n=130, **FULL)], dict(force=_knobs(GEMM_DMA=0, GEMM_TILE=2))),
    ("gemm_kernel_128x128", D16, 257, 64, [dict(n=200, **FULL)], dict(force=_knobs(GEMM_DMA=0, GEMM_TILE=3))),
    # the patch-resident 3x3 convolution (N = Cin = 128, stride 1, raster rows; images straddle 128-pixel tiles)
    ("conv3x3_patch_128", D16, 3 * 10 * 13, 9 * 128, [dict(n=128, bias=True, act=SILU, res="sep", out2=True)],
     dict(conv=(3, 10, 13, 128, 1, 64, 320), force=_knobs(CONV_PATCH=2))),
    # the 256-row large-tile kernel: column tiles 256 / 192 / 128, stage depths 64 / 32
    ("gemm_big_256_kb64", D16, 300, 64, [dict(n=512, **FULL)], dict(force=_big(2))),
    ("gemm_big_256_kb64", D16, 257, 128, [dict(n=256, bias=True), dict(n=600 - 256, bias=True, act=SILU, res="sep")], dict(force=_big(2))),
    ("gemm_big_256_kb32", D16, 300, 128, [dict(n=512, **FULL)], dict(force=_big(32))),
    ("gemm_big_192_kb64", D16, 257, 64, [dict(n=150, **FULL)], dict(force=_big(2))),
    ("gemm_big_128_kb64", D16, 300, 64, _segs3(128, 256, 450, res="sep"), dict(force=_big(2))),
    ("gemm_big_128_kb64", D16, 257, 64, [dict(n=384, bias=True, act=RELU, rowmask=0, res="sep"), dict(n=64, rowmask=1, bias=True)],
     dict(force=_big(2))),
    ("gemm_big_128_kb32", D16, 300, 64, [dict(n=384, **FULL)], dict(force=_big(32))),
    ("gemm_big_256_kb64", D16, 3 * 100, 64, [dict(n=256, mode="heads", heads=(100, 64, 4), bias=True, scale=0.37),
                                             dict(n=256, mode="heads_t", heads=(100, 64, 4), bias=True)], dict(force=_big(2))),
    ("gemm_big_192_kb64", D16, 2 * 8 * 10, 9 * 64, [dict(n=192, bias=True, act=SILU)], dict(conv=(2, 8, 10, 64, 1, 32, 160), force=_big(2))),
    # the 4-wave form asked for by name is not in the default build: the 8-wave kernel serves it (an experiments build: the 4-wave form)
    ("big4_or_256", D16, 300, 64, [dict(n=512, **FULL)], dict(force=_big(128))),
    ("big4_or_256", D16, 300, 64, [dict(n=512, **FULL)], dict(force=lambda lib: (lib.lwdetr_gemm_tuning(2), _knobs(GEMM_BIG_2WG=2)(lib)))),
    # the persistent kernel (forced: by default >= 16384 rows)
    ("gemm_pt", D16, 512, 128, [dict(n=1024, bias=True, act=GELU, scale=0.75, gamma=True, res="sep")], dict(force=_pt)),
    ("gemm_pt", D16, 1000, 128, [dict(n=256, bias=True, act=SILU), dict(n=768, bias=True, res="inplace", out2=True)], dict(force=_pt)),
    ("gemm_pt", D16, 2 * 520, 128, [dict(n=256, mode="heads", heads=(520, 64, 4), bias=True, scale=0.37),
                                    dict(n=256, mode="heads", heads=(520, 64, 4)),
                                    dict(n=256, mode="heads_t", heads=(520, 64, 4), bias=True)], dict(force=_pt)),
    # the short row tails of the 128- and 256-row tiles (1, 17, 65 rows: one partial tile) and of the persistent kernel (264 = 256 + 8)
    *[("gemm_dma_128x64", D16, m, 64, [dict(n=130, **FULL)], dict(force=_knobs(GEMM_TILE=2))) for m in (1, 17, 65)],
    *[("gemm_dma_128x128_d3", D16, m, 64, [dict(n=200, **FULL)], dict(force=_knobs(GEMM_TILE=3))) for m in (1, 65)],
    *[("gemm_dma_64x64_d2", D16, m, 96, [dict(n=130, **FULL)], dict(force=_knobs(GEMM_NST=2))) for m in (1, 17)],
    *[("gemm_dma_64x64_d4", D16, m, 96, [dict(n=130, **FULL)], dict(force=_knobs(GEMM_NST=4))) for m in (1, 17)],
    *[("gemm_dma_64x64_d3_kb64", D16, m, 128, [dict(n=130, **FULL)], dict(force=_knobs(GEMM_KB=64))) for m in (1, 17)],
    ("gemm_kernel_128x64", [F32], 17, 64, [dict(n=130, **FULL)], dict(force=_knobs(GEMM_TILE=2))),
    *[("gemm_big_256_kb64", D16, m, 64, [dict(n=512, **FULL)], dict(force=_big(2))) for m in (1, 17, 65)],
    ("gemm_big_192_kb64", D16, 17, 64, [dict(n=150, **FULL)], dict(force=_big(2))),
    ("gemm_big_128_kb64", D16, 65, 64, [dict(n=384, **FULL)], dict(force=_big(2))),
    ("gemm_pt", D16, 264, 128, [dict(n=1024, bias=True, act=SILU, res="sep", out2=True)], dict(force=_pt)),
    # the persistent kernel refuses a row mask: the launch moves to the large-tile kernel
    ("gemm_big_256_kb64", D16, 512, 128, [dict(n=1024, bias=True, rowmask=1)], dict(force=lambda lib: (_pt(lib), lib.lwdetr_gemm_tuning(2)))),
    # the few-row kernel: PLAIN, CONV with 4 / 6 chunks per batch
    ("gemm_few_plain", D16, 257, 32, [dict(n=16, bias=True, act=RELU)], dict(entry="few")),
    ("gemm_few_plain", D16, 300, 256, [dict(n=256, bias=True, act=SILU, res="inplace", gamma=True)], dict(entry="few")),
    ("gemm_few_conv_kch4", D16, 1 * 12 * 11, 9 * 128, [dict(n=96, **FULL)], dict(entry="few", conv=(1, 12, 11, 128, 1, 32, 224))),
    ("gemm_few_conv_kch4", D16, 2 * 6 * 6, 9 * 128, [dict(n=64, bias=True, act=GELU)], dict(entry="few", conv=(2, 11, 12, 128, 2, 0, 128))),
    ("gemm_few_conv_kch6", D16, 1 * 9 * 10, 9 * 192, [dict(n=192, bias=True, act=SILU, res="sep")], dict(entry="few", conv=(1, 9, 10, 192, 1, 64, 320))),
]


def _case_id(c):
    fam, _, m, k, segs, extra = c
    what = "+".join(sorted({s.get("mode", "lin") for s in segs})) + f"-s{len(segs)}"
    return f"{fam}-M{m}-K{k}-N{sum(s['n'] for s in segs)}-{what}" + ("-a2" if extra.get("a2") else "")


PARAMS = [pytest.param(c, dt, id=f"{_case_id(c)}-{str(dt).split('.')[-1]}") for c in CASES for dt in c[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("case,dtype", PARAMS)
def test_gemm_family_vs_fp64(case, dtype):
    family, _, M, K, segs, extra = case
    if family == "big4_or_256":
        from lwdetr_amd import _native
        family = "gemm_big4_256" if _native.lib().lwdetr_has_experiments() else "gemm_big_256_kb64"
    run_case(family, dtype, M, K, segs, **extra)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", D16)
def test_gemm_few_refusals(dtype):
    """lwdetr_gemm_few answers LWDETR_ERR_UNSUPPORTED (before any launch; nothing written, nothing counted) for what its kernel does not do:
    a row mask, a column tail (N % 16), columns past N, and - host-side check only, nothing is launched - a residual / second destination off
    8-byte alignment and a bias / LayerScale vector off 16-byte alignment."""
    from lwdetr_amd import _native, kernels as K
    UNS = _native.ERR_UNSUPPORTED
    run_case(None, dtype, 64, 64, [dict(n=32, bias=True, rowmask=0)], entry="few", expect_rc=UNS)
    run_case(None, dtype, 64, 64, [dict(n=91, bias=True)], entry="few", expect_rc=UNS)
    dev = _dev()
    a, w = _rand((64, 64), dtype, 1), K.pack_frag16(_rand((32, 64), dtype, 2))
    out = torch.full((64, 48), SENT, dtype=dtype, device=dev)
    snap = out.clone()
    store = torch.zeros(64 * 48 + 16, dtype=dtype, device=dev)
    vec = torch.zeros(64, dtype=torch.float32, device=dev)

    def refused(**kw):
        op = K.GemmFewOp(a, w, 64, 32, 64, [K.seg(out, 0, kw.pop("n_end", 32), ldo=48, **kw)], keep=(out, store, vec))
        before = _native.gemm_path_counts()
        rc = op._fn(op._ref, op.dtype, _native.stream_ptr())
        torch.cuda.synchronize()
        return rc == UNS and _native.gemm_path_counts() == before and torch.equal(out, snap)

    assert refused(n_end=48)                                           # columns past N
    assert refused(res=store[1:], ldres=48)                            # residual at a 2-byte offset
    assert refused(out2=store[2:], ld2=48)                             # second destination at a 4-byte offset
    s = K.seg(out, 0, 32, ldo=48)
    for field in ("bias", "gamma"):                                    # 16-byte loads of the vectors: an 8-byte offset is refused
        op = K.GemmFewOp(a, w, 64, 32, 64, [s], keep=(out, vec))
        setattr(op.desc.seg[0], field, vec.data_ptr() + 8)
        before = _native.gemm_path_counts()
        assert op._fn(op._ref, op.dtype, _native.stream_ptr()) == UNS and _native.gemm_path_counts() == before
    torch.cuda.synchronize()
    assert torch.equal(out, snap)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["gemm", "few"])
def test_unknown_activation_is_refused(entry):
    """act outside {NONE, RELU, GELU, SILU}: the kernels used to disagree (ReLU in some, identity in others); both entries refuse it now."""
    from lwdetr_amd import _native
    for act in (4, -1, 7):
        run_case(None, F16, 100, 64, [dict(n=64, bias=True, act=act)], entry=entry, expect_rc=_native.ERR_BAD_ARG)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", D16)
def test_gemm_op_few_route_mirrors_the_entry(dtype):
    """GemmOp's automatic few-row route takes only what lwdetr_gemm_few takes: a residual with ldres = N + 2 (4-byte rows) stays on the 64 x 64
    ring kernel, which serves it on its element-wise path (it used to be routed to the few entry, which refused it: the op raised); with
    ldres = N the few-row kernel serves it. Both against float64."""
    from lwdetr_amd import kernels as K
    M, N, Kd = 300, 256, 256
    dev = _dev()
    a, w = _rand((M, Kd), dtype, 1), _rand((N, Kd), dtype, 2, Kd ** -0.5)
    bias = _rand((N,), F32, 3)
    acc, s = _products(a, w)
    for ldres, family in ((N + 2, "gemm_dma_64x64_d3"), (N, "gemm_few_plain")):
        res = _rand((M, ldres), dtype, 4)
        out = torch.full((M + 2, N), SENT, dtype=dtype, device=dev)
        snap = out.clone()
        op = K.GemmOp(a, w, M, N, Kd, [K.seg(out, 0, N, ldo=N, bias=bias, act=GELU, res=res, ldres=ldres)], keep=(out, res))
        with served_by(family):
            op()
        y, bnd = epilogue64(acc, s, dtype=dtype, K=Kd, bias=bias, act=GELU, res=res[:, :N])
        exp, b = expected(snap, index_linear(M, N, N, dev), y, bnd)
        ok, worst, nbad = compare(out, exp, b)
        assert ok, (family, nbad, worst)
        key = (family + " (GemmOp route)", str(dtype).split(".")[-1])
        WORST[key] = max(WORST.get(key, 0.0), worst)


def teardown_module(module):
    if WORST:
        print("\nlargest err / bound per family and dtype:")
        for (fam, dt), w in sorted(WORST.items()):
            print(f"  {fam:34s} {dt:9s} {w:.3f}")
