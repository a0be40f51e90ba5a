"""Every entry point of csrc/rowops.hip, called directly and checked ELEMENT BY ELEMENT against float64 arithmetic on the operands as stored:
the LayerNorm family (lwdetr_layernorm, _chain, lwdetr_row_stats, lwdetr_ffn_finish) and the glue of the two-stage selection
(lwdetr_select_gather, lwdetr_decoder_inputs, lwdetr_box_reparam, lwdetr_finalize_outputs). Every output buffer carries guard rows before
and after (and guard columns where ld > C) filled with a sentinel that must come back bit-identical.

LayerNorm bound. u = 2^-24 is the unit roundoff of f32, m = mean|x| of the row, d_i = x_i - mean, rstd = 1 / sqrt(var + eps), and
n_add = (16-byte chunks per lane) * (elements per chunk) + 4 is the number of f32 additions on the longest path of one row reduction
(lane 0's serial adds, then the 4 shuffle steps over the 16 lanes of the row). The kernel computes, all in f32,
    mean^ = fl(S^ / C),  |S^ - S| <= n_add u sum|x|            =>  |delta| := |mean^ - mean| <= (n_add + 1) u m
    d^_i  = fl(x_i - mean^) = (d_i - delta)(1 + e),  |e| <= u
    C var^ = (sum d_i^2 + C delta^2)(1 + t),  |t| <= (n_add + 3) u    (sum d_i = 0: the common shift delta enters the variance only squared)
    rstd^ = rstd (1 + r) / sqrt(1 + delta^2 rstd^2),  |r| <= (n_add / 2 + 4) u     (/ C, + eps, sqrt, 1 / .: half or one u each)
    y^_i  = fl(fl(fl(d^_i rstd^) gamma_i) + beta_i)                      (3 more roundings, the last one relative to |y|)
so to first order, with |d_i| <= |x_i| + m and m rstd <= A_i := (|x_i| + m) rstd,
    |y^_i - y_i| <= u [ (n_add / 2 + 8) |d_i| rstd |gamma_i| + (n_add + 1) m rstd |gamma_i| + |y_i| ]
                 <= u (1.5 n_add + 10) A_i |gamma_i| + u |beta_i|
                 <= 2^-23 (n_add + C_LN) (A_i |gamma_i| + |beta_i|) =: E_i          with C_LN = 5 for the first order; C_LN = 6 is used:
the extra unit (>= 2 u A_i |gamma_i|) covers the second-order terms. The only one that is not O(u^2) is the delta^2 rstd^2 inside rstd^ on a
row whose spread is a few ulp of its mean (the large-mean rows below, in f32): there |d_i| rstd (1 - 1 / sqrt(1 + T^2)) <= |d_i| rstd T / sqrt(2)
with T = |delta| rstd, and these rows are built with |d_i| rstd <= 4, so the term stays below 3 (n_add + 1) u m rstd |gamma_i| < E_i / 2 while the
first-order terms of such a row (d exact by Sterbenz, |d_i| << m) use less than the other half. The stored result is the rounding of y^_i to
the output dtype: half an ulp of that dtype at |y_i| (taken at |y_i| + E_i, which differs only when y^ may sit in the next binade).
Total bound: half_ulp_T(|y_i| + E_i) + E_i. lwdetr_row_stats: |mean^ - mean| <= 2^-23 (n_add + C_LN) m and
|rstd^ - rstd| <= rstd (2^-23 (n_add + C_LN) + 1 - 1 / sqrt(1 + T_max^2)), T_max = 2^-23 (n_add + C_LN) m rstd, each plus half an f32 ulp.

Box bound (lwdetr_decoder_inputs, lwdetr_box_reparam, lwdetr_finalize_outputs), from the kernels' expressions:
    xy = d * w + c  : u |d w| for the product, u |xy| <= u (|d w| + |c|) for the sum (fused: the latter only)   E <= u (2 |d w| + |c|) <= 2^-23 (|d w| + |c|)
    wh = expf(d) * w: expf to 1 ulp (2 u), one product rounding (u)                      E <= 3 u |wh|                        <= 2^-23 * 2 |wh|
and for the second re-parameterisation, whose reference operand is the computed first one (errors E1):
    xy2 = r * wh1 + xy1 : E <= |r| E1_wh + E1_xy + 2^-23 (|r wh1| + |xy1|)
    wh2 = expf(r) * wh1 : E <= 3 u |wh2| + expf(r) E1_wh (<= 3 u |wh2|)                                                 <= 2^-23 * 4 |wh2|
plus half an ulp of the output dtype (ref_out is f32).

Sine bound: half an ulp of the output dtype at 1, plus 2^-21 |e| for the argument e = pos * 2 pi / dim_t as the kernel forms it (the f32 value of
2 pi, one product, one quotient and the error of the reference box behind pos), plus SIN_INTRINSIC for the hardware sine / cosine, measured (below).
"""
import functools
import math

import numpy as np
import pytest
import torch

from lwdetr_amd import _native
from oracle import lwdetr_torch as O

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = [F32, F16, BF16]
D16 = [F16, BF16]
P = {F16: 11, BF16: 8, F32: 24}               # significand bits (with the hidden one): half an ulp of v in [2^e, 2^(e+1)) is 2^(e - P)
EMIN = {F16: -14, BF16: -126, F32: -126}      # below 2^EMIN the spacing stays that of the smallest normal binade
EPC = {F16: 8, BF16: 8, F32: 4}               # elements per 16-byte chunk
U23 = 2.0 ** -23
C_LN = 6                                      # derivation in the module docstring
# Largest |sine(f32 run) - sine(float64 reference)| over the three input sets of test_rowops_decoder_inputs_vs_fp64, measured on an MI355X (the raw
# deviation from the float64 reference, argument error included; that test prints it as "sine f32 max deviation"): 1.754e-06 (1x1x256),
# 3.714e-06 (2x7x256), 3.595e-06 (2x300x384). Margin 4: another valid input set moves the figure by that much.
SIN_MEASURED = 3.714e-06
SIN_INTRINSIC = 4 * SIN_MEASURED
SENT = 1234.0                                 # guard value of every output buffer; 7777 marks input padding that must never be copied
PADV = 7777.0
BAD_ARG, UNSUPPORTED = _native.ERR_BAD_ARG, _native.ERR_UNSUPPORTED
WORST = {}                                    # label -> largest err / bound seen (printed at the end of the module)


def _name(dt):
    return str(dt).split(".")[-1]


def _has_pad(t):
    """Does t hold the input-padding value (as rounded to t's dtype)?"""
    return bool((t.cpu() == torch.tensor(PADV).to(t.dtype)).any())


# ---------------------------------------------------------------------------------------------------------------- bounds and comparison
def half_ulp(v, dtype):
    """Half the spacing of `dtype` at |v| (float64 tensor)."""
    _, e = torch.frexp(v.abs().double())                       # |v| = m 2^e, m in [0.5, 1): floor(log2 |v|) = e - 1
    e = (e - 1).clamp_min(EMIN[dtype])
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - P[dtype])


def compare(got, exp, bnd, label=None):
    """(ok, worst err / bound, failing elements); bound 0 = must be the same number (a guard: bit-identical to the sentinel). NaN fails."""
    d = (got.double().flatten() - exp.double().flatten()).abs()
    b = bnd.double().flatten()
    bad = ~(d <= b)
    pos = b > 0
    worst = float((d[pos] / b[pos]).max()) if bool(pos.any()) else 0.0
    if label is not None and worst == worst:
        WORST[label] = max(WORST.get(label, 0.0), worst)
    return not bool(bad.any()), worst, int(bad.sum())


def assert_close(got, exp, bnd, label):
    ok, worst, nbad = compare(got, exp, bnd, label)
    print(f"{label}: worst err/bound {worst:.3f}")
    assert ok, f"{label}: {nbad} elements outside their bound, worst err/bound {worst:.3f}"


def n_add(C, dtype):
    return -(-C // (16 * EPC[dtype])) * EPC[dtype] + 4


def ln_reference(x, gamma, beta, eps, dtype):
    """float64 LayerNorm of the stored x (M, C) and the element bound for an output of `dtype`; also mean, rstd and their bounds."""
    x = x.double()
    C = x.shape[1]
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + float(np.float32(eps)))
    y = d * rstd * gamma.double() + beta.double()
    m = x.abs().mean(1, keepdim=True)
    k = U23 * (n_add(C, dtype) + C_LN)
    E = k * ((x.abs() + m) * rstd * gamma.double().abs() + beta.double().abs())
    bnd = half_ulp(y.abs() + E, dtype) + E
    e_mean = k * m
    t = k * m * rstd
    e_rstd = rstd * (k + 1 - 1 / torch.sqrt(1 + t * t))
    stats = dict(mean=mean[:, 0], rstd=rstd[:, 0], mean_bnd=(e_mean + half_ulp(mean.abs() + e_mean, F32))[:, 0],
                 rstd_bnd=(e_rstd + half_ulp(rstd + e_rstd, F32))[:, 0])
    return y, bnd, stats


def ln2_propagated(out1_ref, bnd1, gamma2, beta2, eps2, dtype):
    """float64 LN2 of the float64 out1 and the bound of the kernel's out2 against it: the LayerNorm bound of LN2 on the stored out1, plus the
    first-order change of LN2 under a perturbation |dx_i| <= bnd1_i of its input, dy_i = gamma_i rstd (dx_i - mean(dx) - z_i mean(z dx)) with
    z = d rstd, so |dy_i| <= |gamma_i| rstd (bnd1_i + mean(bnd1) + |z_i| mean(|z| bnd1)); 1 % on top for the second order (bnd1 / |x| <= 2^-8)."""
    y, bnd, _ = ln_reference(out1_ref, gamma2, beta2, eps2, dtype)
    x = out1_ref.double()
    d = x - x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + float(np.float32(eps2)))
    z = d * rstd
    prop = gamma2.double().abs() * rstd * (bnd1 + bnd1.mean(1, keepdim=True) + z.abs() * (z.abs() * bnd1).mean(1, keepdim=True))
    return y, bnd + 1.01 * prop


def reparam_reference(delta, ref, dtype):
    """float64 oracle reparam (oracle/lwdetr_torch.py) of the stored delta (R, 4) on ref (R, 4), and the bound for an output of `dtype`."""
    dl, rf = delta.double(), ref.double()
    y = O.reparam(dl, rf)
    E = torch.cat([U23 * ((dl[:, :2] * rf[:, 2:]).abs() + rf[:, :2].abs()), U23 * 2 * y[:, 2:].abs()], 1)
    return y, E, half_ulp(y.abs() + E, dtype) + E


def decoder_reference(enc_delta, props_sel, refpoint, vr, dim_t, B, nq, d, dtype, vr_level=0):
    """float64: enc boxes, reference boxes and the sine embedding of ref * valid_ratio[level 0], with their element bounds."""
    ts, E1, ts_bnd = reparam_reference(enc_delta, props_sel, dtype)
    rp = refpoint.double().repeat(B, 1)
    rf = O.reparam(rp, ts)
    E2 = torch.cat([rp[:, :2].abs() * E1[:, 2:] + E1[:, :2] + U23 * ((rp[:, :2] * ts[:, 2:]).abs() + ts[:, :2].abs()),
                    U23 * 4 * rf[:, 2:].abs()], 1)
    rf_bnd = half_ulp(rf.abs() + E2, F32) + E2
    v = vr.double()[:, vr_level, :]                                                  # (B, 2) = (x, y)
    pos = rf.view(B, nq, 4) * torch.cat([v, v], -1)[:, None, :]
    sine = O.sine_embed(pos, d // 2).reshape(B * nq, 2 * d)
    assert torch.equal(dim_t, (10000 ** (2 * (torch.arange(d // 2, dtype=torch.float32) // 2) / (d // 2))))     # the oracle's own dim_t
    e = (pos[:, :, [1, 0, 2, 3], None] * (2 * math.pi) / dim_t.double()).reshape(B * nq, 2 * d)
    sine_bnd = 2.0 ** -P[dtype] + 2.0 ** -21 * e.abs() + SIN_INTRINSIC
    return ts, ts_bnd, rf, rf_bnd, sine, sine_bnd


# ---------------------------------------------------------------------------------------------------------------- f32 models of the kernels (CPU self-tests)
def _round_to(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


def _row_reduce_f32(v, dtype):
    """Sum over the row in the kernel's order: chunk c belongs to lane c % 16, every lane adds its chunks' elements serially, then 4 xor-shuffle steps."""
    M, C = v.shape
    epc = EPC[dtype]
    nch = -(-C // (16 * epc))
    pad = np.zeros((M, nch * 16 * epc), dtype=np.float32)
    pad[:, :C] = v
    pad = pad.reshape(M, nch, 16, epc)
    lane = np.zeros((M, 16), dtype=np.float32)
    for i in range(nch):
        for e in range(epc):
            lane = lane + pad[:, i, :, e]
    for o in (8, 4, 2, 1):
        lane = lane + lane[:, np.arange(16) ^ o]
    return lane[:, :1]


def ln_f32_model(x, gamma, beta, eps, dtype, bug=None):
    """The LayerNorm kernel's arithmetic in numpy float32 with its rounding points; `bug` plants one of the mistakes the bound has to catch."""
    f = np.float32
    v = x.float().numpy()
    C = v.shape[1]
    g, b = gamma.numpy().astype(f), beta.numpy().astype(f)
    with np.errstate(all="ignore"):
        mean = _row_reduce_f32(v, dtype) / f(C)
        if bug == "onepass":
            var = _row_reduce_f32(v * v, dtype) / f(C) - mean * mean
        else:
            dlt = v - mean
            var = _row_reduce_f32(dlt * dlt, dtype) / f(C - 1 if bug == "unbiased" else C)
        rstd = f(1) / np.sqrt(var + f(0 if bug == "noeps" else eps))
        if bug == "gshift":
            g = np.roll(g, 1)
        y = (v - mean) * rstd * g + b
    return _round_to(y, dtype), mean[:, 0], rstd[:, 0]


def reparam_f32_model(delta, ref, dtype):
    f = np.float32
    dl, rf = delta.float().numpy(), ref.numpy().astype(f)
    y = np.concatenate([dl[:, :2] * rf[:, 2:] + rf[:, :2], np.exp(dl[:, 2:]).astype(f) * rf[:, 2:]], 1).astype(f)
    return y


def sine_f32_model(rf, vr, dim_t, B, nq, d, dtype, bug=None):
    f = np.float32
    rf = rf.reshape(B, nq, 4).astype(f)
    v = vr.numpy().astype(f)[:, 1 if bug == "level1" else 0, :]
    pos = rf * np.concatenate([v, v], -1)[:, None, :]
    order = [0, 1, 2, 3] if bug == "xywh" else [1, 0, 2, 3]
    e = (pos[:, :, order, None] * f(6.283185307179586) / dim_t.numpy().astype(f)).astype(f)          # (B, nq, 4, d/2)
    odd = (np.arange(d // 2) & 1).astype(bool)
    if bug == "swap":
        odd = ~odd
    s = np.where(odd, np.cos(e.astype(np.float64)), np.sin(e.astype(np.float64))).astype(f)
    return _round_to(s.reshape(B * nq, 2 * d), dtype)


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def ln_case(M, C, dtype, kind=None):
    """Stored x (M, C) of `dtype`, gamma / beta (f32) and the float64 reference. Rows 1, 2, 3 and the last three (where M allows) are a constant row,
    a large-mean row 100 + k ulp(100) with |k| <= 3 (k[0] = -3, k[1] = 3: |d| rstd <= 2), and a row of zeros; `kind` makes every row that kind."""
    g = torch.Generator().manual_seed(1000 * C + M)
    x = torch.randn(M, C, generator=g) * 3 + 0.5
    ulp100 = 2.0 ** (6 - (P[dtype] - 1))
    kk = torch.randint(-3, 4, (M, C), generator=g).float()
    kk[:, 0], kk[:, 1] = -3, 3
    special = {"const": torch.full((M, C), -2.75), "large": 100 + kk * ulp100, "zero": torch.zeros(M, C),
               "large_mid": 100 + kk * 2.0 ** -10}              # f32 self-test only: a spread f32 still resolves
    if kind in special:
        x = special[kind]
    elif kind is None:
        for j, name in enumerate(("const", "large", "zero")):
            for r in (1 + j, M - 1 - j):
                if 0 <= r < M and M >= 4:
                    x[r] = special[name][r]
    x = x.to(dtype)
    gamma = torch.randn(C, generator=g) * 0.5 + 1
    beta = torch.randn(C, generator=g) * 0.3
    y, bnd, stats = ln_reference(x, gamma, beta, 1e-5, dtype)
    return x, gamma, beta, y, bnd, stats


def ln_cases(C, dtype):
    """The M values of the issue; M = 1 once per row kind."""
    for M in (1, 15, 16, 17, 1003):
        for kind in ((None, "const", "large", "zero") if M == 1 else (None,)):
            yield M, kind


# chunks per lane (NCH instantiation): 16-bit 8 -> 1 (2), 136 -> 2 ragged (2), 256 -> 2, 320 -> 3, 400 -> 4, 720 -> 6, 1024 -> 8, 1200 -> 10 (12), 2048 -> 16;
# f32 4 -> 1 (2), 68 -> 2 ragged (2), 160 -> 3, 200 -> 4, 360 -> 6, 512 -> 8, 600 -> 10 (12), 1024 -> 16
LN_C = {F16: [8, 136, 256, 320, 400, 720, 1024, 1200, 2048], BF16: [8, 136, 256, 320, 400, 720, 1024, 1200, 2048],
        F32: [4, 68, 160, 200, 360, 512, 600, 1024]}
LN_C_UNSUPPORTED = {F16: 2056, BF16: 2056, F32: 1028}
LN_PARAMS = [pytest.param(dt, c, id=f"{_name(dt)}-C{c}") for dt in DTYPES for c in LN_C[dt]]


# ---------------------------------------------------------------------------------------------------------------- CPU self-tests: the bounds can fail
@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_bound_flags_each_planted_bug(dtype):
    """The bound passes a float32 LayerNorm with the kernel's reduction order and rounding points, and flags: unbiased variance, no eps (constant
    row), one-pass variance (large-mean row in f16; bf16: ulp(100) = 0.5 keeps the sums of that row exact in f32, so one pass is not wrong there;
    f32: the row's spread is a few ulp of its mean, which no f32 LayerNorm resolves - a row 100 + k 2^-10 stands in), gamma shifted by one channel."""
    C = 68 if dtype == F32 else 136
    for M, kind in ((17, None), (1, "const"), (1, "large"), (1, "zero"), (1003, None)):
        x, gamma, beta, y, bnd, st = ln_case(M, C, dtype, kind)
        out, mean, rstd = ln_f32_model(x, gamma, beta, 1e-5, dtype)
        ok, worst, nbad = compare(out, y, bnd)
        assert ok and worst <= 1.0, (M, kind, worst, nbad)
        assert compare(torch.from_numpy(mean), st["mean"], st["mean_bnd"])[0]
        assert compare(torch.from_numpy(rstd), st["rstd"], st["rstd_bnd"])[0]
    x, gamma, beta, y, bnd, st = ln_case(17, C, dtype)
    for bug in ("unbiased", "gshift"):
        out, _, rstd = ln_f32_model(x, gamma, beta, 1e-5, dtype, bug)
        assert not compare(out, y, bnd)[0], bug
    assert not compare(torch.from_numpy(ln_f32_model(x, gamma, beta, 1e-5, dtype, "unbiased")[2]), st["rstd"], st["rstd_bnd"])[0]
    x, gamma, beta, y, bnd, st = ln_case(1, C, dtype, "const")
    out, _, rstd = ln_f32_model(x, gamma, beta, 1e-5, dtype, "noeps")
    assert not compare(out, y, bnd)[0]
    assert not compare(torch.from_numpy(rstd), st["rstd"], st["rstd_bnd"])[0]
    assert float((y - beta.double()).abs().max()) < 1e-12                      # var = 0: the reference is beta
    if dtype != BF16:
        x, gamma, beta, y, bnd, st = ln_case(1, 256, dtype, "large" if dtype == F16 else "large_mid")
        assert compare(ln_f32_model(x, gamma, beta, 1e-5, dtype)[0], y, bnd)[0]
        assert not compare(ln_f32_model(x, gamma, beta, 1e-5, dtype, "onepass")[0], y, bnd)[0]


def test_layernorm_bound_is_a_few_ulp():
    """On an ordinary row the bound stays near half an ulp of the output: it cannot hide a wrong statistic."""
    x, gamma, beta, y, bnd, _ = ln_case(17, 256, F16)
    rows = [0, 4, 5, 6, 7, 8]
    big = y[rows].abs() > 0.25
    assert float((bnd[rows][big] / y[rows][big].abs()).max()) < 2 * 2.0 ** -11


def _decoder_inputs(B, nq, d, L, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * nq + d)
    n = B * nq
    # exp arguments in [-4, 1.5], and +-4 once each where the other factor is small: widths reach ~8, sine arguments ~50 rad
    enc_delta = torch.cat([torch.randn(n, 2, generator=g) * 0.5, torch.rand(n, 2, generator=g) * 5.5 - 4], 1)
    enc_delta[0, 2], enc_delta[0, 3] = 4.0, -4.0
    enc_delta = enc_delta.to(dtype)
    props = torch.cat([torch.rand(n, 2, generator=g), torch.rand(n, 2, generator=g) * 0.35 + 0.05], 1)
    refpoint = torch.cat([torch.randn(nq, 2, generator=g) * 1.5, torch.rand(nq, 2, generator=g) * 5.5 - 4], 1)
    refpoint[0, 2], refpoint[0, 3] = -4.0, 4.0
    vr = 0.5 + 0.5 * (torch.randperm(B * L * 2, generator=g).float() + 1) / (B * L * 2 + 1)      # all different: per image, per level, x != y
    vr = vr.view(B, L, 2)
    query = torch.randn(nq, d, generator=g).to(dtype)
    dim_t = (10000 ** (2 * (torch.arange(d // 2, dtype=torch.float32) // 2) / (d // 2))).contiguous()
    return enc_delta, props, refpoint, vr, query, dim_t


@pytest.mark.parametrize("dtype", DTYPES)
def test_sine_and_reparam_bounds_flag_each_planted_bug(dtype):
    """Sine embedding in (x, y, w, h) order, sin / cos swapped, level-1 valid ratios; re-parameterisation with ref row r % (ref_rows + 1); a logits copy
    with row stride ncls in place of ldc - each is flagged, the float32 model of the kernel passes."""
    B, nq, d, L = 2, 7, 256, 3
    enc_delta, props, refpoint, vr, query, dim_t = _decoder_inputs(B, nq, d, L, dtype)
    ts, ts_bnd, rf, rf_bnd, sine, sine_bnd = decoder_reference(enc_delta, props, refpoint, vr, dim_t, B, nq, d, dtype)
    ts32 = reparam_f32_model(enc_delta, props, dtype)
    assert compare(_round_to(ts32, dtype), ts, ts_bnd)[0]
    rf32 = reparam_f32_model(refpoint.repeat(B, 1), torch.from_numpy(ts32), F32)
    assert compare(torch.from_numpy(rf32), rf, rf_bnd)[0]
    assert compare(sine_f32_model(rf32, vr, dim_t, B, nq, d, dtype), sine, sine_bnd)[0]
    for bug in ("xywh", "swap", "level1"):
        assert not compare(sine_f32_model(rf32, vr, dim_t, B, nq, d, dtype, bug), sine, sine_bnd)[0], bug
    # box_reparam: reference row r % ref_rows
    ref_rows, nl = 7, 3
    delta, ref, _, _ = _final_inputs(ref_rows, 91, 96, nl, dtype)
    R = nl * ref_rows
    y, _, bnd = reparam_reference(delta, ref[torch.arange(R) % ref_rows], dtype)
    assert compare(_round_to(reparam_f32_model(delta, ref[torch.arange(R) % ref_rows], dtype), dtype), y, bnd)[0]
    ref_wrong = torch.cat([ref, ref[:1]])[torch.arange(R) % (ref_rows + 1)]
    assert not compare(_round_to(reparam_f32_model(delta, ref_wrong, dtype), dtype), y, bnd)[0]
    # logits copy: stride ncls in place of ldc reads pad columns / the wrong rows
    _, _, logits_pad, _ = _final_inputs(ref_rows, 91, 96, nl, dtype)
    good = logits_pad[:, :91]
    wrong = logits_pad.flatten()[:R * 91].view(R, 91)
    assert not torch.equal(wrong, good) and _has_pad(wrong) and not _has_pad(good)


def _final_inputs(ref_rows, ncls, ldc, nl, dtype):
    g = torch.Generator().manual_seed(ref_rows * 100 + ncls)
    R = nl * ref_rows
    delta = torch.cat([torch.randn(R, 2, generator=g) * 2, torch.rand(R, 2, generator=g) * 20 - 10], 1)
    delta[0, 2], delta[R - 1, 3] = 10.0, -10.0
    if R > 2:
        delta[1, 2], delta[R - 2, 3] = -10.0, 10.0
    delta = delta.to(dtype)
    ref = torch.cat([torch.randn(ref_rows, 2, generator=g), torch.rand(ref_rows, 2, generator=g) * 1.45 + 0.05], 1)
    logits_pad = torch.randn(R, ldc, generator=g) * 3
    logits_pad[:, ncls:] = PADV
    logits_pad = logits_pad.to(dtype)
    return delta, ref, logits_pad, R


# ---------------------------------------------------------------------------------------------------------------- GPU plumbing
def _dev():
    return torch.device("cuda:0")


class Guarded:
    """A device buffer of rows x ld elements behind `pre` and in front of `post` guard rows (or, for ld = 1 use, elements), everything filled with the
    sentinel: `ptr` is the address of row 0, `check` compares the WHOLE buffer with the expectation (guards and pad columns: bound 0)."""

    def __init__(self, rows, ld, dtype, fill=SENT, pre=2, post=2):
        self.rows, self.ld, self.dtype, self.pre = rows, ld, dtype, pre
        self.buf = torch.full(((pre + rows + post), ld), fill, dtype=dtype, device=_dev())
        self.snap = self.buf.cpu().double()
        self.ptr = self.buf.data_ptr() + pre * ld * self.buf.element_size()

    def body(self):
        return self.buf[self.pre:self.pre + self.rows]

    def load(self, t, cols=None):
        """Store t (rows', cols) into the top-left corner (an in/out buffer: x of the in-place FFN finish); the snapshot follows."""
        self.buf[self.pre:self.pre + t.shape[0], :t.shape[1]] = t.to(_dev())
        self.snap = self.buf.cpu().double()

    def check(self, label, writes):
        """writes: list of (row index tensor, n_cols, expected (len(rows), n_cols) float64, bound) - everything else must be unchanged."""
        exp, bnd = self.snap.clone(), torch.zeros_like(self.snap)
        for rows, ncol, y, b in writes:
            exp[self.pre + rows, :ncol] = y
            bnd[self.pre + rows, :ncol] = b if torch.is_tensor(b) else torch.full_like(y, b)
        assert_close(self.buf.cpu(), exp, bnd, label)

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.buf.cpu().double(), self.snap)


def _ptr(t):
    return t.data_ptr()


def _st():
    return _native.stream_ptr(_dev())


def _x_padded(x, ldx):
    """x (M, C) on the device with row stride ldx; the pad columns hold PADV (they must never be read into a result)."""
    M, C = x.shape
    xb = torch.full((M, ldx), PADV, dtype=x.dtype, device=_dev())
    xb[:, :C] = x.to(_dev())
    return xb


def _layernorm(xb, ldx, gamma, beta, out, ldo, M, C, eps, dtype, remap=(0, 0, 0), out_ptr=None, x_ptr=None):
    return _native.lib().lwdetr_layernorm(x_ptr if x_ptr is not None else _ptr(xb), ldx, _ptr(gamma), _ptr(beta),
                                          out_ptr if out_ptr is not None else out.ptr, ldo, M, C, eps, *remap, _native.dtype_code(dtype), _st())


# ---------------------------------------------------------------------------------------------------------------- 1. LayerNorm family
@pytest.mark.gpu
@pytest.mark.parametrize("padded", [False, True], ids=["tight", "ld"])
@pytest.mark.parametrize("dtype,C", LN_PARAMS)
def test_rowops_layernorm_vs_fp64(dtype, C, padded):
    """lwdetr_layernorm at every NCH instantiation (2 ... 16), ragged chunk counts, idle lanes, rows around a 16-row workgroup edge, ldx = C + 16 / ldo = C + 8."""
    ldx, ldo = (C + 16, C + 8) if padded else (C, C)
    for M, kind in ln_cases(C, dtype):
        x, gamma, beta, y, bnd, _ = ln_case(M, C, dtype, kind)
        xb = _x_padded(x, ldx)
        out = Guarded(M, ldo, dtype)
        gd, bd = gamma.to(_dev()), beta.to(_dev())
        _native.check(_layernorm(xb, ldx, gd, bd, out, ldo, M, C, 1e-5, dtype), "lwdetr_layernorm")
        out.check(f"layernorm {_name(dtype)}", [(torch.arange(M), C, y, bnd)])
        if kind == "const":                                     # variance 0: beta, up to the rounding of the output
            assert float((out.body()[:, :C].cpu().double() - beta.double()).abs().max()) <= float(half_ulp(beta.abs().max().double(), dtype)) + 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("padded", [False, True], ids=["tight", "ld"])
@pytest.mark.parametrize("dtype,C", LN_PARAMS)
def test_rowops_row_stats_vs_fp64(dtype, C, padded):
    """lwdetr_row_stats: planar (2, M) - stats[m] = mean, stats[M + m] = rstd - and nothing written past 2 M."""
    ldx = C + 16 if padded else C
    for M, kind in ln_cases(C, dtype):
        x, _, _, _, _, st = ln_case(M, C, dtype, kind)
        xb = _x_padded(x, ldx)
        stats = Guarded(2 * M, 1, F32, pre=16, post=16)
        rc = _native.lib().lwdetr_row_stats(_ptr(xb), ldx, M, C, 1e-5, stats.ptr, _native.dtype_code(dtype), _st())
        _native.check(rc, "lwdetr_row_stats")
        stats.check(f"row_stats {_name(dtype)}", [(torch.arange(M), 1, st["mean"][:, None], st["mean_bnd"][:, None]),
                                                  (M + torch.arange(M), 1, st["rstd"][:, None], st["rstd_bnd"][:, None])])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rowops_layernorm_unsupported_width_launches_nothing(dtype):
    """One chunk more than 16 lanes x 16 chunks hold: LWDETR_ERR_UNSUPPORTED from all three entries, outputs untouched."""
    C, M = LN_C_UNSUPPORTED[dtype], 17
    g = torch.Generator().manual_seed(C)
    xb = torch.randn(M, C, generator=g).to(dtype).to(_dev())
    gd, bd = torch.ones(C, device=_dev()), torch.zeros(C, device=_dev())
    out, out2, stats = Guarded(M, C, dtype), Guarded(M, C, dtype), Guarded(2 * M, 1, F32)
    code = _native.dtype_code(dtype)
    assert _layernorm(xb, C, gd, bd, out, C, M, C, 1e-5, dtype) == UNSUPPORTED
    assert _native.lib().lwdetr_layernorm_chain(_ptr(xb), C, _ptr(gd), _ptr(bd), 1e-5, out.ptr, C, _ptr(gd), _ptr(bd), 1e-5, out2.ptr, C, M, C, code, _st()) == UNSUPPORTED
    assert _native.lib().lwdetr_row_stats(_ptr(xb), C, M, C, 1e-5, stats.ptr, code, _st()) == UNSUPPORTED
    assert out.untouched() and out2.untouched() and stats.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rowops_layernorm_row_remap(dtype):
    """rows_per_batch 5, out_batch_rows 9, out_row_offset 3, B 3: the slice element-wise, every other row of the destination keeps the sentinel."""
    rpb, obr, oro, B = 5, 9, 3, 3
    M = B * rpb
    for C in (LN_C[dtype][1], 256):
        x, gamma, beta, y, bnd, _ = ln_case(M, C, dtype)
        xb = _x_padded(x, C + 16)
        out = Guarded(B * obr, C + 8, dtype)
        _native.check(_layernorm(xb, C + 16, gamma.to(_dev()), beta.to(_dev()), out, C + 8, M, C, 1e-5, dtype, remap=(rpb, obr, oro)), "lwdetr_layernorm")
        r = torch.arange(M)
        out.check(f"layernorm remap {_name(dtype)}", [((r // rpb) * obr + oro + r % rpb, C, y, bnd)])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rowops_layernorm_chain_vs_fp64(dtype):
    """out1 against float64 LN1(x); out2 against float64 LN2 of the STORED out1 (the LayerNorm bound) and against float64 LN2(LN1(x)) (that bound plus
    the propagated error of out1)."""
    for C in LN_C[dtype][:3] + LN_C[dtype][-1:]:
        for M in (17, 1003):
            x, g1, b1, y1, bnd1, _ = ln_case(M, C, dtype)
            g = torch.Generator().manual_seed(C + 5)
            g2, b2 = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.3
            xb = _x_padded(x, C + 16)
            o1, o2 = Guarded(M, C + 8, dtype), Guarded(M, C, dtype)
            dv = [t.to(_dev()) for t in (g1, b1, g2, b2)]
            rc = _native.lib().lwdetr_layernorm_chain(_ptr(xb), C + 16, _ptr(dv[0]), _ptr(dv[1]), 1e-5, o1.ptr, C + 8, _ptr(dv[2]), _ptr(dv[3]), 1e-6,
                                                      o2.ptr, C, M, C, _native.dtype_code(dtype), _st())
            _native.check(rc, "lwdetr_layernorm_chain")
            rows = torch.arange(M)
            o1.check(f"chain out1 {_name(dtype)}", [(rows, C, y1, bnd1)])
            y2s, bnd2s, _ = ln_reference(o1.body()[:, :C].cpu(), g2, b2, 1e-6, dtype)
            o2.check(f"chain out2|stored out1 {_name(dtype)}", [(rows, C, y2s, bnd2s)])
            y2, bnd2 = ln2_propagated(y1, bnd1, g2, b2, 1e-6, dtype)
            o2.check(f"chain out2 {_name(dtype)}", [(rows, C, y2, bnd2)])


# ---------------------------------------------------------------------------------------------------------------- 2. lwdetr_ffn_finish on its own
def _ffn_case(M, C, dtype):
    """x (multiples of 2^-4, |x| <= 4), b2 and 8 slabs (multiples of 2^-6, |.| <= 2): every partial sum is a multiple of 2^-6 below 32, i.e. 11
    significand bits - exact in f32 in any order. Slabs 3 ... 7 are constant over the rows, so they can be moved into b2."""
    g = torch.Generator().manual_seed(M * 7 + C)
    x = (torch.randint(-64, 65, (M, C), generator=g).float() / 16).to(dtype)
    b2 = torch.randint(-128, 129, (C,), generator=g).float() / 64
    slabs = torch.randint(-128, 129, (8, M, C), generator=g).float() / 64
    slabs[3:] = slabs[3:, :1].expand(5, M, C)
    assert torch.equal(x.float().to(dtype), x)
    g1, be1 = torch.randn(C, generator=g) * 0.2 + 1, torch.randn(C, generator=g) * 0.1
    g2, be2 = torch.randn(C, generator=g) * 0.2 + 1, torch.randn(C, generator=g) * 0.1
    return x, b2, slabs, g1, be1, g2, be2


def _ffn_pre(x, b2, slabs, dtype):
    """The pre-norm row T(x + b2 + sum of slabs): asserts that the f32 sum is exact in both orders (equal to the float64 sum), rounds it once."""
    fwd = x.float() + b2
    for s in slabs:
        fwd = fwd + s
    rev = torch.zeros_like(fwd)
    for s in reversed(slabs):
        rev = rev + s
    rev = (rev + b2) + x.float()
    exact = x.double() + b2.double() + slabs.double().sum(0)
    assert torch.equal(fwd.double(), exact) and torch.equal(rev.double(), exact)
    return fwd.to(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 17, 301])
@pytest.mark.parametrize("C", [256, 384])
@pytest.mark.parametrize("dtype", D16)
def test_rowops_ffn_finish_vs_fp64(dtype, C, M):
    """lwdetr_ffn_finish fed slabs the test wrote itself: splits 1, 3, 4, 5, 8 (the slab loop is unrolled by 4: remainders 1, 3, 0, 1, 0), in place and
    with a separate output, with and without the second LayerNorm, ldx = ldo1 = C + 8. splits 3, 4, 5 carry the remaining row-constant slabs in b2, so
    they produce the same pre-norm rows as splits 8 and must give the same bits."""
    x, b2, slabs, g1, be1, g2, be2 = _ffn_case(M, C, dtype)
    code = _native.dtype_code(dtype)
    dv = {k: v.to(_dev()) for k, v in dict(g1=g1, be1=be1, g2=g2, be2=be2).items()}
    rows = torch.arange(M)
    forms = [("inplace-ln2", True, True, C), ("separate", False, False, C), ("separate-ln2-ld", False, True, C + 8), ("inplace-ld", True, False, C + 8)]
    for name, inplace, ln2, ld in forms:
        same = {}
        for splits in (1, 3, 4, 5, 8):
            use = slabs[:splits]
            bias = b2 if splits == 1 else b2 + slabs[splits:, 0].sum(0)
            pre = _ffn_pre(x, bias, use, dtype)
            y1, bnd1, _ = ln_reference(pre, g1, be1, 1e-5, dtype)
            xg = Guarded(M, ld, dtype)
            xg.load(x)
            o1 = xg if inplace else Guarded(M, ld, dtype)
            o2 = Guarded(M, C, dtype)
            part = use.contiguous().to(_dev())
            bd = bias.to(_dev())
            rc = _native.lib().lwdetr_ffn_finish(xg.ptr, ld, _ptr(part), splits, _ptr(bd), _ptr(dv["g1"]), _ptr(dv["be1"]), 1e-5, o1.ptr, ld,
                                                 _ptr(dv["g2"]) if ln2 else None, _ptr(dv["be2"]) if ln2 else None, 1e-6,
                                                 o2.ptr if ln2 else None, C, M, C, code, _st())
            _native.check(rc, "lwdetr_ffn_finish")
            o1.check(f"ffn_finish out1 {_name(dtype)}", [(rows, C, y1, bnd1)])
            if not inplace:
                assert xg.untouched()
            got1 = o1.body()[:, :C].cpu()
            if ln2:
                y2, bnd2, _ = ln_reference(got1, g2, be2, 1e-6, dtype)
                o2.check(f"ffn_finish out2 {_name(dtype)}", [(rows, C, y2, bnd2)])
            else:
                assert o2.untouched()
            if splits >= 3:
                same[splits] = (got1, o2.body().cpu())
        for splits in (3, 4, 5):
            assert torch.equal(same[splits][0], same[8][0]) and torch.equal(same[splits][1], same[8][1]), (name, splits)


# ---------------------------------------------------------------------------------------------------------------- 3. lwdetr_select_gather
def _gather_idx(B, S, nq, g, variant=0):
    idx = torch.randint(0, S, (B, nq), generator=g)
    for b in range(B):
        fixed = [0, S - 1, (3 + b) % S, (3 + b) % S]            # first row, last row, a duplicate; different per image
        if nq == 1:
            fixed = [fixed[variant]]
        idx[b, :min(nq, 4)] = torch.tensor(fixed[:nq])
        if nq > 8:
            idx[b, -1] = idx[b, 5]
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 5, 1, 256, 1, 4), (2, 40, 7, 260, 91, 96), (3, 400, 300, 384, 366, 368)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_rowops_select_gather(dtype, shape):
    """Pure copies: rows b * S + idx[b, q] of om, enc_cls[:, :ncls] and props. Pad columns of enc_cls and unselected rows of om hold a value that must not
    appear in any output."""
    B, S, nq, d, ncls, ldc = shape
    g = torch.Generator().manual_seed(S + nq)
    for variant in ((0, 1) if nq == 1 else (0,)):
        idx = _gather_idx(B, S, nq, g, variant)
        flat = (torch.arange(B)[:, None] * S + idx).flatten()
        om = torch.randn(B * S, d, generator=g).to(dtype)
        keep = torch.zeros(B * S, dtype=torch.bool)
        keep[flat] = True
        om[~keep] = PADV
        enc_cls = torch.randn(B * S, ldc, generator=g).to(dtype)
        enc_cls[:, ncls:] = PADV
        props = torch.rand(B * S, 4, generator=g)
        n = B * nq
        om_sel, logits, props_sel = Guarded(n, d, dtype), Guarded(n, ncls, dtype), Guarded(n, 4, F32)
        omd, clsd, prd, idxd = om.to(_dev()), enc_cls.to(_dev()), props.to(_dev()), idx.to(_dev())
        rc = _native.lib().lwdetr_select_gather(_ptr(omd), _ptr(clsd), ldc, _ptr(prd), _ptr(idxd), om_sel.ptr, logits.ptr, props_sel.ptr, B, S, d, nq,
                                                ncls, _native.dtype_code(dtype), _st())
        _native.check(rc, "lwdetr_select_gather")
        rows = torch.arange(n)
        for buf, src in ((om_sel, om[flat]), (logits, enc_cls[flat, :ncls]), (props_sel, props[flat])):
            buf.check(f"select_gather {_name(dtype)}", [(rows, src.shape[1], src.double(), 0.0)])
            assert torch.equal(buf.body().cpu(), src) and not _has_pad(buf.body())


# ---------------------------------------------------------------------------------------------------------------- 4. lwdetr_decoder_inputs
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 256, 1), (2, 7, 256, 3), (2, 300, 384, 3)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_rowops_decoder_inputs_vs_fp64(dtype, shape):
    """Encoder boxes (T), decoder reference boxes (f32), all 2 d sine columns and the query broadcast, against the float64 oracle: reparam applied twice,
    sine_embed of ref * valid_ratio[level 0]."""
    B, nq, d, L = shape
    enc_delta, props, refpoint, vr, query, dim_t = _decoder_inputs(B, nq, d, L, dtype)
    ts, ts_bnd, rf, rf_bnd, sine, sine_bnd = decoder_reference(enc_delta, props, refpoint, vr, dim_t, B, nq, d, dtype)
    if nq >= 7:                                                 # the inputs do reach outside the unit square
        assert bool((rf[:, :2] < 0).any()) and bool((rf[:, :2] > 1).any()) and bool((rf[:, 2:] > 1).any()) and bool((enc_delta[:, :2] < 0).any())
    n = B * nq
    boxes, ref_out, sine_out, xdec = Guarded(n, 4, dtype), Guarded(n, 4, F32), Guarded(n, 2 * d, dtype), Guarded(n, d, dtype)
    dv = [t.to(_dev()) for t in (enc_delta, props, refpoint, vr, query, dim_t)]
    rc = _native.lib().lwdetr_decoder_inputs(_ptr(dv[0]), _ptr(dv[1]), _ptr(dv[2]), _ptr(dv[3]), L, _ptr(dv[4]), _ptr(dv[5]), boxes.ptr, ref_out.ptr,
                                             sine_out.ptr, xdec.ptr, B, nq, d, _native.dtype_code(dtype), _st())
    _native.check(rc, "lwdetr_decoder_inputs")
    rows = torch.arange(n)
    if dtype == F32:
        dev_ = float((sine_out.body().cpu().double() - sine).abs().max())
        print(f"sine f32 max deviation from float64 ({B}x{nq}x{d}): {dev_:.3e}")
    boxes.check(f"decoder_inputs enc_boxes {_name(dtype)}", [(rows, 4, ts, ts_bnd)])
    ref_out.check(f"decoder_inputs ref {_name(dtype)}", [(rows, 4, rf, rf_bnd)])
    sine_out.check(f"decoder_inputs sine {_name(dtype)}", [(rows, 2 * d, sine, sine_bnd)])
    xdec.check(f"decoder_inputs xdec {_name(dtype)}", [(rows, d, query.repeat(B, 1).double(), 0.0)])
    assert torch.equal(xdec.body().cpu(), query.repeat(B, 1))


# ---------------------------------------------------------------------------------------------------------------- 5. lwdetr_box_reparam, lwdetr_finalize_outputs
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 91, 96), (86, 3, 4)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_rowops_box_reparam_and_finalize_outputs(dtype, shape):
    """Boxes of all layers against float64 (ref row r % ref_rows), the logits as a pure copy without the pad columns, contiguous and with 5 gap rows per layer
    that both outputs must leave alone; finalize's boxes bit-identical to box_reparam's. (86, 3, 4): R = 258 and R ncls = 774 end in different 256-thread blocks."""
    ref_rows, ncls, ldc = shape
    nl = 3
    delta, ref, logits_pad, R = _final_inputs(ref_rows, ncls, ldc, nl, dtype)
    y, _, bnd = reparam_reference(delta, ref[torch.arange(R) % ref_rows], dtype)
    code = _native.dtype_code(dtype)
    dd, rd, ld_ = delta.to(_dev()), ref.to(_dev()), logits_pad.to(_dev())
    direct = Guarded(R, 4, dtype)
    _native.check(_native.lib().lwdetr_box_reparam(_ptr(dd), _ptr(rd), ref_rows, direct.ptr, R, code, _st()), "lwdetr_box_reparam")
    rows = torch.arange(R)
    direct.check(f"box_reparam {_name(dtype)}", [(rows, 4, y, bnd)])
    for olr in (0, ref_rows + 5):
        stride = olr if olr else ref_rows
        orow = (rows // ref_rows) * stride + rows % ref_rows
        coord, logits = Guarded(nl * stride, 4, dtype), Guarded(nl * stride, ncls, dtype)
        rc = _native.lib().lwdetr_finalize_outputs(_ptr(dd), _ptr(rd), ref_rows, coord.ptr, R, _ptr(ld_), ldc, ncls, logits.ptr, olr, code, _st())
        _native.check(rc, "lwdetr_finalize_outputs")
        coord.check(f"finalize boxes {_name(dtype)}", [(orow, 4, y, bnd)])
        logits.check(f"finalize logits {_name(dtype)}", [(orow, ncls, logits_pad[:, :ncls].double(), 0.0)])
        assert torch.equal(coord.body()[orow].cpu(), direct.body().cpu())
        assert torch.equal(logits.body()[orow].cpu(), logits_pad[:, :ncls]) and not _has_pad(logits.body())


# ---------------------------------------------------------------------------------------------------------------- 7. refusals (host side, nothing launched)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rowops_layernorm_refusals(dtype):
    """Valid device buffers, one offending argument each: LWDETR_ERR_BAD_ARG and the outputs keep their sentinel."""
    C, M = 256, 15
    x, gamma, beta, _, _, _ = ln_case(M, C, dtype)
    xb = _x_padded(x, C + 16)
    gd, bd = gamma.to(_dev()), beta.to(_dev())
    out, out2, stats = Guarded(3 * 9, C + 8, dtype), Guarded(M, C + 8, dtype), Guarded(2 * M, 1, F32, pre=16, post=16)
    code, esz = _native.dtype_code(dtype), xb.element_size()
    L = _native.lib()
    ln = lambda **kw: _layernorm(xb, kw.pop("ldx", C + 16), gd, bd, out, kw.pop("ldo", C + 8), M, C, 1e-5, dtype, **kw)
    chain = lambda ldx=C + 16, ldo1=C + 8, ldo2=C + 8, xp=None, o1=None, o2=None: L.lwdetr_layernorm_chain(
        xp or _ptr(xb), ldx, _ptr(gd), _ptr(bd), 1e-5, o1 or out.ptr, ldo1, _ptr(gd), _ptr(bd), 1e-6, o2 or out2.ptr, ldo2, M, C, code, _st())
    assert ln() == 0 and chain() == 0                            # the baseline call is accepted
    out, out2 = Guarded(3 * 9, C + 8, dtype), Guarded(M, C + 8, dtype)
    assert ln(ldx=C - EPC[dtype]) == BAD_ARG and ln(ldo=C - EPC[dtype]) == BAD_ARG
    assert ln(remap=(5, 4, 0)) == BAD_ARG                        # out_batch_rows < rows_per_batch
    assert ln(remap=(5, 9, -1)) == BAD_ARG                       # out_row_offset < 0
    assert ln(remap=(5, 9, 5)) == BAD_ARG                        # the slice runs into the next batch
    assert ln(remap=(5, 9, 4)) == 0                              # ... and the last offset that fits is accepted
    out = Guarded(3 * 9, C + 8, dtype)
    assert ln(x_ptr=_ptr(xb) + esz) == BAD_ARG and ln(out_ptr=out.ptr + esz) == BAD_ARG
    assert chain(ldx=C - EPC[dtype]) == BAD_ARG and chain(ldo1=C - EPC[dtype]) == BAD_ARG and chain(ldo2=C - EPC[dtype]) == BAD_ARG
    assert chain(xp=_ptr(xb) + esz) == BAD_ARG and chain(o1=out.ptr + esz) == BAD_ARG and chain(o2=out2.ptr + esz) == BAD_ARG
    rs = lambda xp=None, ldx=C + 16: L.lwdetr_row_stats(xp or _ptr(xb), ldx, M, C, 1e-5, stats.ptr, code, _st())
    assert rs(xp=_ptr(xb) + esz) == BAD_ARG and rs(ldx=C - EPC[dtype]) == BAD_ARG
    assert out.untouched() and out2.untouched() and stats.untouched()
    if dtype != F32:
        xg = Guarded(M, C, dtype)
        xg.load(x)
        part = torch.zeros(2 * M * C + 4, device=_dev())
        fin = lambda xp=None, pp=None, o1=None, o2=None, ldx=C: L.lwdetr_ffn_finish(
            xp or xg.ptr, ldx, pp or _ptr(part), 2, _ptr(bd), _ptr(gd), _ptr(bd), 1e-5, o1 or out.ptr, C + 8, _ptr(gd), _ptr(bd), 1e-6, o2 or out2.ptr, C + 8,
            M, C, code, _st())
        assert fin(xp=xg.ptr + esz) == BAD_ARG and fin(pp=_ptr(part) + 4) == BAD_ARG and fin(o1=out.ptr + esz) == BAD_ARG
        assert fin(o2=out2.ptr + esz) == BAD_ARG and fin(ldx=C - 8) == BAD_ARG
        assert out.untouched() and out2.untouched() and xg.untouched()


@pytest.mark.gpu
def test_rowops_glue_refusals():
    """lwdetr_select_gather: S, d, ncls <= 0, ldc < ncls; lwdetr_decoder_inputs: d <= 0, L <= 0; lwdetr_finalize_outputs: logits_out == logits_pad."""
    dtype, L = F16, _native.lib()
    code = _native.dtype_code(dtype)
    B, S, nq, d, ncls, ldc = 2, 40, 7, 256, 91, 96
    g = torch.Generator().manual_seed(3)
    om, cls, props = torch.randn(B * S, d, generator=g).to(dtype).to(_dev()), torch.randn(B * S, ldc, generator=g).to(dtype).to(_dev()), torch.rand(B * S, 4, generator=g).to(_dev())
    idx = _gather_idx(B, S, nq, g).to(_dev())
    n = B * nq
    om_sel, logits, props_sel = Guarded(n, d, dtype), Guarded(n, ncls, dtype), Guarded(n, 4, F32)
    sg = lambda S_=S, d_=d, ncls_=ncls, ldc_=ldc: L.lwdetr_select_gather(_ptr(om), _ptr(cls), ldc_, _ptr(props), _ptr(idx), om_sel.ptr, logits.ptr,
                                                                         props_sel.ptr, B, S_, d_, nq, ncls_, code, _st())
    for kw in (dict(S_=0), dict(S_=-1), dict(d_=0), dict(d_=-8), dict(ncls_=0), dict(ncls_=-1), dict(ldc_=ncls - 1)):
        assert sg(**kw) == BAD_ARG, kw
    assert om_sel.untouched() and logits.untouched() and props_sel.untouched()
    assert sg() == 0
    enc_delta, prs, refpoint, vr, query, dim_t = (t.to(_dev()) for t in _decoder_inputs(B, nq, d, 3, dtype))
    boxes, ref_out, sine_out, xdec = Guarded(n, 4, dtype), Guarded(n, 4, F32), Guarded(n, 2 * d, dtype), Guarded(n, d, dtype)
    di = lambda d_=d, L_=3: L.lwdetr_decoder_inputs(_ptr(enc_delta), _ptr(prs), _ptr(refpoint), _ptr(vr), L_, _ptr(query), _ptr(dim_t), boxes.ptr, ref_out.ptr,
                                                    sine_out.ptr, xdec.ptr, B, nq, d_, code, _st())
    for kw in (dict(d_=0), dict(d_=-2), dict(L_=0), dict(L_=-1)):
        assert di(**kw) == BAD_ARG, kw
    assert boxes.untouched() and ref_out.untouched() and sine_out.untouched() and xdec.untouched()
    assert di() == 0
    delta, ref, logits_pad, R = _final_inputs(7, 91, 96, 3, dtype)
    dd, rd = delta.to(_dev()), ref.to(_dev())
    pad = Guarded(R, 96, dtype)
    pad.load(logits_pad)
    coord = Guarded(R, 4, dtype)
    assert L.lwdetr_finalize_outputs(_ptr(dd), _ptr(rd), 7, coord.ptr, R, pad.ptr, 96, 91, pad.ptr, 0, code, _st()) == BAD_ARG
    assert coord.untouched() and pad.untouched()


def teardown_module(module):
    for k in sorted(WORST):
        print(f"worst err/bound  {k}: {WORST[k]:.3f}")
