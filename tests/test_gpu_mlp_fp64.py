"""The kernels of csrc/mlp.hip (lwdetr_mlp_fused, lwdetr_vit_block_few, lwdetr_ffn_partial), called straight through the C entries at the smallest
shapes at which their tile dealing, buffer-bounded stores and launch forms can go wrong, every launch pinned to ONE instantiation by the launch-form
record (lwdetr_mlp_path_counts, helpers.mlp_served_by) and every output checked ELEMENT BY ELEMENT against float64 arithmetic on the operands as
stored. Output buffers carry guard rows / guard elements / pad columns filled with a sentinel that must come back bit-identical. The machinery
(rounding, tie carrying, propagation, comparison) is that of tests/test_gpu_vitblock.py; what differs is listed here.

Rounding points (T = the storage type), read from mlp.hip. mlp_kernel, ViT mode:
  * weights as kernels.pack_mlp_weights / pack_qkv_weights store them: Wp, W1' = T(fc1 * ln2_w), W2, Wqkv' = T(Wqkv * ln1_w); f32 vectors b1' = b1 + W1
    ln2_b, bp, g1, b2, g2, bqkv' as stored;
  * x1 = T(x + g1 (att Wp^T + bp))    accumulators from ZERO, bias and LayerScale in f32 (`cvt4<T>(up4<T>(x) + gg * (accp + bb))`): no 1/gamma start value;
    without the projection x1 = x as stored;
  * z = T((x1 - mean) rstd)           two-pass f32 statistics of the ROUNDED x1 (`from_f32<T>((to_f32<T>(xf) - mean) * rstd)`);
  * h = T(gelu_for<T>(z W1'^T + b1')) accumulators start at the bias (`acc1 = bia0 / bia1`);
  * out = T(x1 + g2 (h W2^T + b2))    accumulators from zero; the tap is this number bit for bit; (mean', rstd') are those of the ROUNDED rows (eps_next);
  * z' = T((out - mean') rstd'); q = T((z' Wq'^T + bq') qscale), k = T(z' Wk'^T + bk'), v^T = T(z' Wv'^T + bv'): accumulators start at the bias.
mlp_small_kernel (both bodies: TT = 1 with its prefetch, TT = 2) and vit_block_few384_kernel round at the same points: x1 is rounded into LDS
(`cvt4<T>(up4<T>(xr) + gg * (a + bb))`), every wave normalises the rounded tile, h = T(gelu_for<T>(.)) before fc2, out = T(x1 + g2 (sum + b2)) is
written back to LDS and the statistics / z' are taken from those rounded rows. The only difference is the ORDER of the f32 additions of fc2
(mlp_small: eight per-wave partial sums of three hidden chunks each, added in wave order; few384: 48 chunks in order in one accumulator), which
the accumulation bound below covers. The f32 forms (mlp_kernel<float>, mlp_small_f32) have the same expressions with T = f32: nothing is rounded to
16 bits, every stage's f32 rounding is part of that stage's arithmetic error, and ties are not carried.
FFN mode (lwdetr_ffn_partial): h = T(ReLU(x W1[hs]^T + b1[hs])) (accumulators start at the bias), slab s = h W2[:, hs]^T in f32 - not rounded again.

GELU. 16-bit forms: common.h:gelu_fast16, x rcp(1 + exp2(x p(min(x^2, 36)))) with a three-term p. tests/vitblock_sim.py:gelu_fast16 is that expression
(it is NOT vitblock.hip's two-term gelu_vb16); `gelu16` below is the same in torch with the coefficients as f32 stores them, and
tests/test_mlp_bound_host.py checks the two against each other. Error: 1.2 e_h for the argument (|GELU'| <= 1.13) + |g| (2 TRANS_F32 + 3 U23 (1 + |t|)),
t the exponent, for exp2 / rcp and the six roundings. f32 forms: gelu_erf / fast_erf (Abramowitz-Stegun 7.1.26); the reference is the EXACT erf GELU in
float64 and the bound adds |x| / 2 times: the documented approximation error 1.5e-7; exp(-x^2 / 2) (17.2 TRANS_F32 + 57 U23 + x^2 U23) for rcp and exp
and the Horner roundings (condition of the polynomial in t <= sum i |a_i| = 16.2; exp's argument is rounded twice); 2 U23 for x / sqrt 2 and 1 - .;
and 1.5 U23 |g| for the last three operations.

Bound. Stage by stage as in test_gpu_vitblock.py's docstring, with this file's MFMA: Mma<T>::k32 is ONE 16x16x32 step in 16 bits - 32 exact products
and the accumulator, at most 33 additions on an element's path, one accumulator update per step - so over K / 32 steps
|acc^ - acc| <= U23 ((K / 32 + 2) |start| + (K / 32 + 34) S), S = sum_k |a_k w_k| of that element. In f32 k32 is eight 16x16x4 steps whose four
products are rounded: K / 4 steps, U23 ((K / 4 + 2) |start| + (K / 4 + 7) S). fc2 of mlp_small adds three steps per wave and seven partial sums:
fewer additions on any path than the K / 32 = 24 ... 48 steps counted. LayerNorm: a lane adds C / 4 values and two exchanges, fewer than the
C / 2 + 2 of ln_stage. Tie deviations are carried in both modes exactly as there (worst case: every element; tight, Z = 4: SHARE = 1e-3 of a tensor
may lie outside). No term is scaled by a tensor-wide maximum.

Hardware transcendentals: TRANS_F32 = 4 TRANS_MEASURED. Measured on an MI355X over this module's cases:
  * rstd of the statistics output against the float64 rstd of the kernel's own stored rows (check_stats prints it): see MEASURED below;
  * f32 GELU: test_mlp_f32_gelu_measured makes h VISIBLE - rows of zeros (z = 0, so the GELU argument is b1' exactly), W2 a selection matrix, g2 = 1,
    b2 = 0, so out = h bit for bit - and compares it with the float64 erf GELU over 1536 arguments in [-6, 6].
MEASURED (MI355X, 256 CUs, committed seeds). rstd: over the 107 launches of this module that write statistics the raw relative deviation from the
float64 rstd of the stored rows is at most 3.963 x 2^-23 (bf16, C = 384, 32784 rows; f32 forms: 1.482 x 2^-23) and 0.000 x 2^-23 beyond the derived
arithmetic of the two-pass variance in every launch. f32 GELU: over 8 x 192 arguments the raw deviation |h^ - gelu64| is at most 3.388e-7 |x| / 2
(2.842 x 2^-23) - the f32 evaluation of the rational form costs more than its documented 1.5e-7 - and the transcendental share beyond approximation
and arithmetic is 0.000 x 2^-23; worst |diff| / bound 0.327. TRANS_MEASURED is therefore one f32 ulp, 2^-23 (the larger of the two shares and an
ulp), margin factor 4 as everywhere in this project. Worst |diff| / bound per launch form: profiles/mlp_fp64_worst_ratios.txt.

M % Tp != 0 with the chained QKV (case f): the entries accept it. Row m goes to image m / Tp, position m % Tp in all three kernels (`bq_ = mq / p.Tp`),
so rows 20 .. 23 of M = 24, Tp = 20 are positions 0 .. 3 of image 1; q / k / v^T hold ceil(M / Tp) images and the rest of image 1 stays untouched.

mlp_f32_c384_*: the record names them, but two f32 weight-tile buffers at C = 384 are 218 KB, more than a CU's LDS; the launch function refuses them
with LWDETR_ERR_UNSUPPORTED before anything is launched (test_mlp_f32_c384_is_refused), so 41 of the 44 names can be launched.
"""
import numpy as np
import pytest
import torch

from lwdetr_amd import _native
from tests import test_gpu_rowops as R
from tests import test_gpu_vitblock as V
from tests.helpers import mlp_served_by
from tests.test_gpu_rowops import half_ulp, U23, SENT, PADV, F16, BF16, F32
from tests.test_gpu_vitblock import (round_stage, prop, n_eff, ln_stage, stats_bounds, bound_of, check2, fails_exactly, make_rows, make_weights,
                                     rows_layout, Buf, Z, SHARE, GELU_LIP, QSCALE, EPS, EPS_NEXT)

TRANS_MEASURED = 2.0 ** -23   # one f32 ulp: both visible transcendentals measured 0 beyond the derived arithmetic (module docstring)
TRANS_F32 = 4 * TRANS_MEASURED
assert TRANS_F32 == V.TRANS_F32          # stats_bounds (taken over) is built on that module's constant
ERF_APPROX = 1.5e-7           # documented accuracy of the Abramowitz-Stegun 7.1.26 rational form behind fast_erf
BAD_ARG, UNSUPPORTED = _native.ERR_BAD_ARG, _native.ERR_UNSUPPORTED
NAME = {F16: "f16", BF16: "bf16", F32: "f32"}
FORM_WORST = {}               # launch form -> largest |diff| / worst-case bound seen
FORM_TIGHT = {}               # launch form -> (largest |diff| / tight bound among the elements inside it, elements outside, elements)
RAN = set()                   # ids of the element-wise cases that ran to their end in this process
ALL_CASES = set()             # ... and of all there are (filled by the parameter builders)
_CACHE = {}
CHUNK = 16384                 # rows per reference evaluation


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_error():
    """A launch that faulted leaves the device in an error state: the session ends there instead of starting further kernels on it."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"the GPU reported an error; nothing more is started on it: {e}", returncode=3)


def cached(key, fn):
    """Cases and references are computed once and shared between the tests that need them; nothing modifies them."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def ref_device():
    return torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")


def _dev():
    return torch.device("cuda:0")


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def big_form(T, C, proj, qkv):
    return f"mlp_{NAME[T]}_c{C}_proj{int(proj)}_qkv{int(qkv)}"


def small_form(T, tt, qkv, frag):
    return f"mlp_small_{NAME[T]}_tt{tt}_qkv{int(qkv)}_frag{int(frag)}"


def few384_form(T, qkv):
    return f"vit_few384_{NAME[T]}_qkv{int(qkv)}"


def ffn_form(T, C):
    return f"ffn_{NAME[T]}_c{C}"


ALL_FORMS = ([big_form(T, C, p, q) for T in (F16, BF16, F32) for C in (192, 384) for p, q in ((0, 0), (1, 0), (1, 1))]
             + [small_form(T, tt, q, f) for T in (F16, BF16) for tt in (1, 2) for q in (0, 1) for f in (0, 1)]
             + [small_form(F32, 1, q, 1) for q in (0, 1)] + [few384_form(T, q) for T in (F16, BF16) for q in (0, 1)]
             + [ffn_form(T, C) for T in (F16, BF16) for C in (256, 384)])
REFUSED_FORMS = {big_form(F32, 384, p, q) for p, q in ((0, 0), (1, 0), (1, 1))}      # more LDS than a CU has (module docstring)


def big_tt(T, C):
    return 2 if (T != F32 and C == 192) else 1


def big_tpw(T, C, proj):
    return 7 if (T != F32 and C == 192 and proj) else 8


# ------------------------------------------------------------------------------------------------------------ arithmetic models
_GC = [float(np.float32(c)) for c in (0.0010142630555, -0.1067757240036, -2.3011213394584)]


def gelu16(x):
    """common.h:gelu_fast16 in float64 (torch), coefficients as f32 stores them; returns the value and the exponent t = x p."""
    x2 = torch.clamp_max(x * x, 36.0)
    t = x * ((x2 * _GC[0] + _GC[1]) * x2 + _GC[2])
    return x / (1.0 + torch.exp2(t)), t


def gelu_erf64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gelu_erf_bound(x, g):
    """What gelu_erf's f32 result may differ from the float64 erf GELU of the same argument by (module docstring)."""
    u2 = x * x / 2
    return x.abs() / 2 * (ERF_APPROX + torch.exp(-u2) * (17.2 * TRANS_F32 + 57 * U23 + 2 * u2 * U23) + 2 * U23) + 1.5 * U23 * g.abs()


def acc_err(K, start_abs, S, mode, T):
    steps, per = (K // 4, 5) if T == F32 else (K // 32, 32)
    return U23 * (n_eff(steps + 2, mode) * start_abs + n_eff(steps + per + 2, mode) * S)


def stage(pre, e, sg, T, mode):
    """round_stage for the 16-bit types; in f32 nothing is rounded to a shorter type: the value stays, its deviation is carried as it is."""
    if T == F32:
        return pre, e, sg, torch.zeros_like(pre)
    return round_stage(pre, e, sg, T, mode)


def ln_any(x, e, sg, eps, T, mode):
    """ln_stage; for f32 the same first-order propagation without the rounding to T."""
    if T != F32:
        return ln_stage(x, e, sg, eps, T, mode)[:3]
    C = x.shape[1]
    mean = x.mean(1, keepdim=True)
    dd = x - mean
    rstd = 1.0 / torch.sqrt((dd * dd).mean(1, keepdim=True) + float(np.float32(eps)))
    z = dd * rstd
    m = x.abs().mean(1, keepdim=True)
    n = C // 2 + 2
    e_ln = 0.5 * U23 * ((n_eff(n // 2 + 8, mode) + 2) * z.abs() + (n_eff(n + 1, mode) + 3) * m * rstd) + TRANS_F32 * z.abs()
    pe = 1.05 * rstd * (e + e.mean(1, keepdim=True) + z.abs() * (z.abs() * e).mean(1, keepdim=True))
    ps = 1.05 * rstd * torch.sqrt(sg * sg + (sg * sg).sum(1, keepdim=True) / C ** 2 + z * z * (z * z * sg * sg).sum(1, keepdim=True) / C ** 2)
    return z, e_ln + pe, ps


def qkv_tail(rows, e_rows, sg_rows, D, T, eps, mode):
    """q (scaled), k, v as (M, C) float64 BEFORE the last rounding and their E: accumulators start at the bias, q is scaled in f32."""
    C = rows.shape[1]
    z, ez, sz = ln_any(rows, e_rows, sg_rows, eps, T, mode)
    y = z @ D["wq"].t() + D["bq"]
    e = acc_err(C, D["bq"].abs().expand_as(y), z.abs() @ D["wq"].abs().t(), mode, T)
    pe, ps = prop(ez, sz, D["wq"], mode)
    qs = float(np.float32(QSCALE))
    scale = torch.cat([torch.full((C,), qs, dtype=torch.float64), torch.ones(2 * C, dtype=torch.float64)]).to(rows.device)
    y, E = y * scale, (e + pe + Z * ps) * scale + U23 * (y * scale).abs() * (scale != 1)
    return dict(q=(y[:, :C], E[:, :C]), k=(y[:, C:2 * C], E[:, C:2 * C]), v=(y[:, 2 * C:], E[:, 2 * C:]))


def _mlp_reference(x, att, D, T, mode, proj, qkv):
    """float64 evaluation with the kernel's rounding points; {name: (value before the last rounding, E)} for x (the new rows), q, k, v."""
    x = x.double()
    C = x.shape[1]
    zero = torch.zeros_like(x)
    if proj:
        att = att.double()
        t1 = att @ D["wp"].t() + D["bp"]
        pre1 = x + D["g1"] * t1
        e1 = D["g1"].abs() * (acc_err(C, zero, att.abs() @ D["wp"].abs().t(), mode, T) + U23 * t1.abs()) + U23 * (D["g1"] * t1).abs() + U23 * pre1.abs()
        x1, ex1, sx1, _ = stage(pre1, e1, zero, T, mode)
    else:
        x1, ex1, sx1 = x, zero, zero
    z, ez, sz = ln_any(x1, ex1, sx1, EPS, T, mode)
    hpre = z @ D["w1"].t() + D["b1"]
    pe, ps = prop(ez, sz, D["w1"], mode)
    eh = acc_err(C, D["b1"].abs().expand_as(hpre), z.abs() @ D["w1"].abs().t(), mode, T) + pe
    if T == F32:
        g = gelu_erf64(hpre)
        eg = GELU_LIP * eh + gelu_erf_bound(hpre, g)
    else:
        g, t = gelu16(hpre)
        eg = GELU_LIP * eh + g.abs() * (2 * TRANS_F32 + 3 * U23 * (1 + t.abs()))
    h, eh2, sh2, _ = stage(g, eg, GELU_LIP * ps, T, mode)
    t2 = h @ D["w2"].t() + D["b2"]
    pre2 = x1 + D["g2"] * t2
    pe2, ps2 = prop(eh2, sh2, D["w2"], mode)
    e2 = (D["g2"].abs() * (acc_err(4 * C, torch.zeros_like(t2), h.abs() @ D["w2"].abs().t(), mode, T) + pe2 + U23 * t2.abs()) + U23 * (D["g2"] * t2).abs()
          + ex1 + U23 * pre2.abs())
    s2 = torch.sqrt((D["g2"] * ps2) ** 2 + sx1 ** 2)
    out = {"x": (pre2, e2 + Z * s2)}
    if qkv:
        o, eo, so, _ = stage(pre2, e2, s2, T, mode)
        out.update(qkv_tail(o, eo, so, D, T, EPS_NEXT, mode))
    return out


def mlp_reference(x, att, D, T, mode, proj, qkv):
    """_mlp_reference in chunks of rows on the reference device; the result on the CPU."""
    dev = ref_device()
    Dd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in D.items()}
    parts = [_mlp_reference(x[i:i + CHUNK].to(dev), att[i:i + CHUNK].to(dev) if proj else None, Dd, T, mode, proj, qkv) for i in range(0, x.shape[0], CHUNK)]
    return {n: tuple(torch.cat([p[n][j] for p in parts]).cpu() for j in (0, 1)) for n in parts[0]}


# ------------------------------------------------------------------------------------------------------------ inputs
def dense_weights(W, T):
    """The weights and vectors the kernels see, dense, float64: the f32 expressions of kernels.pack_mlp_weights / pack_qkv_weights rounded to T,
    the folded biases as those functions return them (operands as stored)."""
    from lwdetr_amd import kernels as K
    f = lambda t: t.float().to(T).double()
    _, b1f, _ = K.pack_mlp_weights(W["w1"], W["b1"], W["w2"], W["ln2_w"], W["ln2_b"], T)
    _, bq = K.pack_qkv_weights(W["wqkv"], W["qb"], W["vb"], W["ln1_w"], W["ln1_b"], T)
    return dict(wp=f(W["wp"]), w1=f(W["w1"].float() * W["ln2_w"].float()[None, :]), w2=f(W["w2"]), wq=f(W["wqkv"].float() * W["ln1_w"].float()[None, :]),
                b1=b1f.double(), bq=bq.double(), bp=W["bp"].float().double(), g1=W["g1"].float().double(), b2=W["b2"].float().double(),
                g2=W["g2"].float().double())


def packed(W, T, proj):
    """Device operands of both entries: row-major (lwdetr_mlp_fused) and fragment-major (lwdetr_vit_block_few) weights, f32 vectors."""
    def build():
        from lwdetr_amd import kernels as K
        w1p, b1p, w2c = K.pack_mlp_weights(W["w1"], W["b1"], W["w2"], W["ln2_w"], W["ln2_b"], T, proj=proj)
        wq, bq = K.pack_qkv_weights(W["wqkv"], W["qb"], W["vb"], W["ln1_w"], W["ln1_b"], T)
        wp = W["wp"].to(T).contiguous()
        d = dict(w1=w1p, b1=b1p, w2=w2c, wq=wq, bq=bq, wp=wp, w1F=K.pack_frag16(w1p), wqF=K.pack_frag16(wq), wpF=K.pack_frag16(wp),
                 bp=W["bp"].float().contiguous(), g1=W["g1"].float().contiguous(), b2=W["b2"].float().contiguous(), g2=W["g2"].float().contiguous())
        return {k: v.to(_dev()) for k, v in d.items()}
    return cached(("packed", id(W), T, proj), build)


def mlp_case(C, M, T, proj, qkv, seed=0):
    def build():
        W = make_weights(C, seed)
        x, att = make_rows(M, C, T, seed), make_rows(M, C, T, seed + 7, scale=1.0, shift=0.0)
        D = cached(("dense", C, T, seed), lambda: dense_weights(W, T))
        return dict(W=W, x=x, att=att, D=D, tight=mlp_reference(x, att, D, T, "tight", proj, qkv), worst=mlp_reference(x, att, D, T, "worst", proj, qkv))
    return cached(("mlp", C, M, T, proj, qkv, seed), build)


# ------------------------------------------------------------------------------------------------------------ comparison
def check(form, got, ref_t, ref_w, T, label):
    """check2 (every element inside the worst-case bound, at most SHARE outside the tight one) + the per-form table of worst ratios."""
    y, et = ref_t
    ew = ref_w[1]
    got, y, et, ew = got.double().flatten(), y.flatten(), et.flatten(), ew.flatten()
    err = (got - y).abs()
    bw, bt = bound_of(y, ew, T), bound_of(y, et, T)
    FORM_WORST[form] = max(FORM_WORST.get(form, 0.0), float((err / bw).max()))
    inl = err <= bt
    old = FORM_TIGHT.get(form, (0.0, 0, 0))
    FORM_TIGHT[form] = (max(old[0], float((err[inl] / bt[inl]).max()) if bool(inl.any()) else 0.0), old[1] + int((~inl).sum()), old[2] + err.numel())
    try:
        return check2(got, y, et, ew, T, label)
    finally:                                   # check2 files its ratios under the other module's prefix
        for k in [k for k in R.WORST if k.startswith(f"{V.PFX}:{label} (")]:
            R.WORST.pop(k)


def check_stats(st, rows, label):
    """The statistics output against the float64 statistics of the kernel's own stored rows; prints the visible rstd deviation."""
    st = st.cpu().double()
    mean, bm, rstd, br, arith = stats_bounds(rows)(EPS_NEXT)
    raw = (st[:, 1] / rstd - 1).abs()
    dev = (raw - arith / rstd).clamp_min(0).max().item()
    print(f"MLP_RSTD {label}: rstd relative deviation {raw.max().item() / U23:.3f} x 2^-23 (beyond the derived arithmetic: {dev / U23:.3f} x 2^-23)")
    for got, exp, bnd, what in ((st[:, 0], mean, bm, "mean"), (st[:, 1], rstd, br, "rstd")):
        ok, worst, nbad = R.compare(got, exp, bnd)
        assert ok, f"{label}: stats {what}^: {nbad} rows outside their bound, worst err / bound {worst:.3f}"
    assert dev <= TRANS_F32, f"{label}: rstd deviates by {dev / U23:.3f} x 2^-23 beyond the arithmetic, TRANS_F32 is {TRANS_F32 / U23:.0f} x 2^-23"


def teardown_module(module):
    if FORM_WORST:
        print("\nworst |diff| / bound per launch form (worst-case bound; tight bound among the elements inside it, elements outside / all):")
        for f in sorted(f for f in FORM_WORST if f in ALL_FORMS):
            t = FORM_TIGHT[f]
            print(f"MLP_WORST_FORM {f:<34s} {FORM_WORST[f]:.3f}   {t[0]:.3f} {t[1]} / {t[2]}")


# ------------------------------------------------------------------------------------------------------------ GPU plumbing
ARGS = ("x", "ldx", "w1", "b1", "w2", "b2", "g2", "out2", "ld2", "stats", "M", "C", "eps", "eps_next", "att", "ldatt", "wp", "bp", "g1", "wq", "bq", "q", "k",
        "vt", "qscale", "heads", "hd", "Tp", "dtype")


class Run:
    """One lwdetr_mlp_fused (entry "fused") or lwdetr_vit_block_few (entry "few": fragment-major weights) call on guarded buffers: x in place between
    guard rows (pad columns when ldx > C), strided att whose pad columns hold 7777, taps in the right half of a 2 C wide buffer, stats, flat q / k /
    v^T of ceil(M / Tp) images with guard elements in front and behind. shared: x and the tap are column slices of ONE buffer (case g)."""

    def __init__(self, case, C, M, T, *, entry="fused", proj=True, qkv=False, extras=False, hd=32, Tp=4, ldx=None, ldatt=None, ld2=None, shared=False,
                 over_w=None, qscale=QSCALE):
        self.C, self.M, self.T, self.entry, self.proj, self.qkv, self.extras, self.hd, self.Tp, self.shared = C, M, T, entry, proj, qkv, extras, hd, Tp, shared
        self.heads = C // hd
        self.w = dict(packed(case["W"], T, proj))
        self.w.update(over_w or {})
        self.ldatt = ldatt or C
        if shared:
            self.ldx = self.ld2 = 2 * C + 16
            self.tapcol = C + 8
            self.x = Buf(M, self.ldx, T)
            self.taps = self.x
        else:
            self.ldx, self.ld2 = ldx or C, ld2 or 2 * C
            self.tapcol = self.ld2 - C
            self.x = Buf(M, self.ldx, T)
            self.taps = Buf(M, self.ld2, T); self.taps.freeze()
        self.x.load(case["x"]); self.x.freeze()
        self.case_x = case["x"]
        self.att = torch.full((M, self.ldatt), PADV, dtype=T, device=_dev())
        self.att[:, :C] = case["att"].to(_dev())
        self.stats = Buf(M, 2, torch.float32); self.stats.freeze()
        self.nimg = -(-M // Tp)
        self.q, self.k, self.vt = (Buf(self.nimg * Tp * C, 1, T, pre=64, post=64) for _ in range(3))
        for b in (self.q, self.k, self.vt):
            b.freeze()
        self.qscale = qscale

    def args(self, **over):
        w, F = self.w, "F" if self.entry == "few" else ""
        a = dict(x=self.x.ptr(), ldx=self.ldx, w1=w["w1" + F].data_ptr(), b1=w["b1"].data_ptr(), w2=w["w2"].data_ptr(), b2=w["b2"].data_ptr(),
                 g2=w["g2"].data_ptr(), out2=self.taps.ptr(self.tapcol) if self.extras else None, ld2=self.ld2 if self.extras else 0,
                 stats=self.stats.ptr() if self.extras else None, M=self.M, C=self.C, eps=EPS, eps_next=EPS_NEXT,
                 att=self.att.data_ptr() if self.proj else None, ldatt=self.ldatt, wp=w["wp" + F].data_ptr() if self.proj else None,
                 bp=w["bp"].data_ptr() if self.proj else None, g1=w["g1"].data_ptr() if self.proj else None,
                 wq=w["wq" + F].data_ptr() if self.qkv else None, bq=w["bq"].data_ptr() if self.qkv else None,
                 q=self.q.ptr() if self.qkv else None, k=self.k.ptr() if self.qkv else None, vt=self.vt.ptr() if self.qkv else None,
                 qscale=self.qscale, heads=self.heads if self.qkv else 0, hd=self.hd if self.qkv else 0, Tp=self.Tp if self.qkv else 0,
                 dtype=_native.dtype_code(self.T))
        a.update(over)
        return [a[k] for k in ARGS]

    def __call__(self, **over):
        fn = _native.lib().lwdetr_vit_block_few if self.entry == "few" else _native.lib().lwdetr_mlp_fused
        rc = fn(*self.args(**over), _native.stream_ptr(_dev()))
        torch.cuda.synchronize()
        return rc

    def buffers(self):
        return [b for b in (self.x, self.taps, self.stats, self.q, self.k, self.vt) if not (b is self.taps and self.shared)]

    def outputs_untouched(self):
        return all(b.guards_intact() for b in self.buffers())

    def reset(self):
        self.x.load(self.case_x)


def outputs(run, label):
    """The outputs of a Run as rows {x, q, k, v} after the guard checks: rows at or beyond M, pad columns, the left half of the tap buffer, the
    elements in front of and behind q / k / v^T, the positions of a partial last image and every output that was not requested are bit-identical
    to the sentinel; the tap is x bit for bit."""
    C, M, T = run.C, run.M, run.T
    if run.shared:
        a, b = run.x.buf.clone(), run.x.snap.clone()
        for col in ((0, run.tapcol) if run.extras else (0,)):
            a[run.x.pre:run.x.pre + M, col:col + C] = 0
            b[run.x.pre:run.x.pre + M, col:col + C] = 0
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{label}: the shared x / tap buffer was written outside the two column slices"
    else:
        assert run.x.guards_intact(0, C), f"{label}: x rows at or beyond M / pad columns were written"
    got = {"x": run.x.body(0, C).cpu()}
    if run.extras:
        if not run.shared:
            assert run.taps.guards_intact(run.tapcol, C), f"{label}: the tap buffer was written outside its right half / beyond M"
        assert torch.equal(run.taps.body(run.tapcol, C).cpu().view(torch.uint8), got["x"].view(torch.uint8)), f"{label}: the tap is not x bit for bit"
        assert run.stats.guards_intact(0, 2), f"{label}: stats rows beyond M were written"
    else:
        assert run.stats.guards_intact() and (run.shared or run.taps.guards_intact()), f"{label}: taps / stats written although not requested"
    if run.qkv:
        for name, b, tr in (("q", run.q, False), ("k", run.k, False), ("v", run.vt, True)):
            assert b.guards_intact(0, 1), f"{label}: elements in front of / behind {name} were written"
            rows = rows_layout(b.body(0, 1).cpu().flatten(), run.nimg, run.Tp, run.heads, run.hd, tr)
            assert bool((rows[M:] == torch.tensor(SENT).to(T)).all()), f"{label}: {name} was written at positions of the last image that no row has"
            got[name] = rows[:M]
    else:
        assert all(b.guards_intact() for b in (run.q, run.k, run.vt)), f"{label}: q / k / vt written although not requested"
    return got


def check_run(run, case, form, label):
    got = outputs(run, label)
    for n in got:
        check(form, got[n], case["tight"][n], case["worst"][n], run.T, f"{label} {n}")
    if run.extras:
        check_stats(run.stats.body(0, 2), got["x"], label)
    return got


def _case_id(*parts):
    cid = "-".join(str(p) for p in parts)
    ALL_CASES.add(cid)
    return cid


# ------------------------------------------------------------------------------------------------------------ mlp_kernel, ViT mode
HDS = {192: [16, 32, 64], 384: [32, 64, 128]}
BIG_FORMS = [(T, C, p, q) for T in (F16, BF16, F32) for C in (192, 384) for p, q in ((0, 0), (1, 0), (1, 1)) if not (T == F32 and C == 384)]


def _pin_big(knobs, T, C, proj):
    if T != F32 and C == 192 and proj:
        knobs.set("MLP_SMALL", 0)              # below 12800 rows the 16-bit C = 192 forms with the projection go to the few-token kernel


def _big_abc():
    out = []
    for i, (T, C, p, q) in enumerate(BIG_FORMS):
        tt = big_tt(T, C)
        for j, (sid, M, Tp) in enumerate((("a", 4, 4), ("b", 16 * tt + 4, 12 if tt == 2 else 4), ("c", 40, 20))):
            hd = HDS[C][(i + j) % 3]
            out.append(pytest.param(T, C, p, q, sid, M, Tp, hd, sid != "a", id=_case_id("big", big_form(T, C, p, q), sid)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("T,C,proj,qkv,sid,M,Tp,hd,extras", _big_abc())
def test_mlp_kernel_vs_fp64(T, C, proj, qkv, sid, M, Tp, hd, extras, knobs, request):
    """(a) M = 4: one lane group of one tile, seven idle waves on clamped rows; (b) M = 16 TT + 4: a ragged second tile; (c) M = 40, Tp = 20: an image
    boundary and a 4-token V^T run inside a tile. (a) runs without tap / statistics: neither buffer may be touched."""
    _pin_big(knobs, T, C, proj)
    form = big_form(T, C, proj, qkv)
    case = mlp_case(C, M, T, proj, qkv)
    run = Run(case, C, M, T, proj=proj, qkv=qkv, extras=extras, hd=hd, Tp=Tp)
    with mlp_served_by(form):
        assert run() == 0
    check_run(run, case, form, f"{form} ({sid})")
    if sid == "c":                                             # a second launch on the same inputs is bit-identical
        first = [b.buf.clone() for b in run.buffers()]
        run.reset()
        assert run() == 0
        assert all(torch.equal(a.view(torch.uint8), b.buf.view(torch.uint8)) for a, b in zip(first, run.buffers())), f"{form}: a second launch differs"
    RAN.add(request.node.callspec.id)


def _tp_for(M):
    """A divisor of M = 4 (odd) that is a multiple of 4 and not of 16: four times the smallest odd prime factor (M itself when there is none)."""
    odd = M // 4
    assert M % 16 == 4 and odd % 2 == 1
    p = next((d for d in range(3, int(odd ** 0.5) + 1, 2) if odd % d == 0), odd)
    return 4 * p


@pytest.mark.gpu
@pytest.mark.parametrize("T,C", [(F16, 192), (BF16, 384), (F32, 192)], ids=lambda v: str(v).split(".")[-1])
def test_mlp_kernel_uneven_dealing_vs_fp64(T, C, knobs):
    """(d) M = 16 TT (N + 1) + 4: ntiles = N + 2 over N workgroups, tb = 1, tr = 2 - two workgroups run a second wave, the last tile is ragged."""
    _pin_big(knobs, T, C, True)
    M = 16 * big_tt(T, C) * (ncu() + 1) + 4
    Tp = _tp_for(M)
    form = big_form(T, C, True, True)
    case = mlp_case(C, M, T, True, True)
    run = Run(case, C, M, T, qkv=True, extras=True, hd=HDS[C][1], Tp=Tp)
    with mlp_served_by(form):
        assert run() == 0
    check_run(run, case, form, f"{form} (d: M {M}, Tp {Tp})")


@pytest.mark.gpu
@pytest.mark.parametrize("T,C,qkv", [(F16, 192, False), (BF16, 384, True)], ids=["f16-c192-tpw7", "bf16-c384-tpw8"])
def test_mlp_kernel_extra_rounds_vs_fp64(T, C, qkv, knobs):
    """(e) M = 16 TT (N TPW + 1): one tile more than N workgroups take - the grid grows beyond one workgroup per CU. Every row is checked."""
    _pin_big(knobs, T, C, True)
    tt, tpw = big_tt(T, C), big_tpw(T, C, True)
    M = 16 * tt * (ncu() * tpw + 1)
    form = big_form(T, C, True, qkv)
    case = mlp_case(C, M, T, True, qkv)
    run = Run(case, C, M, T, qkv=qkv, extras=True, hd=HDS[C][0], Tp=16)
    with mlp_served_by(form):
        assert run() == 0
    check_run(run, case, form, f"{form} (e: M {M})")


@pytest.mark.gpu
@pytest.mark.parametrize("T,C", [(F16, 192), (BF16, 192), (F32, 192), (F16, 384), (BF16, 384)], ids=lambda v: str(v).split(".")[-1])
def test_mlp_kernel_partial_last_image_vs_fp64(T, C, knobs):
    """(f) M = 24, Tp = 20 with the chained QKV: rows 20 .. 23 are positions 0 .. 3 of image 1 (include/lwdetr_hip.h), the other 16 stay untouched."""
    _pin_big(knobs, T, C, True)
    form = big_form(T, C, True, True)
    case = mlp_case(C, 24, T, True, True)
    run = Run(case, C, 24, T, qkv=True, extras=True, hd=HDS[C][2], Tp=20)
    assert run.nimg == 2
    with mlp_served_by(form):
        assert run() == 0
    check_run(run, case, form, f"{form} (f)")


@pytest.mark.gpu
def test_mlp_kernel_strided_and_shared_buffer_vs_fp64(knobs):
    """(g) x and the tap are column slices of one (M, 2 C + 16) buffer (ldx = ld2 = 2 C + 16), the launch runs in place, ldatt = C + 24."""
    T, C, M = F16, 192, 40
    _pin_big(knobs, T, C, True)
    form = big_form(T, C, True, True)
    case = mlp_case(C, M, T, True, True)
    run = Run(case, C, M, T, qkv=True, extras=True, hd=32, Tp=20, ldatt=C + 24, shared=True)
    with mlp_served_by(form):
        assert run() == 0
    check_run(run, case, form, f"{form} (g)")


@pytest.mark.gpu
def test_mlp_f32_c384_is_refused():
    """float32 at C = 384 needs more LDS than a CU has: UNSUPPORTED from the launch function, nothing written or counted - and no error left behind
    for the next launch's check (the attribute call used to fail with hipErrorInvalidValue, which stayed the runtime's last error: the valid launch
    below then answered LWDETR_ERR_LAUNCH and was not counted)."""
    case = mlp_case(384, 4, F32, True, True)
    for proj, qkv in ((False, False), (True, False), (True, True)):
        run = Run(case, 384, 4, F32, proj=proj, qkv=qkv, extras=True, hd=32, Tp=4)
        before = _native.mlp_path_counts()
        assert run() == UNSUPPORTED
        assert _native.mlp_path_counts() == before and run.outputs_untouched()
    ok = mlp_case(192, 4, F32, True, False)
    run = Run(ok, 192, 4, F32)
    with mlp_served_by(big_form(F32, 192, True, False)):
        assert run() == 0


# ------------------------------------------------------------------------------------------------------------ the few-token kernels
SMALL_SHAPES = [("M4", lambda tt: 4, 4, 16), ("ragged", lambda tt: 16 * tt + 4, 4, 64), ("M40", lambda tt: 40, 20, 32), ("M48", lambda tt: 48, 16, 64)]


def _small16():
    return [pytest.param(T, tt, q, sid, mf(tt), Tp, hd, id=_case_id("small", NAME[T], f"tt{tt}", f"qkv{q}", sid))
            for T in (F16, BF16) for tt in (1, 2) for q in (0, 1) for sid, mf, Tp, hd in SMALL_SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize("T,tt,qkv,sid,M,Tp,hd", _small16())
def test_mlp_small_vs_fp64_and_both_weight_layouts_agree(T, tt, qkv, sid, M, Tp, hd, knobs, request):
    """mlp_small_kernel through both entries - lwdetr_mlp_fused (row-major weights, frag0) and lwdetr_vit_block_few (fragment-major, frag1) - with
    LWDETR_MLP_SMALL_TT pinned: each against float64, and bit-identical to one another."""
    knobs.set("MLP_SMALL_TT", tt)
    case = mlp_case(192, M, T, True, bool(qkv))
    bufs = []
    for frag, entry in ((0, "fused"), (1, "few")):
        form = small_form(T, tt, qkv, frag)
        run = Run(case, 192, M, T, entry=entry, qkv=bool(qkv), extras=sid != "M4", hd=hd, Tp=Tp, ldx=200 if sid == "M48" else None)
        with mlp_served_by(form):
            assert run() == 0
        check_run(run, case, form, f"{form} ({sid})")
        bufs.append([b.buf.clone() for b in run.buffers()])
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*bufs)), "row-major and fragment-major weights give different bits"
    RAN.add(request.node.callspec.id)


def _few_other():
    out = []
    for q in (0, 1):
        for sid, mf, Tp, hd in SMALL_SHAPES:
            out.append(pytest.param(F32, 192, q, sid, mf(1), Tp, hd, id=_case_id("few", "f32-c192", f"qkv{q}", sid)))
            for T in (F16, BF16):
                out.append(pytest.param(T, 384, q, sid, mf(1), Tp, 2 * hd, id=_case_id("few", f"{NAME[T]}-c384", f"qkv{q}", sid)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("T,C,qkv,sid,M,Tp,hd", _few_other())
def test_vit_block_few_f32_and_c384_vs_fp64(T, C, qkv, sid, M, Tp, hd, request):
    """The f32 form of the few-token kernel and vit_block_few384_kernel (16-token workgroups at every M) at the same edge shapes."""
    form = small_form(F32, 1, qkv, 1) if T == F32 else few384_form(T, qkv)
    case = mlp_case(C, M, T, True, bool(qkv))
    run = Run(case, C, M, T, entry="few", qkv=bool(qkv), extras=sid != "M4", hd=hd, Tp=Tp, ldx=C + 8 if sid == "M48" else None)
    with mlp_served_by(form):
        assert run() == 0
    check_run(run, case, form, f"{form} ({sid})")
    RAN.add(request.node.callspec.id)


@pytest.mark.gpu
def test_mlp_routing_without_knobs():
    """Which kernel serves a row count when no switch is set, by the record: 3200 rows and below 16-token workgroups, up to 12796 32-token ones,
    from 12800 mlp_kernel; lwdetr_vit_block_few refuses 12800."""
    T, C = F16, 192
    case = dict(W=make_weights(C, 0), x=make_rows(12800, C, T, 0), att=make_rows(12800, C, T, 7, scale=1.0, shift=0.0))       # no reference: the record is the check
    for entry, M, form in (("fused", 3200, small_form(T, 1, 0, 0)), ("fused", 3204, small_form(T, 2, 0, 0)), ("fused", 12796, small_form(T, 2, 0, 0)),
                           ("fused", 12800, big_form(T, C, True, False)), ("few", 3200, small_form(T, 1, 0, 1)), ("few", 3204, small_form(T, 2, 0, 1)),
                           ("few", 12796, small_form(T, 2, 0, 1))):
        sub = dict(case, x=case["x"][:M], att=case["att"][:M])
        run = Run(sub, C, M, T, entry=entry)
        with mlp_served_by(form):
            assert run() == 0, (entry, M)
        assert run.x.guards_intact(0, C)
    run = Run(case, C, 12800, T, entry="few")
    before = _native.mlp_path_counts()
    assert run() == UNSUPPORTED and _native.mlp_path_counts() == before and run.outputs_untouched()


# ------------------------------------------------------------------------------------------------------------ FFN mode
def ffn_tt(C):
    return 2 if C == 256 else 1


def ffn_splits_model(M, C, hid, n_cu, s_max=16):
    """launch_ffn's S and grid, restated: (S, workgroups in x) or UNSUPPORTED."""
    ntiles = -(-M // (16 * ffn_tt(C)))
    blocks = -(-ntiles // 8)
    nch = hid // 32
    S = 1
    while (nch // S) * 32 > 4 * C and nch % (S * 2) == 0:       # forced: the bias slice lives in 4 C floats of LDS
        S *= 2
    if (nch // S) * 32 > 4 * C:
        return UNSUPPORTED, 0
    while S * 2 * blocks <= n_cu and nch % (S * 2) == 0 and nch // (S * 2) >= 2 and S * 2 <= s_max:
        S *= 2
    if n_cu // S > blocks:                                      # spare CUs: fewer tiles per workgroup
        blocks = min(n_cu // S, ntiles)
    return S, blocks


def ffn_weights(C, hid, T, seed=0):
    def build():
        from lwdetr_amd import kernels as K
        g = torch.Generator().manual_seed(5000 + seed + C + hid)
        w1, b1 = torch.randn(hid, C, generator=g) / C ** 0.5, torch.randn(hid, generator=g) * 0.2
        w2 = torch.randn(C, hid, generator=g) / hid ** 0.5
        w1p, b1p, w2c = K.pack_mlp_weights(w1, b1, w2, None, None, T)
        return dict(w1=w1p, b1=b1p, w2=w2c, D=dict(w1=w1.to(T).double(), b1=b1.double(), w2=w2.to(T).double()))
    return cached(("ffnw", C, hid, T, seed), build)


def ffn_reference(x, D, T, mode, S):
    """Slab s = T(ReLU(x W1[hs]^T + b1[hs])) W2[:, hs]^T in float64 and its E, stacked (S M, C). The output is f32: no last rounding."""
    dev = ref_device()
    x = x.double().to(dev)
    w1, b1, w2 = (D[k].to(dev) for k in ("w1", "b1", "w2"))
    C, hid = x.shape[1], w1.shape[0]
    hpre = x @ w1.t() + b1
    eh = acc_err(C, b1.abs().expand_as(hpre), x.abs() @ w1.abs().t(), mode, T)
    h, eh2, sh2, _ = round_stage(torch.relu(hpre), eh, torch.zeros_like(hpre), T, mode)          # |ReLU(a) - ReLU(b)| <= |a - b|
    n = hid // S
    ys, es = [], []
    for s in range(S):
        sl = slice(s * n, s * n + n)
        y = h[:, sl] @ w2[:, sl].t()
        pe, ps = prop(eh2[:, sl], sh2[:, sl], w2[:, sl], mode)
        ys.append(y)
        es.append(acc_err(n, torch.zeros_like(y), h[:, sl].abs() @ w2[:, sl].abs().t(), mode, T) + pe + Z * ps)
    return torch.cat(ys).cpu(), torch.cat(es).cpu()


def ffn_case(C, hid, M, T, S):
    def build():
        w = ffn_weights(C, hid, T)
        x = make_rows(M, C, T, 11)
        return dict(x=x, w=w, tight={"p": ffn_reference(x, w["D"], T, "tight", S)}, worst={"p": ffn_reference(x, w["D"], T, "worst", S)})
    return cached(("ffn", C, hid, M, T, S), build)


class FfnRun:
    """One lwdetr_ffn_partial call: x with pad columns (7777), S slabs of (M, C) floats between 64 guard floats."""

    def __init__(self, case, C, hid, M, T, S, ldx=None, over_w=None):
        self.C, self.hid, self.M, self.T, self.S = C, hid, M, T, S
        self.ldx = ldx or C + 8
        self.w = {k: v.to(_dev()) for k, v in case["w"].items() if k != "D"}
        self.w.update(over_w or {})
        self.x = torch.full((M, self.ldx), PADV, dtype=T, device=_dev())
        self.x[:, :C] = case["x"].to(_dev())
        self.part = Buf(S * M * C, 1, torch.float32, pre=64, post=64); self.part.freeze()

    def __call__(self, **over):
        a = dict(x=self.x.data_ptr(), ldx=self.ldx, w1=self.w["w1"].data_ptr(), b1=self.w["b1"].data_ptr(), w2=self.w["w2"].data_ptr(), partial=self.part.ptr(),
                 M=self.M, C=self.C, hid=self.hid, dtype=_native.dtype_code(self.T))
        a.update(over)
        rc = _native.lib().lwdetr_ffn_partial(*[a[k] for k in ("x", "ldx", "w1", "b1", "w2", "partial", "M", "C", "hid", "dtype")], _native.stream_ptr(_dev()))
        torch.cuda.synchronize()
        return rc

    def slabs(self, label):
        assert self.part.guards_intact(0, 1), f"{label}: floats in front of the first / behind the last slab were written"
        return self.part.body(0, 1).cpu().reshape(self.S * self.M, self.C)


def check_ffn(form, got, case, label):
    """As check(), on the f32 slabs: the bound is E alone (the kernel does not round the accumulators again)."""
    y, et = case["tight"]["p"]
    ew = case["worst"]["p"][1]
    err = (got.double() - y).abs()
    FORM_WORST[form] = max(FORM_WORST.get(form, 0.0), float((err / ew).max()))
    inl = err <= et
    old = FORM_TIGHT.get(form, (0.0, 0, 0))
    FORM_TIGHT[form] = (max(old[0], float((err[inl] / et[inl]).max()) if bool(inl.any()) else 0.0), old[1] + int((~inl).sum()), old[2] + err.numel())
    print(f"{label}: err/worst-case {float((err / ew).max()):.3f}, {int((~inl).sum())} of {err.numel()} outside the tight bound")
    assert bool((err <= ew).all()), f"{label}: {int((~(err <= ew)).sum())} elements outside the worst-case bound, worst {float((err / ew).max()):.3f}"
    assert int((~inl).sum()) <= int(SHARE * err.numel()), f"{label}: {int((~inl).sum())} of {err.numel()} elements outside the tight bound"


def _ffn_params():
    return [pytest.param(T, C, hid, mid, id=_case_id("ffn", NAME[T], f"c{C}", f"hid{hid}", mid))
            for T in (F16, BF16) for C in (256, 384) for hid in (64, 1024, 2048) for mid in ("M1", "ragged", "M300")]


@pytest.mark.gpu
@pytest.mark.parametrize("T,C,hid,mid", _ffn_params())
def test_ffn_partial_vs_fp64(T, C, hid, mid, request):
    """Every slab of lwdetr_ffn_partial against float64 over its own hidden slice; the slab count is the one lwdetr_ffn_splits announces and the
    Python model of launch_ffn computes."""
    M = {"M1": 1, "ragged": 16 * ffn_tt(C) + 1, "M300": 300}[mid]
    S = _native.lib().lwdetr_ffn_splits(M, C, hid, _native.dtype_code(T))
    assert S == ffn_splits_model(M, C, hid, ncu())[0] and S >= 1
    case = ffn_case(C, hid, M, T, S)
    run = FfnRun(case, C, hid, M, T, S)
    form = ffn_form(T, C)
    with mlp_served_by(form):
        assert run() == 0
    check_ffn(form, run.slabs(form), case, f"{form} hid {hid} M {M} S {S}")
    RAN.add(request.node.callspec.id)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [256, 384])
def test_ffn_splits_follow_the_model(C, knobs):
    """LWDETR_FFN_SPLITS = 1 ... 16 at hid = 2048: lwdetr_ffn_splits is the model's S - never below 2 ((nch / S) 32 > 4 C forces the first split at
    both widths) - the query counts nothing, and a launch at every setting writes exactly S slabs that meet the float64 reference."""
    T, hid = F16, 2048
    seen = set()
    for s in (1, 2, 4, 8, 16):
        knobs.set("FFN_SPLITS", s)
        for M in (1, 300, 4000):
            before = _native.mlp_path_counts()
            S = _native.lib().lwdetr_ffn_splits(M, C, hid, _native.dtype_code(T))
            assert _native.mlp_path_counts() == before, "the query was counted"
            assert S == ffn_splits_model(M, C, hid, ncu(), s)[0], (s, M, S)
            assert S >= 2
        M = 16 * ffn_tt(C) + 1
        S = _native.lib().lwdetr_ffn_splits(M, C, hid, _native.dtype_code(T))
        seen.add(S)
        case = ffn_case(C, hid, M, T, S)
        run = FfnRun(case, C, hid, M, T, S)
        with mlp_served_by(ffn_form(T, C)):
            assert run() == 0
        check_ffn(ffn_form(T, C), run.slabs("splits"), case, f"{ffn_form(T, C)} FFN_SPLITS {s}: S {S}")
    assert seen == {2, 4, 8, 16}                               # 2048 hidden units are more than 4 C at both widths: S = 1 never


@pytest.mark.gpu
@pytest.mark.parametrize("T,C", [(F16, 256), (BF16, 384)], ids=lambda v: str(v).split(".")[-1])
def test_ffn_spare_cu_branch_vs_fp64(T, C, knobs):
    """S pinned to 16, M = 16 TT (N / 16 + 1) + 1: N / 16 + 2 tiles over N / 16 workgroups per split - the "spare CUs" branch with more than one tile
    in two workgroups and a one-row last tile."""
    knobs.set("FFN_SPLITS", 16)
    n, hid = ncu(), 2048
    M = 16 * ffn_tt(C) * (n // 16 + 1) + 1
    S, blocks = ffn_splits_model(M, C, hid, n, 16)
    assert S == 16 and blocks == n // 16 and -(-M // (16 * ffn_tt(C))) == blocks + 2
    assert _native.lib().lwdetr_ffn_splits(M, C, hid, _native.dtype_code(T)) == S
    case = ffn_case(C, hid, M, T, S)
    run = FfnRun(case, C, hid, M, T, S)
    with mlp_served_by(ffn_form(T, C)):
        assert run() == 0
    check_ffn(ffn_form(T, C), run.slabs("spare"), case, f"{ffn_form(T, C)} spare CUs M {M}")


@pytest.mark.gpu
def test_ffn_refusals():
    T, C, hid, M = F16, 256, 1024, 40
    S = _native.lib().lwdetr_ffn_splits(M, C, hid, _native.dtype_code(T))
    case = ffn_case(C, hid, M, T, S)
    run = FfnRun(case, C, hid, M, T, S)

    def refused(expect, label, **over):
        before = _native.mlp_path_counts()
        rc = run(**over)
        assert rc == expect, f"{label}: rc {rc}, expected {expect}"
        assert _native.mlp_path_counts() == before and run.part.guards_intact(), f"{label}: something was written or counted"

    refused(UNSUPPORTED, "hid = 2112 at C = 256", hid=2112)
    assert _native.lib().lwdetr_ffn_splits(M, C, 2112, _native.dtype_code(T)) == -UNSUPPORTED
    refused(BAD_ARG, "hid = 96", hid=96)
    refused(BAD_ARG, "ldx % 8", ldx=C + 4)
    refused(UNSUPPORTED, "C = 192", C=192)
    refused(UNSUPPORTED, "dtype f32", dtype=_native.dtype_code(F32))
    for n in ("x", "w1", "b1", "w2", "partial"):
        refused(BAD_ARG, f"{n} = NULL", **{n: None})
    refused(0, "M = 0", M=0)


# ------------------------------------------------------------------------------------------------------------ sensitivity
SENS_M, SENS_TP, SENS_HD = 40, 20, 32


def _alt(case, T, **changes):
    D = dict(case["D"]); D.update(changes)
    return mlp_reference(case["x"], case["att"], D, T, "tight", True, True)


def quiet_channel(case, T):
    y, e = case["tight"]["x"]
    return int((bound_of(y, e, T) / half_ulp(y, T)).median(0).values.argmin())


def sens_bias(case, T, which):
    """(key of the packed operands, index, new f32 value, alt reference, dependent): one entry of b2 / bp / b1' / bqkv' moved so that the output it
    feeds most moves by four ulps of that channel's typical value."""
    D = case["D"]
    M, C = case["x"].shape
    allrows, col = torch.ones(M, C, dtype=torch.bool), torch.zeros(M, C, dtype=torch.bool)
    ulp4 = lambda name, ch: float(8 * half_ulp(case["tight"][name][0][:, ch].abs().median(), T))
    if which == "bq":
        idx, delta = C + 5, ulp4("k", 5)                               # a k feature
        col[:, 5] = True
        dep = dict(k=col)
    elif which == "b1":
        idx = 37
        gain = (D["g2"] * D["w2"][:, idx]).abs() / half_ulp(case["tight"]["x"][0].abs().median(0).values, T)
        ch = int(gain.argmax())
        delta = ulp4("x", ch) / float((D["g2"] * D["w2"][:, idx]).abs()[ch]) * 2      # GELU' is about 1/2 ... 1 where the unit is active
        dep = dict(x=allrows, q=allrows, k=allrows, v=allrows)
    else:
        idx = quiet_channel(case, T)
        delta = ulp4("x", idx) / float(D["g2" if which == "b2" else "g1"][idx].abs())
        col[:, idx] = True
        dep = dict(x=col if which == "b2" else allrows, q=allrows, k=allrows, v=allrows)
    newv = D[which].clone()
    newv[idx] = float(np.float32(float(newv[idx]) + delta))
    return which, idx, float(newv[idx]), _alt(case, T, **{which: newv}), dep


def sens_swap_w2(case, T):
    """(alt reference, dependent): output channels 0 .. 15 and 16 .. 31 of W2 exchanged = the two 16-row fragments n = 0, 1 of every hidden chunk."""
    D = case["D"]
    M, C = case["x"].shape
    w = D["w2"].clone()
    w[0:16], w[16:32] = D["w2"][16:32], D["w2"][0:16]
    xdep = torch.zeros(M, C, dtype=torch.bool)
    xdep[:, :32] = True
    allrows = torch.ones(M, C, dtype=torch.bool)
    return _alt(case, T, w2=w), dict(x=xdep, q=allrows, k=allrows, v=allrows)


def _sens_run(knobs, kind, over_w=None):
    T, C = F16, 192
    case = mlp_case(C, SENS_M, T, True, True)
    if kind == "big":
        knobs.set("MLP_SMALL", 0)
        form = big_form(T, C, True, True)
    else:
        knobs.set("MLP_SMALL_TT", 1)
        form = small_form(T, 1, 1, 0)
    return case, form, Run(case, C, SENS_M, T, qkv=True, hd=SENS_HD, Tp=SENS_TP, over_w=over_w)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["b2", "bp", "b1", "bq"])
@pytest.mark.parametrize("kind", ["big", "small"])
def test_mlp_sensitivity_one_bias_entry(kind, which, knobs):
    """One entry of b2 / bp / b1' / bqkv' moved by four output ulps; the reference keeps the original: exactly the dependent elements fail."""
    case, form, _ = _sens_run(knobs, kind)
    key, idx, val, alt, dep = sens_bias(case, F16, which)
    vec = packed(case["W"], F16, True)[key].clone()
    vec[idx] = val
    _, _, run = _sens_run(knobs, kind, over_w={key: vec})
    with mlp_served_by(form):
        assert run() == 0
    fails_exactly(outputs(run, which), case, alt, F16, f"sensitivity {form} {which}", dep)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["big", "small"])
def test_mlp_sensitivity_swapped_w2_fragments(kind, knobs):
    case, form, _ = _sens_run(knobs, kind)
    alt, dep = sens_swap_w2(case, F16)
    w2 = packed(case["W"], F16, True)["w2"].clone()                      # chunk-major (4 C / 32, C, 32)
    w2[:, 0:16], w2[:, 16:32] = packed(case["W"], F16, True)["w2"][:, 16:32], packed(case["W"], F16, True)["w2"][:, 0:16]
    _, _, run = _sens_run(knobs, kind, over_w={"w2": w2.contiguous()})
    with mlp_served_by(form):
        assert run() == 0
    fails_exactly(outputs(run, "swap"), case, alt, F16, f"sensitivity {form} swapped W2 fragments", dep)


FFN_SENS = (256, 1024, 40)


def ffn_sens(case, T, S, what):
    """(packed operand, alt reference, dependent (S M, C)) for one altered b1 entry / the exchanged W2 fragments of the FFN."""
    C, hid, M = FFN_SENS
    D = dict(case["w"]["D"])
    dep = torch.zeros(S, M, C, dtype=torch.bool)
    if what == "b1":
        idx = 37
        hp = case["x"].double() @ D["w1"][idx] + D["b1"][idx]
        delta = float(8 * half_ulp(hp[hp > 0].median(), T))                 # four ulps of T at the unit's typical output: the slabs are f32 and have none
        b1 = D["b1"].clone()
        b1[idx] = float(np.float32(float(b1[idx]) + delta))
        D["b1"] = b1
        dep[idx // (hid // S)] = True
        op = ("b1", b1.float())
    else:
        w = D["w2"].clone()
        w[0:16], w[16:32] = D["w2"][16:32], D["w2"][0:16]
        D["w2"] = w
        dep[:, :, :32] = True
        w2 = case["w"]["w2"].clone()
        w2[:, 0:16], w2[:, 16:32] = case["w"]["w2"][:, 16:32], case["w"]["w2"][:, 0:16]
        op = ("w2", w2.contiguous())
    return op, {"p": ffn_reference(case["x"], D, T, "tight", S)}, {"p": dep.reshape(S * M, C)}


def ffn_fails_exactly(got, case, alt, label, dependent):
    """fails_exactly for the f32 slabs, whose bound is E alone."""
    y, e = case["tight"]["p"]
    ya, ea = alt["p"]
    dep = dependent["p"]
    fail = ~((got.double() - y).abs() <= e)
    must = ((ya - y).abs() > e + ea) & dep
    print(f"{label}: {int(fail.sum())} fail, {int(must.sum())} must, {int(dep.sum())} dependent")
    assert not bool((fail & ~dep).any()), f"{label}: {int((fail & ~dep).sum())} elements fail that do not depend on the altered value"
    assert bool((fail | ~must).all()), f"{label}: {int((must & ~fail).sum())} elements pass although their reference moved beyond the bound"
    assert int(must.sum()) > 0, f"{label}: the alteration moves no reference element beyond its bound - it tests nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["b1", "w2"])
def test_ffn_sensitivity(what):
    T = F16
    C, hid, M = FFN_SENS
    S = _native.lib().lwdetr_ffn_splits(M, C, hid, _native.dtype_code(T))
    case = ffn_case(C, hid, M, T, S)
    (key, val), alt, dep = ffn_sens(case, T, S, what)
    run = FfnRun(case, C, hid, M, T, S, over_w={key: val.to(_dev())})
    with mlp_served_by(ffn_form(T, C)):
        assert run() == 0
    ffn_fails_exactly(run.slabs(what), case, alt, f"sensitivity ffn {what}", dep)


# ------------------------------------------------------------------------------------------------------------ measured transcendentals
@pytest.mark.gpu
def test_mlp_f32_gelu_measured():
    """h of the f32 kernel made visible (module docstring): rows of zeros, so the GELU argument is b1' exactly; W2 selects one hidden unit per channel,
    g2 = 1, b2 = 0: out = gelu_erf(b1'[4 c]) bit for bit. 8 launches x 192 arguments over [-6, 6] against the float64 erf GELU."""
    from lwdetr_amd import kernels as K
    T, C, M = F32, 192, 4
    worst_raw = worst_beyond = worst_ratio = 0.0
    for it in range(8):
        g = torch.Generator().manual_seed(6000 + it)
        b1 = (torch.rand(4 * C, generator=g) * 12 - 6).float()
        if it == 0:
            b1[:16] = torch.tensor([0.0, -0.0, 1e-3, -1e-3, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0, 6.0, -6.0])
        w2 = torch.zeros(C, 4 * C)
        w2[torch.arange(C), 4 * torch.arange(C)] = 1.0
        w1p, b1p, w2c = K.pack_mlp_weights(torch.randn(4 * C, C, generator=g), b1, w2, torch.ones(C), torch.zeros(C), T)
        assert torch.equal(b1p, b1)
        x = torch.zeros(M + 2, C, dtype=T, device=_dev())
        x[M:] = SENT
        w1d, b1d, w2d, zer, one = w1p.to(_dev()), b1p.to(_dev()), w2c.to(_dev()), torch.zeros(C, device=_dev()), torch.ones(C, device=_dev())
        rc = _native.lib().lwdetr_mlp_fused(x.data_ptr(), C, w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), zer.data_ptr(), one.data_ptr(), None, 0, None, M, C, EPS, EPS_NEXT,
                                            None, C, None, None, None, None, None, None, None, None, 1.0, 0, 0, 0, _native.dtype_code(T), _native.stream_ptr(_dev()))
        torch.cuda.synchronize()
        assert rc == 0 and bool((x[M:] == SENT).all())
        arg = b1[4 * torch.arange(C)].double()
        ref = gelu_erf64(arg)
        for r in range(M):
            d = (x[r].cpu().double() - ref).abs()
            nz = arg.abs() > 0
            worst_raw = max(worst_raw, float((d[nz] / (arg[nz].abs() / 2)).max()))
            arith = arg.abs() / 2 * (ERF_APPROX + torch.exp(-arg * arg / 2) * (57 * U23 + arg * arg * U23) + 2 * U23) + 1.5 * U23 * ref.abs() + half_ulp(ref, F32)
            beyond = ((d - arith).clamp_min(0)[nz] / (arg[nz].abs() / 2 * torch.exp(-arg[nz] ** 2 / 2) * 17.2)).max()
            worst_beyond = max(worst_beyond, float(beyond))
            bnd = gelu_erf_bound(arg, ref) + half_ulp(ref, F32)
            worst_ratio = max(worst_ratio, float((d / bnd.clamp_min(1e-300)).max()))
            assert bool((d <= bnd).all())
    print(f"MLP_TRANS f32 GELU: worst |h^ - gelu64| / (|x| / 2) = {worst_raw:.3e} ({worst_raw / U23:.3f} x 2^-23); transcendental share beyond approximation "
          f"and arithmetic {worst_beyond / U23:.3f} x 2^-23; worst |diff| / bound {worst_ratio:.3f}")
    assert worst_beyond <= TRANS_F32


# ------------------------------------------------------------------------------------------------------------ refusals of lwdetr_mlp_fused
@pytest.mark.gpu
def test_mlp_fused_refusals(knobs):
    T, C, M, Tp, hd = F16, 192, 40, 20, 32
    case = mlp_case(C, M, T, True, True)
    run = Run(case, C, M, T, qkv=True, extras=True, hd=hd, Tp=Tp, ldx=C + 8, ldatt=C + 16)

    def refused(expect, label, **over):
        before = _native.mlp_path_counts()
        rc = run(**over)
        assert rc == expect, f"{label}: rc {rc}, expected {expect}"
        assert _native.mlp_path_counts() == before, f"{label}: the record moved"
        assert run.outputs_untouched(), f"{label}: an output was written"

    for small in (None, 0):                                   # with the few-token kernel ahead (default at this M) and with mlp_kernel pinned
        if small is not None:
            knobs.set("MLP_SMALL", small)
        for n in ("x", "w1", "b1", "w2", "b2", "g2"):
            refused(BAD_ARG, f"{n} = NULL", **{n: None})
        for n in ("wp", "bp", "g1"):
            refused(BAD_ARG, f"att without {n}", **{n: None})
        for n in ("bq", "q", "k", "vt"):
            refused(BAD_ARG, f"wqkv without {n}", **{n: None})
        refused(BAD_ARG, "M < 0", M=-4)
        refused(BAD_ARG, "ldx % 8", ldx=C + 4)
        refused(BAD_ARG, "ld2 % 8", ld2=2 * C + 4)
        refused(BAD_ARG, "ldatt % 8", ldatt=C + 4)
        refused(UNSUPPORTED, "wqkv without att", att=None)
        refused(BAD_ARG, "M % 4 with QKV", M=38)
        refused(BAD_ARG, "Tp % 4 with QKV", Tp=10)
        refused(BAD_ARG, "hd % 4", heads=32, hd=6)
        refused(BAD_ARG, "heads * hd != C", heads=5, hd=32)
        refused(BAD_ARG, "heads = 0", heads=0)
        refused(UNSUPPORTED, "C = 256", C=256, heads=8)
        refused(UNSUPPORTED, "dtype f64", dtype=_native.DT_F64)
        refused(0, "M = 0", M=0)


# ------------------------------------------------------------------------------------------------------------ the record, at the end
@pytest.mark.gpu
def test_mlp_every_instantiation_was_launched():
    """Every name of lwdetr_mlp_path_name was launched at least once by an element-wise case of this module - except the three f32 C = 384 names, which
    must never have been (module docstring). Skipped unless all of the module's cases ran before it (it is the module's last test)."""
    counts = _native.mlp_path_counts()
    assert list(counts) == ALL_FORMS and len(counts) == 44
    assert all(counts[f] == 0 for f in REFUSED_FORMS), {f: counts[f] for f in REFUSED_FORMS}
    if RAN != ALL_CASES:
        pytest.skip(f"{len(ALL_CASES - RAN)} of the module's {len(ALL_CASES)} cases did not run in this process")
    missing = [f for f in ALL_FORMS if f not in REFUSED_FORMS and (counts[f] == 0 or f not in FORM_WORST)]
    assert not missing, missing
    assert all(FORM_WORST[f] < 1 for f in ALL_FORMS if f in FORM_WORST), {f: v for f, v in FORM_WORST.items() if f in ALL_FORMS and not v < 1}
