"""The three kernels of csrc/vitblock.hip (lwdetr_vit_block, lwdetr_vit_qkv, lwdetr_vit_stem), called directly at the smallest shapes at which
their token dealing, buffer-bounded stores and launch forms can go wrong, every launch pinned to ONE instantiation by the launch-form record
(lwdetr_vit_path_counts, helpers.vit_served_by) and every output checked ELEMENT BY ELEMENT against float64 arithmetic on the operands as stored.
Output buffers carry guard rows / guard elements / pad columns filled with a sentinel that must come back bit-identical.

Reference. float64 throughout, rounded to the storage type T exactly where the kernel rounds (read from vitblock.hip), nowhere else:
  * the 16-bit weights: Wp, W1' = fc1 * ln2_w, W2, Wqkv' = Wqkv * ln1_w (the f32 products rounded to T, as kernels.pack_vit_block does); the f32
    vectors b1' = b1 + W1 ln2_b, bp, g1, fl(1/g1), b2, fl(1/g2), g2, bqkv' are taken from the packed `vec` (operands as stored);
  * x1 = T(g1 (x fl(1/g1) + bp + att Wp^T))                          (`pack2<T>(gg * acc2)` of the LayerNorm section);
  * z = T((x1 - mean) rstd), the B fragments of fc1                   (`pack2<T>(fmaf(v, rstd, nmr))`);
  * h = T(GELU(z W1'^T + b1')), the B fragments of fc2: the kernel's own two-term expression, vitblock_sim.gelu_vb16 (f32 arithmetic, one
    rounding at the end) or gelu_vb16_packed (the f16 default: the argument and every operation rounded to f16);
  * out = T(g2 (x1 fl(1/g2) + b2 + h W2^T)), the stored result (and the tap, bit for bit);
  * z' = T((out - mean') rstd'), the B fragments of the chained QKV (statistics of the ROUNDED rows, eps_next);
  * q = T((z' Wq'^T + bq') qscale), k = T(z' Wk'^T + bk'), v^T = T(z' Wv'^T + bv').
lwdetr_vit_qkv is the last two lines on the stored x. lwdetr_vit_stem: x0 = T(pos + b + patch Wpe^T) (Wpe rounded to T, the 768 = (channel, patch
row, pixel) values of the token's patch; accumulators start at fl(pos + b)), then the same tail. PAD ROWS of the stem (rows i >= (Hp/4)(Wp/4) of a
window): the kernel reads no pixels for them (their loads are out of the buffer's range: zeros), so a pad row is the row of an all-zero patch,
x = T(pos[row] + b), and its q / k / v^T are the tail of that row - stored like any other row, independent of the image.

Bound. For an output element with float64 value y (before the last rounding) the kernel's stored number may differ by half_ulp_T(|y| + E) + E,
E = the deviation of the kernel's f32 value from y. E is built stage by stage from the reference's own numbers (U23 = 2^-23):
  f32 accumulation. A 32x32x16 MFMA adds 16 exact products to the accumulator: at most 17 additions on an element's path inside a step and one
    accumulator update per step, each off by at most 2^-23 of the partial sum (2^-24 if the matrix pipe rounded to nearest; it may truncate, so
    2^-23). Over K/16 steps: |acc^ - acc| <= U23 ((K/16 + 2) |start| + (K/16 + 18) S), S = sum_k |a_k w_k| of THAT element and `start` what the
    accumulator starts at (+ 2: the fma that forms it and the final scale);
  x (1/gamma) start. The accumulators start at x fl(1/g) + b and the result is g acc: the reference evaluates exactly that expression with the
    stored fl(1/g), so what remains is the accumulation error of the start value, |g| U23 (K/16 + 2) |x fl(1/g)| ~ U23 (K/16 + 2) |x| whatever g is
    (14 / 26 / 50 / 98 units of 2^-23 |x| for K = 192 / 384 / 768 / 1536: 3e-6 ... 1.2e-5 |x|, against 2^-11 |x| for half an f16 ulp);
  LayerNorm. The derivation of test_gpu_rowops.ln_reference with n_add = C / 2 + 2 serial f32 additions per lane (+ the half-wave exchange):
    |z^ - z| <= U23 (n_add + C_LN) (|x_i| + mean|x|) rstd; the kernel's fmaf(x, rstd, -mean rstd) form is covered by the (|x_i| + m) rstd factor;
  GELU (f32 form): 1.2 e_h for the argument (|GELU'| <= 1.13) + |g| (2 TRANS_F32 + 3 U23 (1 + |t|)), t the exponent, for exp2 / rcp and 5 roundings;
  the other side of a tie. An intermediate v that is rounded to T with |v^ - v| <= e lands on the same T number as the reference's unless v is
    within e of a rounding tie of T; where it is, the kernel's rounded number may differ by up to e + ulp_T. These elements are FOUND in the
    reference's own intermediates (x1, z, h, the f16 GELU argument, out, z') and their deviation d is carried into everything computed from them:
    directly (out inherits d(x1): the residual), through a LayerNorm (first order, as test_gpu_rowops.ln2_propagated) and through a product, where
      worst case:  sum_k d_k |w_k|                        (every flagged operand off, all with the worst sign)
      tight     :  Z sqrt(sum_k s_k^2 w_k^2),  Z = 4      STATISTICAL: the flagged operands are off independently, with either sign.
    The tight bound may leave SHARE = 1e-3 of a tensor's elements outside (floor(SHARE n) elements); every element meets the worst-case bound.
    tests/test_vitblock_bound_host.py shows on the CPU that an independent f32 evaluation stays within both.
  packed-f16 GELU (G16). gelu_vb16_packed is the bit-level model up to v_exp_f16 / v_rcp_f16, modelled correctly rounded. The hardware's may be off
    by an ulp each; through x * rcp(1 + exp) that is at most G16_HW ulp_f16(h) on h. Carried like a tie deviation (on EVERY hidden element).
No term is scaled by a tensor-wide maximum.

Hardware transcendentals: TRANS_F32 = 4 * TRANS_MEASURED. The one f32 transcendental whose result is visible is the reciprocal square root of the
statistics output. Measured on an MI355X over this module's block cases (make_rows / make_weights with the committed seeds; f16 / bf16, C = 192 / 384,
M = 8 ... 520; check_stats prints it as "rstd relative deviation"): rstd^ of `stats` deviates from the float64 rstd of the stored rows by NOTHING
beyond the derived f32 arithmetic of the two-pass variance (0.00 x 2^-23 in every launch) - `1.f / sqrtf(.)` is compiled correctly rounded here.
TRANS_MEASURED is therefore kept at one f32 ulp, 2^-23, the documented accuracy of v_exp_f32 / v_rcp_f32 / v_rsq_f32, which the f32 GELU uses and
whose results are not visible on their own; factor 4: another valid input set moves such a figure by that much. G16_HW: see above (ISA accuracy, 1 ulp
per instruction); the worst-ratio table in profiles/r8a_vitblock_fp64_worst_ratios.txt is the check that both suffice.

Statistics output: mean^ / rstd^ against the float64 statistics of the kernel's own stored rows, bounds from ln_reference's derivation (n_add as
above); the blanket 1e-4 of test_gpu_kernels.py::test_vit_block is kept as a secondary check.

What the norm-wise assertions of test_vit_block accept (arithmetic on its inputs, see the issue this module answers): max|ref| = 10.7 (C = 192) /
10.9 (C = 384), so 6e-3 / 5e-2 of it lets every element be off by 0.064 (f16) / 0.54 (bf16), while max|gamma2 b2| = 0.113 and max|gamma1 bp| =
0.139 ... 0.146: a bf16 kernel that never adds b2 or bp passes them, an f16 one on most channels. The sensitivity tests below alter ONE entry of b2 /
bp / bqkv' by four output ulps and must fail - on exactly the elements that depend on it.

The `while (...) ++grid` of launch_vb cannot trigger with grid = need: need = ceil(U / (16 NH)) for U = M / 8 units, so U <= 16 NH need and
ceil(U / (4 need)) <= 4 NH units = 32 NH tokens per wave; a larger grid (VB_GRID) only lowers the quotient. test_vitblock_bound_host.py checks the
host formula over every M up to 4096; no shape reaches the loop body.
"""
import math

import numpy as np
import pytest
import torch

from lwdetr_amd import _native
from tests import test_gpu_rowops as R
from tests.test_gpu_rowops import half_ulp, C_LN, U23, SENT, PADV, F16, BF16
from tests.vitblock_sim import gelu_vb16, gelu_vb16_packed

Z = 4.0                       # tight bound: flagged operands combine in quadrature, Z standard deviations
SHARE = 1e-3                  # share of a tensor's elements the tight bound may leave outside (they still meet the worst-case bound)
TRANS_MEASURED = 2.0 ** -23   # one f32 ulp; the visible transcendental (rstd of the statistics) measured 0 beyond the derived arithmetic (module docstring)
TRANS_F32 = 4 * TRANS_MEASURED
G16_HW = 1.0                  # ulp_f16 of the GELU output: standard deviation of what v_exp_f16 / v_rcp_f16 (1 ulp each) move it by (tight bound)
G16_HW_WORST = 3.0            # ... and the most they can: an ulp of exp through rcp (|d rcp| <= |d exp|), an ulp of rcp, one more rounding of x * rcp
GELU_LIP = 1.2
BAD_ARG, UNSUPPORTED = _native.ERR_BAD_ARG, _native.ERR_UNSUPPORTED
PFX = "vit"


def _name(dt):
    return {F16: "f16", BF16: "bf16"}[dt]


# ------------------------------------------------------------------------------------------------------------ rounding and deviations
def rnd(v, T):
    """float64 -> nearest T (ties to even), as float64: ONE rounding (a cast through float32 would round twice)."""
    ulp = 2 * half_ulp(v, T)
    return torch.round(v / ulp) * ulp


def tie_dist(v, T):
    """Distance of v to the nearest rounding tie of T (the midpoints between neighbouring T numbers)."""
    ulp = 2 * half_ulp(v, T)
    t = v.abs() / ulp
    return (t - torch.floor(t) - 0.5).abs() * ulp


def round_stage(pre, e, sg, T, mode):
    """The reference's rounded value r = T(pre) and what the kernel's rounded value may differ from it by, when its unrounded one is pre + (an
    error within e) + (a random part of standard deviation sg). Returns (r, e', sg', P).
    worst: e' = e + ulp where pre is within e of a tie, else 0 (sg = 0 throughout).
    tight: e is a Z sigma bound (n_eff), so the perturbation has standard deviation sqrt((e / Z)^2 + sg^2) =: s and the kernel lands on another T number
    with probability at most P = exp(-(t / s)^2 / 2) at distance t from the tie; then it is off by at most e + ulp + the random part:
    e' = 0, sg'^2 = P ((e + ulp)^2 + sg^2)."""
    t = tie_dist(pre, T)
    ulp = 2 * half_ulp(pre.abs() + e + Z * sg, T)
    if mode == "worst":
        return rnd(pre, T), torch.where(t <= e, e + ulp, torch.zeros_like(pre)), torch.zeros_like(pre), (t <= e).double()
    sig = torch.sqrt((e / Z) ** 2 + sg * sg).clamp_min(1e-300)      # e is the Z sigma bound of the arithmetic part in this mode
    P = torch.exp(-0.5 * (t / sig) ** 2)
    P = torch.where(P < 1e-12, torch.zeros_like(P), P)
    return rnd(pre, T), torch.zeros_like(pre), torch.sqrt(P * ((e + ulp) ** 2 + sg * sg)), P


def prop(e, sg, W, mode):
    """(e, sg) of a @ W^T when a is off by at most e plus a random part of standard deviation sg, element-wise: e adds up with the worst signs,
    the random parts in quadrature (independent operands)."""
    return e @ W.abs().t(), torch.sqrt((sg * sg) @ (W * W).t())


def n_eff(n, mode):
    """n roundings on a path: n u in the worst case; Z sqrt(n) u when they are taken as independent zero-mean errors (STATISTICAL, tight mode;
    the probabilistic rounding-error bound of Higham & Mary, SIAM J. Sci. Comput. 41 (2019), with lambda = Z)."""
    return n if mode == "worst" else min(n, Z * math.sqrt(n))


def acc_err(K, start_abs, S, mode):
    return U23 * (n_eff(K // 16 + 2, mode) * start_abs + n_eff(K // 16 + 18, mode) * S)


def ln_stage(x, e, sg, eps, T, mode):
    """z = T((x - mean) rstd) of the rows x (float64, exact T numbers) that the kernel holds up to (e, sg); returns z, e_z, sg_z, mean, rstd.
    First order in the rows' deviation (as test_gpu_rowops.ln2_propagated; 5 % on top for the second order: the deviations are below an eighth
    of a row's spread here)."""
    C = x.shape[1]
    mean = x.mean(1, keepdim=True)
    dd = x - mean
    rstd = 1.0 / torch.sqrt((dd * dd).mean(1, keepdim=True) + float(np.float32(eps)))
    z = dd * rstd
    m = x.abs().mean(1, keepdim=True)
    # ln_reference's derivation before its last simplification (u = 2^-24, n = n_add): (n / 2 + 8) |z_i| for rstd^ and the subtraction, (n + 1) m rstd
    # for mean^, |z_i| for the result; the kernel's fmaf(x, rstd, -mean rstd) form adds the rounding of -mean rstd (m rstd) - and C_LN's spare unit
    n = C // 2 + 2
    e_ln = 0.5 * U23 * ((n_eff(n // 2 + 8, mode) + 2) * z.abs() + (n_eff(n + 1, mode) + 3) * m * rstd)
    pe = 1.05 * rstd * (e + e.mean(1, keepdim=True) + z.abs() * (z.abs() * e).mean(1, keepdim=True))
    ps = 1.05 * rstd * torch.sqrt(sg * sg + (sg * sg).sum(1, keepdim=True) / C ** 2 + z * z * (z * z * sg * sg).sum(1, keepdim=True) / C ** 2)
    zr, ez, sz, _ = round_stage(z, e_ln + pe, ps, T, mode)
    return zr, ez, sz, mean[:, 0], rstd[:, 0]


def stats_bounds(rows):
    """float64 mean / rstd of stored rows and the bounds of the kernel's f32 statistics (ln_reference's derivation, n_add = C / 2 + 2)."""
    def f(eps):
        x = rows.double()
        C = x.shape[1]
        mean = x.mean(1)
        dd = x - mean[:, None]
        rstd = 1.0 / torch.sqrt((dd * dd).mean(1) + float(np.float32(eps)))
        m = x.abs().mean(1)
        k = U23 * (C // 2 + 2 + C_LN)
        t = k * m * rstd
        e_mean = k * m
        e_rstd = rstd * (k + TRANS_F32 + 1 - 1 / torch.sqrt(1 + t * t))
        return mean, e_mean + half_ulp(mean.abs() + e_mean, torch.float32), rstd, e_rstd + half_ulp(rstd + e_rstd, torch.float32), rstd * k
    return f


# ------------------------------------------------------------------------------------------------------------ inputs
def _gamma(g, c):
    """LayerScale entries from 1e-5 to 1, both signs (real checkpoints have small ones, and the kernel divides by them)."""
    mag = 10.0 ** (-5.0 * torch.rand(c, generator=g))
    mag[0], mag[1] = 1e-5, 1.0
    return mag * torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)


def make_weights(C, seed):
    return cached(("weights", C, seed), lambda: _make_weights(C, seed))


def _make_weights(C, seed):
    """f32 master tensors of one block + the next block's norm1 / QKV: non-trivial LayerNorm affines, LayerScale over five decades."""
    g = torch.Generator().manual_seed(1000 + seed + C)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(wp=r(C, C) / C ** 0.5, bp=r(C) * 0.3, g1=_gamma(g, C), w1=r(4 * C, C) / C ** 0.5, b1=r(4 * C) * 0.2, w2=r(C, 4 * C) / (4 * C) ** 0.5,
                b2=r(C) * 0.3, g2=_gamma(g, C), ln2_w=r(C) * 0.3 + 1, ln2_b=r(C) * 0.2, wqkv=r(3 * C, C) / C ** 0.5, qb=r(C) * 0.3, vb=r(C) * 0.3,
                ln1_w=r(C) * 0.3 + 1, ln1_b=r(C) * 0.2)


def make_rows(M, C, T, seed, scale=1.5, shift=0.3):
    """(M, C) rows of T; three of them (first, middle, last) with a mean twelve times their spread."""
    g = torch.Generator().manual_seed(2000 + seed + M)
    x = torch.randn(M, C, generator=g) * scale + shift
    for i in sorted({0, M // 2, M - 1}):
        x[i] = 6.0 * (-1.0) ** i + 0.5 * torch.randn(C, generator=g)
    return x.to(T)


QSCALE = 0.37                 # not a power of two
EPS, EPS_NEXT = 1e-6, 1e-5


def dense_weights(W, T):
    """The weights and vectors the kernel sees, dense, float64: the f32 expressions of kernels.pack_vit_block / pack_vit_qkv rounded to T."""
    f64 = lambda t: t.to(T).double()
    D = dict(wp=f64(W["wp"]), w1=f64(W["w1"] * W["ln2_w"][None, :]), w2=f64(W["w2"]), wq=f64(W["wqkv"] * W["ln1_w"][None, :]))
    C = W["wp"].shape[0]
    vec = packed_block(W, T, True)[1].double()                                     # the f32 vectors as stored
    for name, n in (("b1", 4 * C), ("bp", C), ("g1", C), ("rg1", C), ("b2", C), ("rg2", C), ("g2", C), ("bq", 3 * C)):
        o = _vec_section(C, name)
        D[name] = vec[o:o + n].clone()
    return D


def packed_block(W, T, qkv):
    from lwdetr_amd import kernels as K
    return cached(("pack", id(W), T, qkv), lambda: K.pack_vit_block(
        W["wp"], W["bp"], W["g1"], W["w1"], W["b1"], W["w2"], W["b2"], W["g2"], W["ln2_w"], W["ln2_b"], T,
        qkv=(W["wqkv"], W["qb"], W["vb"], W["ln1_w"], W["ln1_b"]) if qkv else None))


def _vec_section(C, name):
    return {"b1": 0, "bp": 4 * C, "g1": 5 * C, "rg1": 6 * C, "b2": 7 * C, "rg2": 8 * C, "g2": 9 * C, "bq": 10 * C}[name]


# ------------------------------------------------------------------------------------------------------------ references
def qkv_tail(rows, e_rows, sg_rows, D, T, eps, mode, chained):
    """q (scaled), k, v as (M, C) float64 BEFORE the last rounding and their E, from the rows the kernel normalises (exact T numbers, held up to
    (e_rows, sg_rows)). chained: the block kernel's form (accumulators from zero, bias then scale in f32); else lwdetr_vit_qkv / lwdetr_vit_stem
    (accumulators start at the bias)."""
    C = rows.shape[1]
    z, ez, sz, _, _ = ln_stage(rows, e_rows, sg_rows, eps, T, mode)
    y = z @ D["wq"].t() + D["bq"]
    S = z.abs() @ D["wq"].abs().t()
    e = (acc_err(C, torch.zeros_like(y), S, mode) + 2 * U23 * y.abs()) if chained else acc_err(C, D["bq"].abs().expand_as(y), S, mode)
    pe, ps = prop(ez, sz, D["wq"], mode)
    qs = float(np.float32(QSCALE))
    scale = torch.cat([torch.full((C,), qs, dtype=torch.float64), torch.ones(2 * C, dtype=torch.float64)])
    y, E = y * scale, (e + pe + Z * ps) * scale + U23 * (y * scale).abs() * (scale != 1)
    return dict(q=(y[:, :C], E[:, :C]), k=(y[:, C:2 * C], E[:, C:2 * C]), v=(y[:, 2 * C:], E[:, 2 * C:]))


def block_reference(x, att, D, T, gelu, mode, with_qkv=True):
    """float64 evaluation of lwdetr_vit_block with the kernel's rounding points. Returns {name: (value before the last rounding, E)} for
    x (the new rows), q, k, v, and under "flags" the probability-weighted share of each intermediate that may land on the other side of a tie."""
    x, att = x.double(), att.double()
    C = x.shape[1]
    zero = torch.zeros_like(x)
    start = x * D["rg1"] + D["bp"]
    S = att.abs() @ D["wp"].abs().t()
    pre1 = D["g1"] * (start + att @ D["wp"].t())
    e1 = D["g1"].abs() * acc_err(C, (x * D["rg1"]).abs() + D["bp"].abs(), S, mode) + U23 * pre1.abs()
    x1, ex1, sx1, P1 = round_stage(pre1, e1, zero, T, mode)
    z, ez, sz, _, _ = ln_stage(x1, ex1, sx1, EPS, T, mode)
    hpre = z @ D["w1"].t() + D["b1"]
    pe, ps = prop(ez, sz, D["w1"], mode)
    eh = acc_err(C, D["b1"].abs().expand_as(hpre), z.abs() @ D["w1"].abs().t(), mode) + pe
    if gelu == "packed_f16":
        assert T == F16
        xh, exh, sxh, Ph = round_stage(hpre, eh, ps, F16, mode)
        h = torch.from_numpy(gelu_vb16_packed(xh.numpy())).double()
        ulp_h = 2 * half_ulp(h, F16)
        # another f16 argument: the chain's result moves by GELU' times that, and each of its roundings may fall the other way (3 ulp);
        # the hardware's exp / rcp: G16_HW ulp on every element (worst case: with one sign; tight: independently)
        if mode == "worst":
            eh2, sh2 = GELU_LIP * exh + 3 * ulp_h * Ph + G16_HW_WORST * ulp_h, torch.zeros_like(h)
        else:
            eh2, sh2 = torch.zeros_like(h), torch.sqrt((GELU_LIP * sxh) ** 2 + Ph * (3 * ulp_h) ** 2 + (G16_HW * ulp_h) ** 2)
    else:
        g = torch.from_numpy(gelu_vb16(hpre.numpy())).double()
        t = (hpre * (-2.3087653 - 0.10012561 * hpre * hpre)).abs()
        eg = GELU_LIP * eh + g.abs() * (2 * TRANS_F32 + 3 * U23 * (1 + t))
        h, eh2, sh2, Ph = round_stage(g, eg, GELU_LIP * ps, T, mode)
    K2 = 4 * C
    pre2 = D["g2"] * (x1 * D["rg2"] + D["b2"] + h @ D["w2"].t())
    pe2, ps2 = prop(eh2, sh2, D["w2"], mode)
    gr = (D["g2"] * D["rg2"]).abs()
    e2 = D["g2"].abs() * (acc_err(K2, (x1 * D["rg2"]).abs() + D["b2"].abs(), h.abs() @ D["w2"].abs().t(), mode) + pe2) + ex1 * gr + U23 * pre2.abs()
    s2 = torch.sqrt((D["g2"] * ps2) ** 2 + (sx1 * gr) ** 2)
    out = {"x": (pre2, e2 + Z * s2), "flags": dict(x1=float(P1.mean()), z=float((sz > 0).double().mean() if mode == "tight" else (ez > 0).double().mean()),
                                                  h=float(Ph.mean()))}
    if with_qkv:
        o, eo, so, _ = round_stage(pre2, e2, s2, T, mode)
        out.update(qkv_tail(o, eo, so, D, T, EPS_NEXT, mode, chained=True))
    return out


def qkv_reference(x, D, T, mode):
    x = x.double()
    return qkv_tail(x, torch.zeros_like(x), torch.zeros_like(x), D, T, EPS_NEXT, mode, chained=False)


def bound_of(y, e, T):
    return half_ulp(y.abs() + e, T) + e


def heads_layout(y, nb, Tp, heads, hd, transposed):
    """(M, C) -> the flat (B, heads, Tp, hd) or, transposed, (B, heads, hd, Tp) order of q / k or v^T."""
    t = y.reshape(nb, Tp, heads, hd)
    return (t.permute(0, 2, 3, 1) if transposed else t.permute(0, 2, 1, 3)).reshape(-1)


def rows_layout(flat, nb, Tp, heads, hd, transposed):
    """The inverse of heads_layout: flat q / k or v^T -> (M, C) rows."""
    t = flat.reshape(nb, heads, hd, Tp).permute(0, 3, 1, 2) if transposed else flat.reshape(nb, heads, Tp, hd).permute(0, 2, 1, 3)
    return t.reshape(nb * Tp, heads * hd)


_CACHE = {}


def cached(key, fn):
    """References are computed once per (case, mode) and shared between the tests that need them; nothing modifies them."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def block_case(C, M, T, gelu, seed=0):
    def build():
        W = make_weights(C, seed)
        x, att = make_rows(M, C, T, seed), make_rows(M, C, T, seed + 7, scale=1.0, shift=0.0)
        D = dense_weights(W, T)
        return dict(W=W, x=x, att=att, D=D, tight=block_reference(x, att, D, T, gelu, "tight"), worst=block_reference(x, att, D, T, gelu, "worst"))
    return cached(("block", C, M, T, gelu, seed), build)


# ------------------------------------------------------------------------------------------------------------ comparison
def check2(got, y, e_tight, e_worst, T, label, mask=None):
    """Every element within the worst-case bound; at most floor(SHARE n) outside the tight one. Returns the elements outside the tight bound."""
    got, y = got.double().flatten(), y.double().flatten()
    bt, bw = bound_of(y, e_tight.flatten(), T), bound_of(y, e_worst.flatten(), T)
    err = (got - y).abs()
    R.compare(got, y, bw, f"{PFX}:{label} (worst-case bound)")
    out_t = ~(err <= bt)
    n_out = int(out_t.sum())
    inl = ~out_t
    ratio = float((err[inl] / bt[inl]).max()) if bool(inl.any()) else 0.0
    key = f"{PFX}:{label} (tight bound, {SHARE:g} may exceed)"
    R.WORST[key] = max(R.WORST.get(key, 0.0), ratio)
    print(f"{label}: err/tight {ratio:.3f} ({n_out} of {err.numel()} outside), err/worst-case {float((err / bw).max()):.3f}")
    assert bool((err <= bw).all()), f"{label}: {int((~(err <= bw)).sum())} elements outside the worst-case bound, worst {float((err / bw).max()):.3f}"
    assert n_out <= int(SHARE * err.numel()), f"{label}: {n_out} of {err.numel()} elements outside the tight bound (allowed {int(SHARE * err.numel())})"
    return out_t


def teardown_module(module):
    rows = [(k, v) for k, v in sorted(R.WORST.items()) if k.startswith(PFX + ":")]
    if rows:
        print("\nworst err / bound per label:")
        for k, v in rows:
            print(f"  {k[len(PFX) + 1:]:<72s} {v:.3f}")


# ------------------------------------------------------------------------------------------------------------ GPU plumbing
def _dev():
    return torch.device("cuda:0")


def form_name(T, C, half, qkv, g16):
    nh, wpc = (1, 2) if (C == 192 and half) else ((2, 1) if C == 192 else (1, 1))
    return f"vitblock_{_name(T)}_c{C}_nh{nh}_wpc{wpc}_qkv{int(qkv)}_g16_{int(g16)}"


class Buf:
    """rows x ld elements between `pre` / `post` guard rows, all sentinel; `ptr(col)` = address of (row 0, col)."""

    def __init__(self, rows, ld, dtype, pre=3, post=3, fill=SENT):
        self.rows, self.ld, self.pre = rows, ld, pre
        self.buf = torch.full((pre + rows + post, ld), fill, dtype=dtype, device=_dev())
        self.snap = None

    def load(self, t, col=0):
        self.buf[self.pre:self.pre + t.shape[0], col:col + t.shape[1]] = t.to(_dev())

    def freeze(self):
        self.snap = self.buf.clone()

    def ptr(self, col=0):
        return self.buf.data_ptr() + (self.pre * self.ld + col) * self.buf.element_size()

    def body(self, col=0, n=None):
        return self.buf[self.pre:self.pre + self.rows, col:col + (n if n is not None else self.ld - col)]

    def guards_intact(self, col=0, n=0):
        """Everything except body(col, n) is bit-identical to the snapshot."""
        a, b = self.buf.clone(), self.snap.clone()
        a[self.pre:self.pre + self.rows, col:col + n] = 0
        b[self.pre:self.pre + self.rows, col:col + n] = 0
        return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


class BlockRun:
    """One lwdetr_vit_block call on guarded buffers (x in place, strided att, taps in the right half of a 2 C wide buffer, stats, flat q / k / v^T
    with guard elements behind and in front), straight through the C entry."""

    def __init__(self, case, C, M, T, *, qkv, extras, heads=0, Tp=0, ldx=None, ldatt=None, ld2=None, stream=None, vec=None, att=None, qscale=QSCALE):
        W = case["W"]
        self.C, self.M, self.T, self.qkv, self.extras, self.heads, self.Tp = C, M, T, qkv, extras, heads, Tp
        self.hd = C // heads if heads else 0
        self.ldx, self.ldatt, self.ld2 = ldx or C, ldatt or C, ld2 or 2 * C
        if stream is None:
            stream, vec = packed_block(W, T, qkv)
        self.stream, self.vec = stream.to(_dev()), vec.to(_dev())
        self.x = Buf(M, self.ldx, T); self.x.load(case["x"]); self.x.freeze()
        self.att = torch.full((M, self.ldatt), PADV, dtype=T, device=_dev())
        self.att[:, :C] = (case["att"] if att is None else att).to(_dev())
        self.taps = Buf(M, self.ld2, T); self.taps.freeze()
        self.stats = Buf(M, 2, torch.float32); self.stats.freeze()
        self.q, self.k, self.vt = (Buf(M * C, 1, T, pre=64, post=64) for _ in range(3))
        for b in (self.q, self.k, self.vt):
            b.freeze()
        self.qscale = qscale


    def args(self, **over):
        C, M = self.C, self.M
        a = dict(x=self.x.ptr(), ldx=self.ldx, att=self.att.data_ptr(), ldatt=self.ldatt, wstream=self.stream.data_ptr(), vec=self.vec.data_ptr(),
                 out2=self.taps.ptr(self.ld2 - C) if self.extras else None, ld2=self.ld2 if self.extras else 0,
                 stats=self.stats.ptr() if self.extras else None, M=M, C=C, eps=EPS, eps_next=EPS_NEXT, has_qkv=1 if self.qkv else 0,
                 q=self.q.ptr() if self.qkv else None, k=self.k.ptr() if self.qkv else None, vt=self.vt.ptr() if self.qkv else None,
                 qscale=self.qscale, heads=self.heads, hd=self.hd, Tp=self.Tp, dtype=_native.dtype_code(self.T))
        a.update(over)
        return [a[k] for k in ("x", "ldx", "att", "ldatt", "wstream", "vec", "out2", "ld2", "stats", "M", "C", "eps", "eps_next", "has_qkv", "q", "k", "vt",
                               "qscale", "heads", "hd", "Tp", "dtype")]

    def __call__(self, **over):
        rc = _native.lib().lwdetr_vit_block(*self.args(**over), _native.stream_ptr(_dev()))
        torch.cuda.synchronize()
        return rc

    def reset_x(self, case):
        self.x.load(case["x"])

    def outputs_untouched(self):
        return all(b.guards_intact() for b in (self.x, self.taps, self.stats, self.q, self.k, self.vt))


def block_outputs(run, label):
    """The outputs of a BlockRun as (M, C) rows {x, q, k, v}, after the guard checks: rows at or beyond M, pad columns, the left half of the tap
    buffer, the elements in front of and behind q / k / v^T, and every output that was not requested are bit-identical to the sentinel."""
    C, M = run.C, run.M
    assert run.x.guards_intact(0, C), f"{label}: x rows at or beyond M / pad columns were written"
    got = {"x": run.x.body(0, C).cpu()}
    if run.extras:
        assert run.taps.guards_intact(run.ld2 - C, C), f"{label}: the tap buffer was written outside its right half / beyond M"
        assert torch.equal(run.taps.body(run.ld2 - C, C).cpu().view(torch.int16), got["x"].view(torch.int16)), f"{label}: the tap is not x bit for bit"
        assert run.stats.guards_intact(0, 2), f"{label}: stats rows beyond M were written"
    else:
        assert run.taps.guards_intact() and run.stats.guards_intact(), f"{label}: taps / stats written although not requested"
    if run.qkv:
        for name, b, tr in (("q", run.q, False), ("k", run.k, False), ("v", run.vt, True)):
            assert b.guards_intact(0, 1), f"{label}: elements in front of / behind {name} were written"
            got[name] = rows_layout(b.body(0, 1).cpu().flatten(), M // run.Tp, run.Tp, run.heads, run.hd, tr)
    else:
        assert all(b.guards_intact() for b in (run.q, run.k, run.vt)), f"{label}: q / k / vt written although not requested"
    return got


def check_stats(st, rows, label):
    """The statistics output against the float64 statistics of the kernel's own stored rows."""
    st = st.cpu().double()
    mean, bm, rstd, br, arith = stats_bounds(rows)(EPS_NEXT)
    R.assert_close(st[:, 0], mean, bm, f"{PFX}:{label} stats mean^")
    raw = (st[:, 1] / rstd - 1).abs()
    dev = (raw - arith / rstd).clamp_min(0).max().item()
    print(f"{label}: rstd relative deviation {raw.max().item() / U23:.3f} x 2^-23 (beyond the derived arithmetic: {dev / U23:.3f} x 2^-23)")
    R.assert_close(st[:, 1], rstd, br, f"{PFX}:{label} stats rstd^")
    assert (st[:, 0] - mean).abs().max().item() < 1e-4 and ((st[:, 1] - rstd).abs() / rstd).max().item() < 1e-4      # the secondary, blanket check


def check_block(run, case, label):
    got = block_outputs(run, label)
    for n in got:
        check2(got[n], case["tight"][n][0], case["tight"][n][1], case["worst"][n][1], run.T, f"{label} {n}")
    if run.extras:
        check_stats(run.stats.body(0, 2), got["x"], label)


def outside_tight(got, y, e_tight, T):
    return ~((got.double() - y).abs() <= bound_of(y, e_tight, T))


# ------------------------------------------------------------------------------------------------------------ lwdetr_vit_block
# (M, Tp, heads divisor -> hd, VB_GRID, what it exercises); NH4 = 32 NH 4 rows = one full workgroup, filled in per form
BLOCK_SHAPES = [
    ("M8", lambda nh: 8, 8, 0, None),                 # one unit, three idle waves
    ("M24", lambda nh: 24, 8, 1, None),               # three waves with one unit, one empty
    ("M40", lambda nh: 40, 8, 2, None),               # uneven deal, a wave with two units over two images
    ("WG", lambda nh: 128 * nh, 32, 3, None),         # exactly one full workgroup
    ("WG+8", lambda nh: 128 * nh + 8, 8, 0, None),    # second workgroup; floor dealing
    ("M264", lambda nh: 264, 8, "hd8", None),         # a wave's tokens span three or more images; heads = C / 8, hd = 8
    ("M64g4", lambda nh: 64, 32, 1, 4),               # grid forced above need: most waves empty
    ("Tp=M", lambda nh: 264 if nh == 1 else 520, None, 2, None),      # M = 8 (4 g 4 NH + 1), g = 2, one image
]
HDS = {192: [16, 32, 64, 8], 384: [32, 64, 128, 16]}


def _block_params():
    out = []
    for T in (F16, BF16):
        for C in (192, 384):
            for half in ((True, False) if C == 192 else (False,)):
                for g16 in ((True, False) if T == F16 else (False,)):
                    nh = 2 if (C == 192 and not half) else 1
                    for i, (sid, mf, tp, hsel, grid) in enumerate(BLOCK_SHAPES):
                        M = mf(nh)
                        hd = 8 if hsel == "hd8" else HDS[C][hsel]
                        # thinning: the bare form alternates with QKV + tap + stats over the shapes, the other way round for the other GELU / form
                        full = (i + int(half) + int(g16)) % 2 == 0
                        for qkv_extras in ((True, False) if sid in ("M40", "WG+8") else (full,)):
                            out.append(pytest.param(T, C, half, g16, sid, M, tp or M, hd, grid, qkv_extras,
                                                    id=f"{_name(T)}-C{C}-{'half' if half else 'full'}-{'g16' if g16 else 'g32'}-{sid}-{'qkv' if qkv_extras else 'bare'}"))
    return out


def _set_form(knobs, C, half, g16, grid=None):
    if C == 192:
        knobs.set("VB_HALF", 1 if half else 0)
    knobs.set("VB_GELU16", 1 if g16 else 0)
    if grid:
        knobs.set("VB_GRID", grid)


@pytest.mark.gpu
@pytest.mark.parametrize("T,C,half,g16,sid,M,Tp,hd,grid,full", _block_params())
def test_vit_block_vs_fp64(T, C, half, g16, sid, M, Tp, hd, grid, full, knobs):
    from tests.helpers import vit_served_by
    _set_form(knobs, C, half, g16, grid)
    case = block_case(C, M, T, "packed_f16" if g16 else "f32")
    run = BlockRun(case, C, M, T, qkv=full, extras=full, heads=C // hd, Tp=Tp)
    with vit_served_by(form_name(T, C, half, full, g16)):
        assert run() == 0
    label = f"block {form_name(T, C, half, full, g16)[9:]}"
    check_block(run, case, label)
    first = [b.buf.clone() for b in (run.x, run.taps, run.stats, run.q, run.k, run.vt)]
    run.reset_x(case)
    assert run() == 0
    for a, b in zip(first, (run.x, run.taps, run.stats, run.q, run.k, run.vt)):
        assert torch.equal(a.view(torch.uint8), b.buf.view(torch.uint8)), f"{label}: a second launch on the same inputs differs"


@pytest.mark.gpu
@pytest.mark.parametrize("T,C,half", [(F16, 192, True), (BF16, 192, False), (F16, 384, False), (BF16, 384, False)], ids=lambda v: str(v).split(".")[-1])
def test_vit_block_strided_vs_fp64(T, C, half, knobs):
    """ldx = C + 8, ldatt = C + 16, ld2 = 2 C: the pad columns of x and the left half of the tap buffer are guards, att's pad columns hold 7777."""
    from tests.helpers import vit_served_by
    g16 = T == F16
    _set_form(knobs, C, half, g16)
    M, Tp, hd = 136, 8, 32
    case = block_case(C, M, T, "packed_f16" if g16 else "f32")
    run = BlockRun(case, C, M, T, qkv=True, extras=True, heads=C // hd, Tp=Tp, ldx=C + 8, ldatt=C + 16, ld2=2 * C)
    with vit_served_by(form_name(T, C, half, True, g16)):
        assert run() == 0
    check_block(run, case, f"block strided {form_name(T, C, half, True, g16)[9:]}")


# ------------------------------------------------------------------------------------------------------------ lwdetr_vit_qkv
def qkv_case(C, M, T, seed=3):
    def build():
        W = make_weights(C, seed)
        x = make_rows(M, C, T, seed)
        D = dense_weights(W, T)
        return dict(W=W, x=x, D=D, tight=qkv_reference(x, D, T, "tight"), worst=qkv_reference(x, D, T, "worst"))
    return cached(("qkv", C, M, T, seed), build)


def _qkv_params():
    out = []
    for T in (F16, BF16):
        for C in (192, 384):
            nh = 2 if C == 192 else 1
            for i, (sid, mf, tp, hsel, grid) in enumerate(BLOCK_SHAPES):
                if grid:
                    continue                                # VB_GRID is a switch of the block kernel's launch only
                M = mf(nh)
                hd = 8 if hsel == "hd8" else HDS[C][hsel]
                out.append(pytest.param(T, C, M, tp or M, hd, id=f"{_name(T)}-C{C}-{sid}"))
    return out


def run_qkv(case, C, M, T, heads, Tp, ldx=None, over=None):
    from lwdetr_amd import kernels as K
    W = case["W"]
    ldx = ldx or C
    stream, vec = K.pack_vit_qkv(W["wqkv"], W["qb"], W["vb"], W["ln1_w"], W["ln1_b"], T)
    stream, vec = stream.to(_dev()), vec.to(_dev())
    x = torch.full((M, ldx), PADV, dtype=T, device=_dev())
    x[:, :C] = case["x"].to(_dev())
    q, k, vt = (Buf(M * C, 1, T, pre=64, post=64) for _ in range(3))
    for b in (q, k, vt):
        b.freeze()
    a = dict(x=x.data_ptr(), ldx=ldx, wstream=stream.data_ptr(), vec=vec.data_ptr(), M=M, C=C, eps=EPS_NEXT, q=q.ptr(), k=k.ptr(), vt=vt.ptr(),
             qscale=QSCALE, heads=heads, hd=C // heads if heads else 0, Tp=Tp, dtype=_native.dtype_code(T))
    a.update(over or {})
    rc = _native.lib().lwdetr_vit_qkv(*[a[n] for n in ("x", "ldx", "wstream", "vec", "M", "C", "eps", "q", "k", "vt", "qscale", "heads", "hd", "Tp", "dtype")],
                                      _native.stream_ptr(_dev()))
    torch.cuda.synchronize()
    return rc, (q, k, vt), (x, stream, vec)


def check_qkv(bufs, case, M, C, T, heads, Tp, label):
    nb, hd = M // Tp, C // heads
    for name, b, tr in zip("qkv", bufs, (False, False, True)):
        assert b.guards_intact(0, 1), f"{label}: elements in front of / behind {name} were written"
        lay = lambda t: heads_layout(t, nb, Tp, heads, hd, tr)
        check2(b.body(0, 1).cpu().flatten(), lay(case["tight"][name][0]), lay(case["tight"][name][1]), lay(case["worst"][name][1]), T, f"{label} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("T,C,M,Tp,hd", _qkv_params())
def test_vit_qkv_vs_fp64(T, C, M, Tp, hd):
    from tests.helpers import vit_served_by
    case = qkv_case(C, M, T)
    with vit_served_by(f"vit_qkv_{_name(T)}_c{C}"):
        rc, bufs, _keep = run_qkv(case, C, M, T, C // hd, Tp, ldx=C + 8 if M == 40 else None)
    assert rc == 0
    check_qkv(bufs, case, M, C, T, C // hd, Tp, f"qkv {_name(T)}_c{C}")
    rc2, bufs2, _keep2 = run_qkv(case, C, M, T, C // hd, Tp, ldx=C + 8 if M == 40 else None)
    assert rc2 == 0 and all(torch.equal(a.buf.view(torch.uint8), b.buf.view(torch.uint8)) for a, b in zip(bufs, bufs2)), "a second launch differs"


# ------------------------------------------------------------------------------------------------------------ lwdetr_vit_stem
STEM_GEOM = [(1, 4, 4, 1), (1, 8, 4, 3), (3, 12, 8, 7), (2, 8, 8, 4)]       # (B, Hp, Wp, Twp)


def stem_tokens(B, Hp, Wp, Twp):
    """For every row of x (window-major, common.h:tok_decode): (image, patch y, patch x, valid)."""
    h, w = Hp // 4, Wp // 4
    r = torch.arange(B * 16 * Twp)
    b, rr = r // (16 * Twp), r % (16 * Twp)
    win, i = rr // Twp, rr % Twp
    iy, ix = i // w, i % w
    return b, (win // 4) * h + iy, (win % 4) * w + ix, i < h * w


def stem_case(C, geom, T, seed=5, img_seed=0):
    def build():
        B, Hp, Wp, Twp = geom
        W = make_weights(C, seed)
        g = torch.Generator().manual_seed(3000 + seed + C)
        wpe, bpe = torch.randn(C, 3, 16, 16, generator=g) / 768 ** 0.5, torch.randn(C, generator=g) * 0.3
        pos = (torch.randn(16 * Twp, C, generator=g) * 0.5).to(T)          # pad rows too: the kernel adds whatever the table holds
        gi = torch.Generator().manual_seed(4000 + img_seed)
        img = torch.randn(B, 3, 16 * Hp, 16 * Wp, generator=gi).to(T)
        D = dense_weights(W, T)
        D["wpe"], D["bpe"] = wpe.reshape(C, 768).to(T).double(), bpe.double()
        b, y, x, valid = stem_tokens(B, Hp, Wp, Twp)
        patches = img.double().reshape(B, 3, Hp, 16, Wp, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, Hp, Wp, 768)
        P = torch.zeros(B * 16 * Twp, 768, dtype=torch.float64)
        P[valid] = patches[b[valid], y[valid], x[valid]]
        M = B * 16 * Twp
        start = pos.double().repeat(B, 1) + D["bpe"]
        pre0 = start + P @ D["wpe"].t()
        res = {}
        for mode in ("tight", "worst"):
            e0 = acc_err(768, start.abs(), P.abs() @ D["wpe"].abs().t(), mode) + U23 * start.abs()
            x0, ex0, sx0, _ = round_stage(pre0, e0, torch.zeros_like(pre0), T, mode)
            res[mode] = dict(x=(pre0, e0), **qkv_tail(x0, ex0, sx0, D, T, EPS_NEXT, mode, chained=False))
        return dict(W=W, wpe=wpe, bpe=bpe, pos=pos, img=img, D=D, valid=valid, M=M, **res)
    return cached(("stem", C, geom, T, seed, img_seed), build)


def run_stem(case, C, geom, T, heads, img=None, over=None):
    from lwdetr_amd import kernels as K
    B, Hp, Wp, Twp = geom
    W, M = case["W"], case["M"]
    stream, vec = K.pack_vit_stem(case["wpe"], case["bpe"], W["wqkv"], W["qb"], W["vb"], W["ln1_w"], W["ln1_b"], T)
    stream, vec = stream.to(_dev()), vec.to(_dev())
    img = (case["img"] if img is None else img).to(_dev()).contiguous()
    pos = case["pos"].to(_dev()).contiguous()
    x = Buf(M, C, T); x.freeze()
    q, k, vt = (Buf(M * C, 1, T, pre=64, post=64) for _ in range(3))
    for b in (q, k, vt):
        b.freeze()
    a = dict(img=img.data_ptr(), B=B, img_h=16 * Hp, img_w=16 * Wp, Hp=Hp, Wp=Wp, Twp=Twp, pos=pos.data_ptr(), ldpos=C, x=x.ptr(), ldx=C,
             wstream=stream.data_ptr(), vec=vec.data_ptr(), M=M, C=C, eps=EPS_NEXT, q=q.ptr(), k=k.ptr(), vt=vt.ptr(), qscale=QSCALE, heads=heads,
             hd=C // heads if heads else 0, dtype=_native.dtype_code(T))
    a.update(over or {})
    rc = _native.lib().lwdetr_vit_stem(*[a[n] for n in ("img", "B", "img_h", "img_w", "Hp", "Wp", "Twp", "pos", "ldpos", "x", "ldx", "wstream", "vec", "M", "C",
                                                        "eps", "q", "k", "vt", "qscale", "heads", "hd", "dtype")], _native.stream_ptr(_dev()))
    torch.cuda.synchronize()
    return rc, (x, q, k, vt), (img, pos, stream, vec)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", STEM_GEOM, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("T,C,hd", [(F16, 192, 16), (BF16, 192, 64), (F16, 384, 32), (BF16, 384, 128)], ids=lambda v: str(v).split(".")[-1])
def test_vit_stem_vs_fp64(T, C, hd, geom):
    """Every row of x / q / k / v^T, pad rows included (the row of an all-zero patch: module docstring); pad rows do not depend on the image."""
    from tests.helpers import vit_served_by
    case = stem_case(C, geom, T)
    B, Hp, Wp, Twp = geom
    M, Tp, heads = case["M"], 16 * Twp, C // hd
    with vit_served_by(f"vit_stem_{_name(T)}_c{C}"):
        rc, (x, q, k, vt), _keep = run_stem(case, C, geom, T, heads)
    assert rc == 0
    label = f"stem {_name(T)}_c{C}"
    assert x.guards_intact(0, C), f"{label}: x rows beyond M were written"
    check2(x.body(0, C).cpu(), case["tight"]["x"][0], case["tight"]["x"][1], case["worst"]["x"][1], T, f"{label} x")
    for name, b, tr in zip("qkv", (q, k, vt), (False, False, True)):
        assert b.guards_intact(0, 1), f"{label}: elements in front of / behind {name} were written"
        lay = lambda t: heads_layout(t, B, Tp, heads, hd, tr)
        check2(b.body(0, 1).cpu().flatten(), lay(case["tight"][name][0]), lay(case["tight"][name][1]), lay(case["worst"][name][1]), T, f"{label} {name}")
    # a second launch is bit-identical; another image changes no pad row
    other = stem_case(C, geom, T, img_seed=1)["img"]
    rc2, (x2, q2, k2, vt2), _keep2 = run_stem(case, C, geom, T, heads)
    rc3, (x3, q3, k3, vt3), _keep3 = run_stem(case, C, geom, T, heads, img=other)
    assert rc2 == 0 and rc3 == 0
    for a, b in ((x, x2), (q, q2), (k, k2), (vt, vt2)):
        assert torch.equal(a.buf.view(torch.uint8), b.buf.view(torch.uint8)), f"{label}: a second launch differs"
    pad = ~case["valid"]
    if bool(pad.any()):
        rows = lambda b_, tr: (b_.body(0, 1).flatten().reshape(B, heads, hd, Tp).permute(0, 3, 1, 2) if tr
                               else b_.body(0, 1).flatten().reshape(B, heads, Tp, hd).permute(0, 2, 1, 3)).reshape(M, C).cpu()
        assert torch.equal(x.body(0, C).cpu()[pad].view(torch.int16), x3.body(0, C).cpu()[pad].view(torch.int16)), f"{label}: pad rows of x depend on the image"
        for a, b, tr in ((q, q3, False), (k, k3, False), (vt, vt3, True)):
            assert torch.equal(rows(a, tr)[pad].view(torch.int16), rows(b, tr)[pad].view(torch.int16)), f"{label}: pad rows of q / k / v^T depend on the image"
        assert not torch.equal(x.body(0, C).cpu()[~pad], x3.body(0, C).cpu()[~pad])


# ------------------------------------------------------------------------------------------------------------ sensitivity
SENS_C, SENS_M, SENS_TP, SENS_HD = 192, 40, 8, 32


def _sens_run(knobs, T=F16, **kw):
    _set_form(knobs, SENS_C, True, False)
    case = block_case(SENS_C, SENS_M, T, "f32")
    return case, BlockRun(case, SENS_C, SENS_M, T, qkv=True, extras=False, heads=SENS_C // SENS_HD, Tp=SENS_TP, **kw)


def fails_exactly(got, case, alt, T, label, dependent):
    """got: {name: (M, C) rows} computed with ONE altered operand; case: the reference of the original operands; alt: the reference of the altered
    ones; dependent: {name: (M, C) bool} the elements that depend on the altered value. The comparison with the ORIGINAL reference must fail on
    every dependent element whose reference moved by more than both tight bounds together, and on no element that does not depend on it."""
    total = 0
    for name in got:
        y, e = case["tight"][name]
        ya, ea = alt[name]
        dep = dependent.get(name, torch.zeros_like(y, dtype=torch.bool))
        fail = outside_tight(got[name], y, e, T)
        must = ((ya - y).abs() > bound_of(y, e, T) + bound_of(ya, ea, T)) & dep
        print(f"{label}: {name}: {int(fail.sum())} fail, {int(must.sum())} must, {int(dep.sum())} dependent")
        assert not bool((fail & ~dep).any()), f"{label}: {int((fail & ~dep).sum())} elements of {name} fail that do not depend on the altered value"
        assert bool((fail | ~must).all()), f"{label}: {int((must & ~fail).sum())} elements of {name} pass although their reference moved beyond the bound"
        total += int(must.sum())
    assert total > 0, f"{label}: the alteration moves no reference element beyond its bound - it tests nothing"


def quiet_channel(case, T):
    """The channel whose new rows have the tightest bound (a small |gamma2|: the MLP's share of the element is small)."""
    y, e = case["tight"]["x"]
    return int((bound_of(y, e, T) / half_ulp(y, T)).median(0).values.argmin())


def sens_bias(case, T, which):
    """(vec index, new f32 value, alt reference, dependent): one entry of b2 / bp / bqkv' raised by four output ulps of that channel's typical value."""
    D, C = case["D"], case["x"].shape[1]
    M = case["x"].shape[0]
    allrows, col = torch.ones(M, C, dtype=torch.bool), torch.zeros(M, C, dtype=torch.bool)
    if which == "bq":
        ch = C + 5                                                       # a k feature
        delta = float(8 * half_ulp(case["tight"]["k"][0][:, 5].abs().median(), T))
        col[:, 5] = True
        dep = dict(k=col)
    else:
        ch = quiet_channel(case, T)
        delta = float(8 * half_ulp(case["tight"]["x"][0][:, ch].abs().median(), T) / D["g2" if which == "b2" else "g1"][ch].abs())
        col[:, ch] = True
        # b2 moves the new rows in its channel; bp moves x1 there, and LayerNorm spreads that over the row; q / k / v follow from the whole row
        dep = dict(x=col if which == "b2" else allrows, q=allrows, k=allrows, v=allrows)
    newv = D[which].clone()
    newv[ch] = float(np.float32(float(newv[ch]) + delta))
    return _vec_section(C, which) + ch, float(newv[ch]), _alt_reference(case, T, **{which: newv}), dep


def sens_att(case, T):
    """(altered att, alt reference, dependent): one token of att moved by two ulps in one channel."""
    D, M, C = case["D"], case["x"].shape[0], case["x"].shape[1]
    att = case["att"].clone()
    ch = int((D["g1"][:, None] * D["wp"])[quiet_channel(case, T)].abs().argmax())     # the att channel the quiet output channel listens to most
    mag = att[:, ch].double().abs()
    mag[[0, M // 2, M - 1]] = 0                                           # (not one of the large-mean rows)
    tok = int(mag.argmax())
    v = att[tok, ch].double()
    att[tok, ch] = (v + 4 * half_ulp(v, T) * (1 if v >= 0 else -1)).to(T)
    assert att[tok, ch].double() != v
    row = torch.zeros(M, C, dtype=torch.bool)
    row[tok] = True
    return att, _alt_reference(case, T, att=att), dict(x=row, q=row, k=row, v=row)


def sens_swap(case, T, region):
    """(stream fragment indices to swap, alt reference, dependent): two 1 KB fragments inside Wp tile 0 (k-steps 0 and 1) / inside the first W2
    piece (output tiles 0 and 1 of its k-half 0 = hidden units 0 .. 15)."""
    D, M, C = case["D"], case["x"].shape[0], case["x"].shape[1]
    KS, NTI = C // 16, C // 32
    allrows = torch.ones(M, C, dtype=torch.bool)
    if region == "wp":
        w = D["wp"].clone()
        w[0:32, 0:16], w[0:32, 16:32] = D["wp"][0:32, 16:32], D["wp"][0:32, 0:16]
        return (0, 1), _alt_reference(case, T, wp=w), dict(x=allrows, q=allrows, k=allrows, v=allrows)
    piece = NTI + 2                                                      # pieces: Wp tiles, W1c(0), W1c(1), W2c(0), ...
    w = D["w2"].clone()
    w[0:32, :16], w[32:64, :16] = D["w2"][32:64, :16], D["w2"][0:32, :16]
    x_dep = torch.zeros(M, C, dtype=torch.bool)
    x_dep[:, :64] = True
    return (piece * KS, piece * KS + 1), _alt_reference(case, T, w2=w), dict(x=x_dep, q=allrows, k=allrows, v=allrows)


def sens_qscale(case, T):
    qs2 = QSCALE * (1 + 2.0 ** -7)
    r = float(np.float32(qs2)) / float(np.float32(QSCALE))
    alt = {n: case["tight"][n] for n in ("x", "k", "v")}
    alt["q"] = (case["tight"]["q"][0] * r, case["tight"]["q"][1] * r)
    return qs2, alt, dict(q=torch.ones_like(case["tight"]["q"][0], dtype=torch.bool))


def _alt_reference(case, T, **changes):
    D = dict(case["D"])
    att = changes.pop("att", case["att"])
    D.update(changes)
    return block_reference(case["x"], att, D, T, "f32", "tight")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["b2", "bp", "bq"])
def test_vit_block_sensitivity_one_bias_entry(which, knobs):
    """One entry of b2 / bp / bqkv' raised by four output ulps of that channel's typical value; the reference keeps the original."""
    case, run = _sens_run(knobs)
    idx, val, alt, dep = sens_bias(case, F16, which)
    vec = run.vec.clone()
    vec[idx] = val
    run.vec = vec
    assert run() == 0
    fails_exactly(block_outputs(run, which), case, alt, F16, f"sensitivity {which}", dep)


@pytest.mark.gpu
@pytest.mark.parametrize("region", ["wp", "w2"])
def test_vit_block_sensitivity_swapped_fragments(region, knobs):
    case, run = _sens_run(knobs)
    (a, b), alt, dep = sens_swap(case, F16, region)
    st = run.stream.clone().reshape(-1, 512)                             # fragments of 1 KB
    st[[a, b]] = st[[b, a]]
    run.stream = st.reshape(-1)
    assert run() == 0
    fails_exactly(block_outputs(run, region), case, alt, F16, f"sensitivity swap {region}", dep)


@pytest.mark.gpu
def test_vit_block_sensitivity_qscale(knobs):
    """qscale off by 2^-7 relative: only q fails."""
    case, _ = _sens_run(knobs)
    qs2, alt, dep = sens_qscale(case, F16)
    _, run = _sens_run(knobs, qscale=qs2)
    assert run() == 0
    fails_exactly(block_outputs(run, "qscale"), case, alt, F16, "sensitivity qscale", dep)


@pytest.mark.gpu
def test_vit_block_sensitivity_one_att_element(knobs):
    """One token of att moved by two ulps in one channel: only that token's row fails (and its q / k / v^T)."""
    case, _ = _sens_run(knobs)
    att, alt, dep = sens_att(case, F16)
    _, run = _sens_run(knobs, att=att)
    assert run() == 0
    fails_exactly(block_outputs(run, "att"), case, alt, F16, "sensitivity att", dep)


# ------------------------------------------------------------------------------------------------------------ refusals
def _refused(run, expect, label, **over):
    before = _native.vit_path_counts()
    rc = run(**over)
    assert rc == expect, f"{label}: rc {rc}, expected {expect}"
    assert _native.vit_path_counts() == before, f"{label}: the record moved"
    assert run.outputs_untouched(), f"{label}: an output was written"


@pytest.mark.gpu
def test_vit_block_refusals(knobs):
    T, C, M, Tp, hd = F16, 192, 40, 8, 32
    case = block_case(C, M, T, "f32")
    run = BlockRun(case, C, M, T, qkv=True, extras=True, heads=C // hd, Tp=Tp, ldx=C + 8, ldatt=C + 16)
    a = dict(zip(("x", "ldx", "att", "ldatt", "wstream", "vec", "out2", "ld2", "stats", "M", "C", "eps", "eps_next", "has_qkv", "q", "k", "vt", "qscale",
                  "heads", "hd", "Tp", "dtype"), run.args()))
    _refused(run, UNSUPPORTED, "M % 8", M=36)
    for n in ("ldx", "ldatt", "ld2"):
        _refused(run, BAD_ARG, f"{n} % 8", **{n: a[n] + 4})
        _refused(run, BAD_ARG, f"{n} < C", **{n: C - 8})
    for n in ("x", "att", "wstream", "vec", "out2", "stats", "q", "k", "vt"):
        _refused(run, BAD_ARG, f"{n} misaligned", **{n: a[n] + 2})
    _refused(run, UNSUPPORTED, "C = 256", C=256, ldx=256, ldatt=256, ld2=512, heads=8, M=8)
    _refused(run, UNSUPPORTED, "dtype f32", dtype=_native.dtype_code(torch.float32))
    _refused(run, UNSUPPORTED, "hd = 4", heads=48, hd=4)
    _refused(run, BAD_ARG, "hd = 24", heads=8, hd=24)
    _refused(run, BAD_ARG, "heads * hd != C", heads=5, hd=32)
    _refused(run, UNSUPPORTED, "Tp % 8 (Tp = 4)", Tp=4)
    _refused(run, BAD_ARG, "Tp % 4 (Tp = 10)", Tp=10)
    _refused(run, UNSUPPORTED, "M % Tp", Tp=16)
    _refused(run, BAD_ARG, "q / k overlap", k=a["q"] + 16)
    _refused(run, BAD_ARG, "k / vt overlap", vt=a["k"] + (M * C - 8) * 2)
    _refused(run, 0, "M = 0", M=0)


@pytest.mark.gpu
def test_vit_qkv_refusals():
    T, C, M, Tp, heads = BF16, 192, 40, 8, 6
    case = qkv_case(C, M, T)

    def refused(expect, label, **over):
        before = _native.vit_path_counts()
        rc, bufs, keep = run_qkv(case, C, M, T, heads, Tp, over=over)
        assert rc == expect, f"{label}: rc {rc}, expected {expect}"
        assert _native.vit_path_counts() == before and all(b.guards_intact() for b in bufs), f"{label}: something was written or counted"

    _, bufs, keep = run_qkv(case, C, M, T, heads, Tp)
    x, stream, vec = keep
    refused(UNSUPPORTED, "M % 8", M=36)
    refused(BAD_ARG, "ldx % 8", ldx=C + 4)
    refused(BAD_ARG, "ldx < C", ldx=C - 8)
    for n, t in (("x", x), ("wstream", stream), ("vec", vec)):
        refused(BAD_ARG, f"{n} misaligned", **{n: t.data_ptr() + 2})
    refused(UNSUPPORTED, "C = 256", C=256, ldx=256)
    refused(UNSUPPORTED, "dtype f32", dtype=_native.dtype_code(torch.float32))
    refused(UNSUPPORTED, "hd = 4", heads=48, hd=4)
    refused(UNSUPPORTED, "hd = 24", heads=8, hd=24)
    refused(UNSUPPORTED, "heads * hd != C", heads=5, hd=32)
    refused(UNSUPPORTED, "Tp % 8", Tp=4)
    refused(UNSUPPORTED, "M % Tp", Tp=16)
    refused(0, "M = 0", M=0)
    q2 = Buf(2 * M * C, 1, T, pre=64, post=64)
    refused(BAD_ARG, "q / k overlap", q=q2.ptr(), k=q2.ptr() + 64)
    for n in ("q", "k", "vt"):
        refused(BAD_ARG, f"{n} misaligned", **{n: q2.ptr() + 2})


@pytest.mark.gpu
def test_vit_stem_refusals():
    T, C, geom, heads = F16, 192, (1, 8, 4, 3), 6
    case = stem_case(C, geom, T)
    B, Hp, Wp, Twp = geom

    def refused(expect, label, **over):
        before = _native.vit_path_counts()
        rc, bufs, keep = run_stem(case, C, geom, T, heads, over=over)
        assert rc == expect, f"{label}: rc {rc}, expected {expect}"
        assert _native.vit_path_counts() == before and all(b.guards_intact() for b in bufs), f"{label}: something was written or counted"

    refused(BAD_ARG, "img_h != 16 Hp", img_h=16 * Hp - 16)
    refused(BAD_ARG, "Hp % 4", Hp=6, img_h=96)
    refused(BAD_ARG, "Twp < (Hp/4)(Wp/4)", Twp=1, M=16)
    refused(BAD_ARG, "M != B 16 Twp", M=case["M"] - 8)
    refused(BAD_ARG, "ldx % 8", ldx=C + 4)
    refused(BAD_ARG, "ldpos < C", ldpos=C - 8)
    refused(UNSUPPORTED, "C = 256", C=256, ldx=256, ldpos=256)
    refused(UNSUPPORTED, "dtype f32", dtype=_native.dtype_code(torch.float32))
    refused(UNSUPPORTED, "hd = 4", heads=48, hd=4)
    refused(UNSUPPORTED, "heads * hd != C", heads=5, hd=32)
    refused(0, "M = 0", M=0)
    _, bufs, keep = run_stem(case, C, geom, T, heads)
    img, pos, stream, vec = keep
    for n, t in (("img", img), ("pos", pos), ("wstream", stream), ("vec", vec)):
        refused(BAD_ARG, f"{n} misaligned", **{n: t.data_ptr() + 2})
    q2 = Buf(2 * case["M"] * C, 1, T, pre=64, post=64)
    refused(BAD_ARG, "q / vt overlap", q=q2.ptr(), vt=q2.ptr() + 64)
    for n in ("x", "q", "k", "vt"):
        refused(BAD_ARG, f"{n} misaligned", **{n: q2.ptr() + 2})


# ------------------------------------------------------------------------------------------------------------ the record, at the end
@pytest.mark.gpu
@pytest.mark.parametrize("T", [F16, BF16], ids=_name)
def test_vit_every_instantiation_was_launched(T):
    """After this module every instantiation the record names has a non-zero count (this test runs last in the module)."""
    counts = _native.vit_path_counts()
    mine = {k: v for k, v in counts.items() if f"_{_name(T)}_" in k}
    assert len(mine) == {F16: 12 + 4, BF16: 6 + 4}[T], sorted(mine)
    assert all(v > 0 for v in mine.values()), {k: v for k, v in mine.items() if v == 0}
