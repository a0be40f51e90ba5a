"""The kernels of csrc/msda.hip (lwdetr_msda_forward, lwdetr_msda_fused_forward, lwdetr_msda_backward), called directly through the C ABI at the
smallest shapes at which their work split, level / head / channel-group indexing, border handling and launch forms can go wrong. Every launch is
pinned to ONE instantiation by the launch-form record (lwdetr_msda_path_counts, helpers.msda_served_by) and every output is checked ELEMENT BY
ELEMENT against a float64 evaluation of the same operation on the operands as stored (16-bit inputs widened exactly, the f32 ref_boxes /
valid_ratios as f32 numbers). Outputs (forward out, grad_loc, grad_aw) live in larger buffers whose guard rows, filled with a sentinel, must come
back bit-identical. tests/test_gpu_msda.py (goldens, the C restatement of the reference's kernels, gradcheck) stays as the cross-check; nothing
here calls oracle/msda_c or O.msda_core.

Reference (the definition in include/lwdetr_hip.h). h_im = loc_y H - 0.5, w_im = loc_x W - 0.5; a sample contributes iff h_im > -1 && w_im > -1 &&
h_im < H && w_im < W (so a sample with a non-finite location contributes nothing); hl = floor(h_im), lh = h_im - hl, hh = 1 - lh (w alike); the four
corners (hl, wl) (hl, wl + 1) (hl + 1, wl) (hl + 1, wl + 1) with weights hh hw, hh lw, lh hw, lh lw, a corner outside the map reading 0;
out[b, q, m D + c] = sum_{l, p} a[b, q, m, l, p] bilinear(value[b, level l, :, m, c]). Fused form: per level l, vr = valid_ratios[b, l] = (vx, vy),
loc = ref_xy vr + off / P (ref_wh vr) 0.5 and a = softmax over the L P logits of a (row, head). Backward: the derivatives of that sum.

Bound. The stored number may differ from the float64 y by half_ulp_T(|y| + E) + E (half_ulp of test_gpu_rowops; float64 storage: its own spacing),
E = E1 + E2 + E3 per element from the reference's own numbers, u = 2^-24 (one f32 rounding), U23 = 2 u; float64 kernels: 2^-53 / 2^-52:
  E1, f32 accumulation: n U23 S, S = sum_k |w_k v_k| of THAT element over its 4 L P corner terms. vec8 / fused (sample_level): 4 L P fmas onto the
    accumulator + the 4 roundings of a corner weight (hh, hw, hh hw, . a): n = 4 L P + 4. generic: a sample's value is 3 roundings for a weight, one
    product, 3 additions, one product with a, then at most L P additions onto col: n = L P + 8.
  E2, location arithmetic. h_im^ = fl(fl(loc_y H) - 0.5) (or one fma): |d h_im| <= u (|loc_y| H + |h_im|), w alike. Fused: cy = fl(ry vy),
    bh = fl(rh vy), t = fl(oy / P bh) 0.5 (the divisions by P = 2, 4 and the halving are exact), loc_y = fl(cy + t):
    |d loc_y| <= u (|cy| + 2 |t| + |loc_y|) and |d h_im| <= H |d loc_y| + u (|loc_y| H + |h_im|). Bilinear sampling with zero padding is
    continuous in the location and bilinear inside a cell, so a sample's value moves by at most |dh| |f_h| + |dw| |f_w| + |dh| |dw| |f_hw| with
    f_h = hw (v3 - v1) + lw (v4 - v2), f_w = hh (v2 - v1) + lh (v4 - v3), f_hw = v1 - v2 - v3 + v4 from the reference's (zero-padded) corner values
    - exact while both evaluations are in the same cell. + 5 % on top. That they are in the same cell is a CONDITION ON THE INPUTS, asserted by the
    case builders: every sample is either `exact` (its f32 location arithmetic reproduces the float64 numbers: the engineered samples, which
    include the cell edges and the -1 / H borders themselves) or at least 8 U23 max(H, W) away from every integer h_im / w_im;
  E3, fused softmax: a = e_i / sum, e_i = __expf(l_i - mx) = v_exp_f32((l_i - mx) log2 e). The exponent t = l_i - mx <= 0 carries the roundings of
    the subtraction, of the product and of log2 e (3 u |t| on e_i), a fl(e_i inv) adds u: rel(e_i) = C1 U23 (1 + |t_i|) + TRANS_F32, C1 = 2;
    rel(sum) = sum_j a_j rel(e_j) + L P U23; inv = 1.f / sum: TRANS_F32 more. |d a_i| <= a_i (rel(e_i) + rel(sum) + TRANS_F32) + 2^-125 (an
    exponential below 2^-126 may come back as 0). E3 = sum_k |d a_k| (sum of the |w v| of sample k).
  Backward (lwdetr_msda_backward, T = f32 / f64 arithmetic throughout): grad_value[e]: (number of contributions to e + 1) U23 sum |contributions|,
    both scatter-added from the reference; grad_loc / grad_aw: (ceil(D / GS) + log2 GS + 7) U23 sum |terms|, GS = min(64, pow2(D)) lanes per item,
    7 = the roundings of one channel's term (4 corner updates, tg a, the W / H scale, the product); float64: 2^-52 for U23. These have NO location
    term: the backward cases draw their random locations from the grid of multiples of 2^-12, on which loc W - 0.5, lh, hh are exact in f32 for
    W <= 8, so the f32 and float64 evaluations differ by the roundings counted above only. Two more f32 cases (`full`) take locations with every
    mantissa bit, so that the kernel's loc W - 0.5, lh and hh round: their bounds add the location term |d h_im| <= u (|loc_y| H + |h_im|) through
    the derivatives of each output (a corner weight wy wx moves by dh wx + dw wy + dh dw; grad_aw as E2; d grad_loc_x = W |a tg| dh |f_hw|, y alike;
    + 5 %) and one more U23 for fl(1 - lh), fl(1 - lw). grad_loc is discontinuous in the location at cell edges: the builders, and the test before
    its launch, assert the same distance condition as above on every sample that is not engineered (no exemption by f32 exactness here).
No term is scaled by a tensor-wide maximum; every element must meet its bound.

Hardware transcendentals: TRANS_F32 = 4 TRANS_MEASURED (the margin of test_gpu_vitblock.py: another valid input set moves such a figure by that
much). __expf and the reciprocal are VISIBLE here through the weights, so they are measured: test_msda_fused_softmax_weights_measured runs value
maps that are 1 at one pixel per (level, point) with every sample aimed exactly at its pixel's centre, so that output channel l P + p IS the
softmax weight, in f32, logits within [-1, 1] (|t| <= 2: the exponent's own roundings stay below two ulp). Measured on an MI355X, worst relative
deviation of a weight from the float64 softmax of the stored logits over 512 (row, head)s per form: 1.440 (l1p2), 2.166 (l1p4), 2.385 (l2p2),
2.216 (l2p4) x 2^-23 (profiles/r8b_msda_fp64_worst_ratios.txt). TRANS_MEASURED is the larger of that and one f32 ulp: 2.385 x 2^-23 (the raw
figure, the exponent's roundings included - they are counted again in C1, on the safe side).

What the norm-wise assertions of test_gpu_msda.py accept: max |diff| < tol max |ref| lets one wrong (query, head) out of hundreds of small ones
pass; tests/test_msda_bound_host.py shows on the CPU, on exactly these cases, that an independent f32 evaluation stays inside this module's bound
and that each of twelve planted indexing / border / scale mistakes leaves it.
"""
import math

import numpy as np
import pytest
import torch

from lwdetr_amd import _native
from tests import test_gpu_rowops as R
from tests.test_gpu_rowops import U23, SENT, F16, BF16, F32

F64 = torch.float64
NAME = {F32: "f32", F16: "f16", BF16: "bf16", F64: "f64"}
U52 = 2.0 ** -52
TRANS_MEASURED = 2.385 * 2.0 ** -23   # the larger of the measured deviation of a softmax weight (module docstring) and one f32 ulp
TRANS_F32 = 4 * TRANS_MEASURED
C1 = 2.0
FLUSH = 2.0 ** -125
BIG = 30000.0                 # fills the padding / gap columns of oa: finite in every type, must never be read
BAD_ARG, UNSUPPORTED = _native.ERR_BAD_ARG, _native.ERR_UNSUPPORTED
PFX = "msda"


def urt(T):
    """2 u of the arithmetic type of T's kernels (f32 for f32 / f16 / bf16)."""
    return U52 if T == F64 else U23


def half_ulp(v, T):
    if T == F64:
        return np.spacing(np.abs(v)) / 2
    return R.half_ulp(torch.from_numpy(np.ascontiguousarray(v)), T).numpy()


def bound_of(y, e, T):
    return half_ulp(np.abs(y) + e, T) + e


def store(a, T):
    """float64 numpy -> torch tensor of T (one rounding)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(T)


def wide(t):
    return t.double().numpy()


_CACHE = {}


def cached(key, fn):
    """Cases and references are computed once and shared between the tests that need them; nothing modifies them."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ sampling in float64
def level_table(levels):
    shapes = np.array(levels, dtype=np.int64).reshape(-1, 2)
    sizes = shapes[:, 0] * shapes[:, 1]
    lsi = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return shapes, lsi, int(sizes.sum())


def sample_parts(value, levels, loc, mut=()):
    """Per level: the geometry and the four zero-padded corner values of every sample. value (B, S, M, D), loc (B, Q, M, L, P, 2) float64.
    `mut`: planted mistakes (tests/test_msda_bound_host.py)."""
    B, S, M, D = value.shape
    _, lsi, _ = level_table(levels)
    bI = np.arange(B).reshape(B, 1, 1, 1)
    if "image_plus8" in mut:
        bI = (bI + 8) % B
    mI = np.arange(M).reshape(1, 1, M, 1)
    parts = []
    half = 0.0 if "no_half" in mut else 0.5
    for l, (H, W) in enumerate(levels):
        x, y = loc[:, :, :, l, :, 0], loc[:, :, :, l, :, 1]
        with np.errstate(invalid="ignore"):
            h_im, w_im = y * H - half, x * W - half
            inside = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
        hs, ws = np.where(inside, h_im, 0.0), np.where(inside, w_im, 0.0)
        hl, wl = np.floor(hs), np.floor(ws)
        lh, lw = hs - hl, ws - wl
        if "swap_lhlw" in mut:
            lh, lw = lw, lh
        hl, wl = hl.astype(np.int64), wl.astype(np.int64)
        start = int(lsi[l]) + (1 if ("level_start_plus1" in mut and l == len(levels) - 1) else 0)
        v, idx, ok = [], [], []
        for dh, dw in ((0, 0), (0, 1), (1, 0), (1, 1)):
            hi, wi = hl + dh, wl + dw
            valid = inside & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
            if "replicate" in mut:
                valid = inside
            i = np.minimum(start + np.clip(hi, 0, H - 1) * W + np.clip(wi, 0, W - 1), S - 1)
            v.append(value[bI, i, mI] * valid[..., None])
            idx.append(i)
            ok.append(valid)
        parts.append(dict(H=H, W=W, inside=inside, lh=lh, lw=lw, v=v, idx=idx, ok=ok, h_im=h_im, w_im=w_im, x=x, y=y))
    return parts


def corner_weights(pt):
    lh, lw = pt["lh"], pt["lw"]
    hh, hw = 1 - lh, 1 - lw
    return [hh * hw, hh * lw, lh * hw, lh * lw]


def forward_sum(value, levels, loc, a, da, dloc, n_acc, T, mut=()):
    """y (B, Q, M D) and the bound of a stored T result. a, da (B, Q, M, L, P): weights and their deviation; dloc (B, Q, M, L, P, 2): |d w_im|, |d h_im|."""
    B, S, M, D = value.shape
    Q = loc.shape[1]
    y, S1, E2, E3 = (np.zeros((B, Q, M, D)) for _ in range(4))
    for l, pt in enumerate(sample_parts(value, levels, loc, mut)):
        w = corner_weights(pt)
        v1, v2, v3, v4 = pt["v"]
        lh, lw = pt["lh"][..., None], pt["lw"][..., None]
        val = sum(wk[..., None] * vk for wk, vk in zip(w, pt["v"]))
        aval = sum(wk[..., None] * np.abs(vk) for wk, vk in zip(w, pt["v"]))
        al = a[:, :, :, l, :, None]
        ins = pt["inside"][..., None]
        dw_, dh_ = (np.where(pt["inside"], dloc[:, :, :, l, :, k], 0.0)[..., None] for k in (0, 1))
        f_h = (1 - lw) * (v3 - v1) + lw * (v4 - v2)
        f_w = (1 - lh) * (v2 - v1) + lh * (v4 - v3)
        f_hw = v1 - v2 - v3 + v4
        y += np.where(ins, al * val, 0.0).sum(3)
        S1 += np.where(ins, np.abs(al) * aval, 0.0).sum(3)
        E2 += np.where(ins, np.abs(al) * (dh_ * np.abs(f_h) + dw_ * np.abs(f_w) + dh_ * dw_ * np.abs(f_hw)), 0.0).sum(3)
        E3 += np.where(ins, da[:, :, :, l, :, None] * aval, 0.0).sum(3)
    if "transpose_head_group" in mut:            # head and channel group transposed in the output index (D = 8 G)
        G = D // 8
        y = y.reshape(B, Q, M, G, 8).transpose(0, 1, 3, 2, 4).reshape(B, Q, M, D)
    E = n_acc * urt(T) * S1 + 1.05 * E2 + E3
    y, E = y.reshape(B, Q, M * D), E.reshape(B, Q, M * D)
    return y, bound_of(y, E, T)


def plain_dloc(loc, levels, T):
    u = urt(T) / 2
    d = np.zeros_like(loc)
    with np.errstate(invalid="ignore"):
        for l, (H, W) in enumerate(levels):
            for k, n in ((0, W), (1, H)):
                d[:, :, :, l, :, k] = u * (np.abs(loc[:, :, :, l, :, k]) * n + np.abs(loc[:, :, :, l, :, k] * n - 0.5))
    return d


def n_acc(form, L, P):
    return L * P + 8 if form.startswith("msda_generic") else 4 * L * P + 4


# ------------------------------------------------------------------------------------------------------------ engineered locations
def _pow2(n):
    return n & (n - 1) == 0


def step_in(t, n=1):
    """The T number n steps nearer to zero than t (|t| > 0)."""
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return (t.view(it) - n).view(t.dtype)


def engineered(H, W, T, coarse=False):
    """(x, y) locations of T whose f32 arithmetic loc n - 0.5 is exact, as float64 pairs: pixel centres, lh == 0, the -1 / H borders themselves,
    loc 0 / 1, just inside each border (two T steps: -1 + 2^-24 is an f32 number, -1 + 2^-25 is not; coarse: 2^-6, for offsets of few bits), one axis outside, far outside."""
    one = lambda v: float(store(np.array([v]), T).double()[0])
    inn = (lambda v: v - math.copysign(2.0 ** -6, v)) if coarse else (lambda v: float(step_in(store(np.array([v]), T), 2).double()[0]))
    pts = [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.5, 0.5), (3.0, 3.0), (-3.0, -3.0), (3.0, 0.5), (0.5, 1.5), (-0.5, 0.5)]
    xs = [(0.5 / W, -0.5 / W, 1 + 0.5 / W, (W - 0.5) / W)] if _pow2(W) else []
    ys = [(0.5 / H, -0.5 / H, 1 + 0.5 / H, (H - 0.5) / H)] if _pow2(H) else []
    if xs and ys:
        (xc, xlo, xhi, xl), (yc, ylo, yhi, yl) = xs[0], ys[0]
        pts += [(xc, yl), (xl, yc), (one(0.3), yc), (xc, one(0.3)),                 # pixel centres; lh == 0; lw == 0
                (xc, ylo), (xlo, yc), (xc, yhi), (xhi, yc), (xlo, ylo), (xhi, yhi),   # exactly on the -1 / H / W borders: outside
                (xc, inn(ylo)), (inn(xlo), yc), (xc, inn(yhi)), (inn(xhi), yc), (inn(xlo), inn(yhi))]   # just inside each border
    return [(one(x), one(y)) for x, y in pts]


def f32_exact(loc, n):
    """Is loc n - 0.5 reproduced exactly by f32 arithmetic (product and difference both representable)?"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = loc * n
        return (p.astype(np.float32).astype(np.float64) == p) & ((p - 0.5).astype(np.float32).astype(np.float64) == p - 0.5)


def assert_locations_safe(loc, levels, exempt, what, f32_exempt, unit=U23):
    """The condition on the inputs of the module docstring: a sample is exempt (engineered), or - only where `f32_exempt` says that the kernel's
    location arithmetic is the plain f32 loc n - 0.5 - reproduced exactly by f32, or 8 unit max(H, W) away from every cell edge and from the
    -1 / H borders (the integers of h_im / w_im) in both axes. unit: U23, or 2^-52 for a kernel that computes in float64."""
    dist = 8 * unit
    for l, (H, W) in enumerate(levels):
        for k, n in ((0, W), (1, H)):
            c = loc[:, :, :, l, :, k]
            with np.errstate(invalid="ignore"):
                im = c * n - 0.5
                near = np.abs(im - np.round(im)) <= dist * max(H, W)
                relevant = (im > -2) & (im < n + 1)
            ok = ~(near & relevant) | exempt[:, :, :, l, :] | ~np.isfinite(c)
            if f32_exempt:
                ok |= f32_exact(c, n)
            assert bool(ok.all()), f"{what}: {int((~ok).sum())} samples of level {l} within {dist * max(H, W):.2e} of a cell edge"


# ------------------------------------------------------------------------------------------------------------ forward operator cases
def fwd_case(T, B, Q, M, D, P, levels, seed=0, nonfinite=False):
    return cached(("fwd", T, B, Q, M, D, P, tuple(levels), seed, nonfinite), lambda: _fwd_case(T, B, Q, M, D, P, levels, seed, nonfinite))


def _fwd_case(T, B, Q, M, D, P, levels, seed, nonfinite):
    L = len(levels)
    shapes, lsi, S = level_table(levels)
    for attempt in range(64):                       # the first seed whose random samples meet the distance condition
        g = np.random.default_rng(7919 * seed + 104729 * attempt + B * 1000 + Q * 10 + D + P)
        value = store(g.standard_normal((B, S, M, D)), T)             # every image its own map
        loc = g.uniform(-0.15, 1.15, (B, Q, M, L, P, 2))
        aw = g.standard_normal((B, Q, M, L, P)) * 0.6
        exempt = np.zeros((B, Q, M, L, P), dtype=bool)
        for l, (H, W) in enumerate(levels):          # engineered samples: images 0 and B - 1, one per (q, m, p) slot of level l, weight 1
            for b in {0, B - 1}:
                for i, (x, y) in enumerate(engineered(H, W, T)):
                    q, m, p = (i // (M * P)) % Q, (i // P) % M, i % P
                    loc[b, q, m, l, p] = (x, y)
                    aw[b, q, m, l, p] = 1.0 if (i + b) % 2 == 0 else -1.0
                    exempt[b, q, m, l, p] = True
        if nonfinite:                                # one (b, q, m) each; the other samples of the item are ordinary
            b, q = B - 1, Q - 1
            loc[b, q, 0, 0, 0, 0] = np.inf
            loc[b, q, 1, L - 1, P - 1, 1] = -np.inf
            loc[b, q - 1, M - 1, 0, 0] = np.nan
            aw[b, q, 0, 0, 0] = aw[b, q, 1, L - 1, P - 1] = aw[b, q - 1, M - 1, 0, 0] = 1.0
        loc_t, aw_t = store(loc, T), store(aw, T)
        locw = wide(loc_t)
        try:
            assert_locations_safe(locw, levels, exempt, "forward case", f32_exempt=T != F64, unit=urt(T))
            break
        except AssertionError:
            continue
    else:
        raise AssertionError("no seed met the distance condition")
    if T != F64:
        for l, (H, W) in enumerate(levels):
            e = exempt[:, :, :, l, :]
            assert bool((f32_exact(locw[:, :, :, l, :, 0], W) & f32_exact(locw[:, :, :, l, :, 1], H))[e].all()), "an engineered sample is not exact in f32"
    return dict(T=T, B=B, Q=Q, M=M, D=D, P=P, L=L, S=S, levels=list(levels), shapes=shapes, lsi=lsi, value=value, loc=loc_t, aw=aw_t,
                exempt=exempt)


def fwd_reference(case, form, mut=()):
    def build():
        T, L, P = case["T"], case["L"], case["P"]
        loc = wide(case["loc"])
        a = wide(case["aw"])
        return forward_sum(wide(case["value"]), case["levels"], loc, a, np.zeros_like(a), plain_dloc(loc, case["levels"], T), n_acc(form, L, P), T, mut)
    return cached(("fwd_ref", id(case), form, tuple(mut)), build)


LV1, LV2, LV3 = [(5, 7)], [(5, 7), (1, 3)], [(4, 8), (1, 3), (1, 1)]
PFORM = {1: "n", 2: "2", 3: "n", 4: "4", 8: "n"}
# (B, Q, M, D, P, levels): per_img = Q M D / 8 = 111 / 222 / 333 / 256; B = 3 (no remap), 8, 16 (remap; images 8 ... 15 behind slot / chunks == 1)
VEC8_SHAPES = [(3, 37, 3, 8, 1, LV3), (8, 37, 3, 16, 2, LV2), (16, 37, 3, 24, 3, LV3), (3, 32, 4, 16, 4, LV1), (8, 37, 3, 16, 8, LV3), (16, 37, 3, 8, 4, LV2),
               (3, 37, 3, 24, 2, LV3)]
GENERIC_SHAPES = [(F16, 3, 37, 3, 16, 9, LV2), (F32, 3, 37, 3, 5, 2, LV3), (F16, 8, 37, 3, 5, 3, LV2), (BF16, 3, 37, 3, 5, 1, LV3), (F64, 3, 37, 3, 16, 2, LV3),
                  (F64, 2, 37, 3, 5, 4, LV1)]


def fwd_params():
    out = [pytest.param(T, *s, f"msda_vec8_{NAME[T]}_p{PFORM[s[4]]}", id=f"vec8-{NAME[T]}-B{s[0]}-D{s[3]}-P{s[4]}-L{len(s[5])}") for T in (F32, F16, BF16) for s in VEC8_SHAPES]
    out += [pytest.param(*s, f"msda_generic_{NAME[s[0]]}", id=f"generic-{NAME[s[0]]}-B{s[1]}-D{s[4]}-P{s[5]}-L{len(s[6])}") for s in GENERIC_SHAPES]
    return out


NONFINITE = [(F32, 3, 37, 3, 16, 2, LV2, "msda_vec8_f32_p2"), (F16, 8, 37, 3, 8, 3, LV3, "msda_vec8_f16_pn"), (BF16, 3, 37, 3, 16, 4, LV1, "msda_vec8_bf16_p4"),
             (F32, 3, 37, 3, 5, 2, LV2, "msda_generic_f32"), (F16, 3, 37, 3, 5, 3, LV3, "msda_generic_f16")]


# ------------------------------------------------------------------------------------------------------------ fused cases
def fused_case(T, B, Q, M, D, L, P, levels, seed=0, nonfinite=False, measure=False):
    return cached(("fused", T, B, Q, M, D, L, P, tuple(levels), seed, nonfinite, measure), lambda: _fused_case(T, B, Q, M, D, L, P, levels, seed, nonfinite, measure))


def fused_locations(case, mut=()):
    """float64 loc (B, Q, M, L, P, 2), its f32 deviation bound, the weights and their deviation bound, from the stored operands."""
    B, Q, M, L, P = (case[k] for k in "BQMLP")
    mlp = M * L * P
    oa = wide(case["oa"]).reshape(B, Q, -1)
    off = oa[:, :, :2 * mlp].reshape(B, Q, M, L, P, 2)
    col = case["logit_col"] - (8 if "logit_col_minus8" in mut else 0)
    lg = oa[:, :, col:col + mlp].reshape(B, Q, M, L * P)
    ref = case["ref"].astype(np.float64)          # f32 numbers
    vr = case["vr"].astype(np.float64)
    if "vx_vy" in mut:
        vr = vr[:, :, ::-1]
    u = U23 / 2
    loc, dloc = np.zeros((B, Q, M, L, P, 2)), np.zeros((B, Q, M, L, P, 2))
    div = L * P if "div_LP" in mut else P
    with np.errstate(invalid="ignore"):
        for l, (H, W) in enumerate(case["levels"]):
            for k, n in ((0, W), (1, H)):
                c = (ref[:, :, k] * vr[:, None, l, k])[:, :, None, None]
                bw = (ref[:, :, 2 + k] * vr[:, None, l, k])[:, :, None, None]
                t = off[:, :, :, l, :, k] / div * bw * 0.5
                x = c + t
                loc[:, :, :, l, :, k] = x
                dloc[:, :, :, l, :, k] = n * u * (np.abs(c) + 2 * np.abs(t) + np.abs(x)) + u * (np.abs(x) * n + np.abs(x * n - 0.5))
    if "softmax_P" in mut:
        lgp = lg.reshape(B, Q, M, L, P)
        tt = lgp - lgp.max(-1, keepdims=True)
        a = (np.exp(tt) / np.exp(tt).sum(-1, keepdims=True)).reshape(B, Q, M, L * P)
        tt = tt.reshape(B, Q, M, L * P)
    else:
        tt = lg - lg.max(-1, keepdims=True)
        a = np.exp(tt) / np.exp(tt).sum(-1, keepdims=True)
    rel_e = C1 * U23 * (1 + np.abs(tt)) + TRANS_F32
    rel_sum = (a * rel_e).sum(-1, keepdims=True) + L * P * U23
    da = a * (rel_e + rel_sum + TRANS_F32) + FLUSH
    return loc, dloc, a.reshape(B, Q, M, L, P), da.reshape(B, Q, M, L, P)


def _fused_case(T, B, Q, M, D, L, P, levels, seed, nonfinite, measure):
    assert len(levels) == L
    shapes, lsi, S = level_table(levels)
    mlp = M * L * P
    logit_col, ld_oa = 2 * mlp + 8, 2 * mlp + 8 + mlp + 8
    for attempt in range(64):
        g = np.random.default_rng(6007 * seed + 15485863 * attempt + B * 1000 + Q * 10 + D + 7 * L + P)
        value = g.standard_normal((B, S, M, D))
        off = g.standard_normal((B, Q, M, L, P, 2)) * 2.0
        ref = np.stack([g.uniform(0.1, 0.9, (B, Q)), g.uniform(0.1, 0.9, (B, Q)), g.uniform(0.1, 0.6, (B, Q)), g.uniform(0.1, 0.6, (B, Q))], -1).astype(np.float32)
        vr = g.uniform(0.55, 1.0, (B, L, 2)).astype(np.float32)     # differ per image, per level and between w and h
        spread = np.where(g.uniform(size=(B, Q, M, 1)) < 0.5, 0.3, 4.0)          # flat and peaked (row, head)s
        lg = g.standard_normal((B, Q, M, L * P)) * spread
        lg[:, :, :, 0] += np.where(spread[..., 0] > 1, 9.0 * (g.uniform(size=(B, Q, M)) < 0.5), 0.0)      # a spread of 8 or more
        lg[B - 1, 1] = 0.75                                          # one row with all logits equal
        exempt = np.zeros((B, Q, M, L, P), dtype=bool)
        if measure:                  # the value map is 1 at pixel p of level l in channel l P + p; every sample aimed at its pixel's centre
            assert D == 8 and L * P <= 8 and all(_pow2(h) and _pow2(w) and h * w >= P for h, w in levels)
            value[:] = 0.0
            ref[:] = (0.5, 0.5, 1.0, 1.0)
            vr[:] = 1.0
            lg = g.standard_normal((B, Q, M, L * P)) * g.uniform(0.2, 2.0, (B, Q, M, 1))
            lg = np.clip(lg, -1, 1)
            for l, (H, W) in enumerate(levels):
                for p in range(P):
                    value[:, lsi[l] + p, :, l * P + p] = 1.0
                    off[:, :, :, l, p, 0] = 2 * P * ((p % W + 0.5) / W - 0.5)
                    off[:, :, :, l, p, 1] = 2 * P * ((p // W + 0.5) / H - 0.5)
            exempt[:] = True
        else:
            if T == F32:
                lg[B - 1, 2, :, :] = np.array([0.0, -120.0, -150.0, -101.0, -200.0, -130.0, -110.0, -170.0])[:L * P]     # most exponentials underflow
            # engineered rows of image 0: box (0.5, 0.5, 0.5, 0.25), valid ratios (1, 0.5) -> off = (4 P (x - 0.5), 16 P (y - 0.25)), exact in T
            vr[0] = (1.0, 0.5)
            for l, (H, W) in enumerate(levels):
                for i, (x, y) in enumerate(engineered(H, W, T, coarse=True)):
                    q, m, p = (i // (M * P)) % Q, (i // P) % M, i % P
                    o = np.array([4 * P * (x - 0.5), 16 * P * (y - 0.25)])
                    if not np.array_equal(wide(store(o, T)), o):
                        continue
                    ref[0, q] = (0.5, 0.5, 0.5, 0.25)
                    off[0, q, m, l, p] = o
                    lg[0, q, m] = lg[0, q, m] * 0.05
                    exempt[0, q, m, l, p] = True
            assert int(exempt.sum()) >= 6 * L, "too few engineered samples are representable"
        if nonfinite:
            b, q = B - 1, Q - 1
            off[b, q, 0, 0, 0, 0] = np.inf
            off[b, q, 1, L - 1, P - 1, 1] = -np.inf
            off[b, q - 1, M - 1, 0, 0] = np.nan
            lg[b, q, 0] = lg[b, q, 1] = lg[b, q - 1, M - 1] = 0.25
        oa = np.full((B * Q, ld_oa), BIG)
        oa[:, :2 * mlp] = off.reshape(B * Q, -1)
        oa[:, logit_col:logit_col + mlp] = lg.reshape(B * Q, -1)
        case = dict(T=T, B=B, Q=Q, M=M, D=D, L=L, P=P, S=S, levels=list(levels), shapes=shapes, lsi=lsi, value=store(value, T), oa=store(oa, T), ref=ref, vr=vr,
                    logit_col=logit_col, ld_oa=ld_oa, exempt=exempt)
        loc, dloc, a, da = fused_locations(case)
        try:
            assert_locations_safe(loc, levels, exempt, "fused case", f32_exempt=False)       # (no exemption by f32 exactness: the arithmetic is longer)
            break
        except AssertionError:
            continue
    else:
        raise AssertionError("no seed met the distance condition")
    # the engineered samples: f32 evaluation of the kernel's expression reproduces the float64 location
    f = np.float32
    o32, r32, v32 = wide(case["oa"]).reshape(B, Q, -1)[:, :, :2 * mlp].reshape(B, Q, M, L, P, 2).astype(f), ref, vr
    for l, (H, W) in enumerate(levels):
        for k, n in ((0, W), (1, H)):
            with np.errstate(invalid="ignore", over="ignore"):
                c = (r32[:, :, k] * v32[:, None, l, k])[:, :, None, None]
                bw = (r32[:, :, 2 + k] * v32[:, None, l, k])[:, :, None, None]
                x = (c + o32[:, :, :, l, :, k] / f(P) * bw * f(0.5)).astype(f)
                im = (x * f(n)).astype(f) - f(0.5)
                e = exempt[:, :, :, l, :]
                assert np.array_equal(im.astype(np.float64)[e], (loc[:, :, :, l, :, k] * n - 0.5)[e]), "an engineered sample is not exact in f32"
    return case


def fused_reference(case, mut=()):
    def build():
        loc, dloc, a, da = fused_locations(case, mut)
        return forward_sum(wide(case["value"]), case["levels"], loc, a, da, dloc, 4 * case["L"] * case["P"] + 4, case["T"], mut)
    return cached(("fused_ref", id(case), tuple(mut)), build)


LF1, LF1P, LF2, LF2P = [(5, 7)], [(4, 8)], [(5, 7), (1, 3)], [(4, 8), (1, 1)]
# (B, Q, M, D, L, P, levels) per dtype: all four (L, P) forms, B = 3 / 8 / 16, D = 8 / 16 / 24, per_img ragged and exact
FUSED_SHAPES = {F32: [(3, 37, 3, 8, 1, 2, LF1), (8, 37, 3, 16, 1, 4, LF1P), (16, 37, 3, 24, 2, 2, LF2P), (3, 32, 4, 16, 2, 4, LF2)],
                F16: [(16, 37, 3, 16, 1, 2, LF1P), (3, 37, 3, 24, 1, 4, LF1), (8, 32, 4, 16, 2, 2, LF2), (8, 37, 3, 8, 2, 4, LF2P)],
                BF16: [(8, 37, 3, 24, 1, 2, LF1P), (16, 32, 4, 16, 1, 4, LF1), (3, 37, 3, 8, 2, 2, LF2P), (16, 37, 3, 16, 2, 4, LF2)]}
FUSED_NONFINITE = [(F32, 3, 37, 3, 16, 2, 4, LF2), (F16, 8, 37, 3, 8, 1, 2, LF1P), (BF16, 3, 37, 3, 16, 2, 2, LF2P)]
MEASURE_SHAPES = [(2, 64, 4, 8, 1, 2, [(4, 8)]), (2, 64, 4, 8, 2, 4, [(4, 8), (2, 2)]), (2, 64, 4, 8, 1, 4, [(2, 4)]), (2, 64, 4, 8, 2, 2, [(1, 2), (8, 8)])]


def fused_form(T, L, P):
    return f"msda_fused_{NAME[T]}_l{L}p{P}"


# ------------------------------------------------------------------------------------------------------------ backward cases
BWD_D = [1, 5, 8, 16, 32, 71]
BWD_LP = [(1, 1, [(2, 3)]), (2, 3, [(5, 7), (1, 3)])]      # a tiny map: the grad_value atomics collide heavily
BWD_B, BWD_Q, BWD_M = 2, 7, 3


def group_size(D):
    gs = 1
    while gs < D and gs < 64:
        gs <<= 1
    return gs


def bwd_case(T, D, L, P, levels, full=False, seed=0):
    """full: random locations with every mantissa bit of T (the kernel's loc W - 0.5 rounds; the bound then carries a location term)."""
    return cached(("bwd", T, D, L, P, tuple(levels), full, seed), lambda: _bwd_case(T, D, L, P, levels, full, seed))


def _bwd_case(T, D, L, P, levels, full, seed):
    B, Q, M = BWD_B, BWD_Q, BWD_M
    shapes, lsi, S = level_table(levels)
    for attempt in range(64):
        g = np.random.default_rng(3571 * seed + 32452843 * attempt + 100 * D + 10 * L + P)
        value = g.standard_normal((B, S, M, D))
        loc = g.uniform(-0.15, 1.15, (B, Q, M, L, P, 2))
        loc = wide(store(loc, T)) if full else np.round(loc * 4096) / 4096          # the 2^-12 grid: f32 location arithmetic is exact
        aw = g.standard_normal((B, Q, M, L, P)) * 0.6
        go = g.standard_normal((B, Q, M * D))
        exempt = np.zeros((B, Q, M, L, P), dtype=bool)
        for l, (H, W) in enumerate(levels):
            for i, (x, y) in enumerate(engineered(H, W, T)):
                b, q, m, p = i % B, (i // (B * M * P)) % Q, (i // (B * P)) % M, (i // B) % P
                loc[b, q, m, l, p] = (x, y)
                exempt[b, q, m, l, p] = True
        try:
            assert_locations_safe(loc, levels, exempt, "backward case", f32_exempt=False)
            break
        except AssertionError:
            continue
    else:
        raise AssertionError("no seed met the distance condition")
    for l, (H, W) in enumerate(levels):
        assert T == F64 or full or bool((f32_exact(loc[:, :, :, l, :, 0], W) & f32_exact(loc[:, :, :, l, :, 1], H)).all()), "a backward location is not exact in f32"
    return dict(T=T, B=B, Q=Q, M=M, D=D, L=L, P=P, S=S, levels=list(levels), shapes=shapes, lsi=lsi, value=store(value, T), loc=store(loc, T), aw=store(aw, T),
                go=store(go, T), exempt=exempt, full=full)


def bwd_reference(case, mut=()):
    return cached(("bwd_ref", id(case), tuple(mut)), lambda: _bwd_reference(case, mut))


def _bwd_reference(case, mut):
    """(grad_value, grad_loc, grad_aw) in float64 and their bounds."""
    T, B, Q, M, D, L, P, S = (case[k] for k in ("T", "B", "Q", "M", "D", "L", "P", "S"))
    value, loc, aw = wide(case["value"]), wide(case["loc"]), wide(case["aw"])
    tg = wide(case["go"]).reshape(B, Q, M, 1, D)
    gv, gv_abs, gv_n, gv_loc = (np.zeros((B, S, M, D)) for _ in range(4))
    gl, gl_abs, gl_loc = (np.zeros((B, Q, M, L, P, 2)) for _ in range(3))
    ga, ga_abs, ga_loc = (np.zeros((B, Q, M, L, P)) for _ in range(3))
    full, u = case["full"], urt(T) / 2
    bI = np.broadcast_to(np.arange(B).reshape(B, 1, 1, 1), (B, Q, M, P))
    mI = np.broadcast_to(np.arange(M).reshape(1, 1, M, 1), (B, Q, M, P))
    for l, pt in enumerate(sample_parts(value, case["levels"], loc)):
        H, W = pt["H"], pt["W"]
        w = corner_weights(pt)
        v1, v2, v3, v4 = pt["v"]
        a = aw[:, :, :, l, :, None]
        ins = pt["inside"]
        lh, lw = pt["lh"][..., None], pt["lw"][..., None]
        hh, hw = 1 - lh, 1 - lw
        # full-mantissa locations: |d h_im| <= u (|loc_y| H + |h_im|) as in the forward bound; a corner weight wy wx moves by at most dh wx + dw wy + dh dw
        dh = np.where(ins, u * (np.abs(pt["y"]) * H + np.abs(pt["h_im"])), 0.0)[..., None] if full else 0.0
        dw = np.where(ins, u * (np.abs(pt["x"]) * W + np.abs(pt["w_im"])), 0.0)[..., None] if full else 0.0
        for wk, (wy, wx), i, ok in zip(w, ((hh, hw), (hh, lw), (lh, hw), (lh, lw)), pt["idx"], pt["ok"]):
            c = np.where(ok[..., None], wk[..., None] * a * tg, 0.0)
            np.add.at(gv, (bI, i, mI), c)
            if full:
                np.add.at(gv_loc, (bI, i, mI), np.where(ok[..., None], np.abs(a * tg) * (dh * wx + dw * wy + dh * dw), 0.0))
            np.add.at(gv_abs, (bI, i, mI), np.abs(c))
            np.add.at(gv_n, (bI, i, mI), np.broadcast_to(ok[..., None], c.shape).astype(np.float64))
        val = sum(wk[..., None] * vk for wk, vk in zip(w, pt["v"]))
        aval = sum(wk[..., None] * np.abs(vk) for wk, vk in zip(w, pt["v"]))
        g_w, g_wa = hh * (v2 - v1) + lh * (v4 - v3), hh * (np.abs(v1) + np.abs(v2)) + lh * (np.abs(v3) + np.abs(v4))
        g_h, g_ha = hw * (v3 - v1) + lw * (v4 - v2), hw * (np.abs(v1) + np.abs(v3)) + lw * (np.abs(v2) + np.abs(v4))
        sx, sy = (H, W) if "swap_WH" in mut else (W, H)
        z = np.zeros(ins.shape)
        ga[:, :, :, l] = np.where(ins, (tg * val).sum(-1), z)
        ga_abs[:, :, :, l] = np.where(ins, (np.abs(tg) * aval).sum(-1), z)
        gx, gy = np.where(ins, sx * (a * tg * g_w).sum(-1), z), np.where(ins, sy * (a * tg * g_h).sum(-1), z)
        gxa, gya = np.where(ins, sx * (np.abs(a * tg) * g_wa).sum(-1), z), np.where(ins, sy * (np.abs(a * tg) * g_ha).sum(-1), z)
        if full:
            f_hw = np.abs(v1 - v2 - v3 + v4)
            ga_loc[:, :, :, l] = np.where(ins, (np.abs(tg) * (dh * np.abs(g_h) + dw * np.abs(g_w) + dh * dw * f_hw)).sum(-1), z)
            gl_loc[:, :, :, l, :, 0] = np.where(ins, sx * (np.abs(a * tg) * dh * f_hw).sum(-1), z)          # d f_w / d h = f_hw
            gl_loc[:, :, :, l, :, 1] = np.where(ins, sy * (np.abs(a * tg) * dw * f_hw).sum(-1), z)
        if "swap_xy" in mut:
            gx, gy, gxa, gya = gy, gx, gya, gxa
        gl[:, :, :, l, :, 0], gl[:, :, :, l, :, 1] = gx, gy
        gl_abs[:, :, :, l, :, 0], gl_abs[:, :, :, l, :, 1] = gxa, gya
    gs = group_size(D)
    r = 1 if full else 0             # hh = fl(1 - lh), hw = fl(1 - lw) round too once lh / lw have every bit: two more roundings u = one more U23
    n = -(-D // gs) + int(math.log2(gs)) + 7 + r
    U = urt(T)
    return dict(gv=gv, gv_b=bound_of(gv, (gv_n + 1 + r) * U * gv_abs + 1.05 * gv_loc, T), gl=gl, gl_b=bound_of(gl, n * U * gl_abs + 1.05 * gl_loc, T),
                ga=ga, ga_b=bound_of(ga, n * U * ga_abs + 1.05 * ga_loc, T))


def bwd_params():
    out = [pytest.param(T, D, L, P, lv, False, id=f"{NAME[T]}-D{D}-L{L}P{P}") for T in (F32, F64) for D in BWD_D for L, P, lv in BWD_LP]
    # the kernel's f32 loc W - 0.5 / lh / hh on locations that round: full-mantissa f32 locations, the bound with its location term
    return out + [pytest.param(F32, D, 2, 3, BWD_LP[1][2], True, id=f"f32-D{D}-L2P3-full-mantissa") for D in (5, 16)]


def all_forward_cases():
    """(label, case, reference) of every forward / fused case of this module - what tests/test_msda_bound_host.py walks."""
    for p in fwd_params():
        T, B, Q, M, D, P, lv, form = p.values
        yield f"{form} {p.id}", "fwd", fwd_case(T, B, Q, M, D, P, lv), form
    for T, B, Q, M, D, P, lv, form in NONFINITE:
        yield f"{form} non-finite", "fwd", fwd_case(T, B, Q, M, D, P, lv, nonfinite=True), form
    for T, shapes in FUSED_SHAPES.items():
        for B, Q, M, D, L, P, lv in shapes:
            yield f"{fused_form(T, L, P)} B{B}", "fused", fused_case(T, B, Q, M, D, L, P, lv), fused_form(T, L, P)
    for T, B, Q, M, D, L, P, lv in FUSED_NONFINITE:
        yield f"{fused_form(T, L, P)} non-finite", "fused", fused_case(T, B, Q, M, D, L, P, lv, nonfinite=True), fused_form(T, L, P)


# ------------------------------------------------------------------------------------------------------------ GPU plumbing
def _dev():
    return torch.device("cuda:0")


def _st():
    return _native.stream_ptr(_dev())


def served_by(form):
    from tests.helpers import msda_served_by
    return msda_served_by(form)


class Guard:
    """rows x width elements of T between `pre` / `post` guard rows, everything filled with the sentinel; `off` shifts the body by that many elements."""

    def __init__(self, rows, width, T, pre=3, post=3, off=0):
        self.rows, self.width, self.pre, self.off = rows, width, pre, off
        self.buf = torch.full(((pre + rows + post) * width,), SENT, dtype=T, device=_dev())
        self.snap = self.buf.clone()
        self.lo = pre * width + off

    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.buf.element_size()

    def body(self):
        return self.buf[self.lo:self.lo + self.rows * self.width].cpu()

    def guards_intact(self):
        torch.cuda.synchronize()
        a, b = self.buf.clone(), self.snap.clone()
        a[self.lo:self.lo + self.rows * self.width] = 0
        b[self.lo:self.lo + self.rows * self.width] = 0
        return torch.equal(a.view(torch.uint8), b.view(torch.uint8))

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.buf.view(torch.uint8), self.snap.view(torch.uint8))


def dev_shifted(t, off=0):
    """t on the device, its first element `off` elements behind an allocation's start."""
    buf = torch.zeros(t.numel() + off, dtype=t.dtype, device=_dev())
    buf[off:] = t.reshape(-1).to(_dev())
    return buf[off:]


def check(got, y, bnd, label):
    got = got.double().numpy().reshape(-1)
    ok, worst, nbad = R.compare(torch.from_numpy(got), torch.from_numpy(y.reshape(-1)), torch.from_numpy(bnd.reshape(-1)), f"{PFX}:{label}")
    print(f"{label}: worst err/bound {worst:.3f}")
    assert ok, f"{label}: {nbad} of {got.size} elements outside their bound (NaN counted), worst err/bound {worst:.3f}"


def run_forward(case, form, value_off=0, out_off=0, label=None):
    T, B, Q, M, D, L, P, S = (case[k] for k in ("T", "B", "Q", "M", "D", "L", "P", "S"))
    value = dev_shifted(case["value"], value_off)
    shapes, lsi = torch.from_numpy(case["shapes"]).to(_dev()), torch.from_numpy(case["lsi"]).to(_dev())
    loc, aw = case["loc"].to(_dev()), case["aw"].to(_dev())
    out = Guard(B * Q, M * D, T, off=out_off)
    with served_by(form):
        rc = _native.lib().lwdetr_msda_forward(value.data_ptr(), shapes.data_ptr(), lsi.data_ptr(), loc.data_ptr(), aw.data_ptr(), out.ptr(), B, S, M, D, L, Q, P,
                                               _native.dtype_code(T), _st())
        assert rc == 0, rc
    y, bnd = fwd_reference(case, form)
    assert out.guards_intact(), f"{form}: a guard row was written"
    check(out.body(), y, bnd, label or f"{form} out")


def fused_args(case, out):
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    keep = [case["value"].to(_dev()), g(case["shapes"]), g(case["lsi"]), case["oa"].to(_dev()), g(case["ref"]), g(case["vr"])]
    v, sh, ls, oa, ref, vr = keep
    B, Q, M, D, L, P, S = (case[k] for k in ("B", "Q", "M", "D", "L", "P", "S"))
    return dict(value=v.data_ptr(), shapes=sh.data_ptr(), lsi=ls.data_ptr(), oa=oa.data_ptr(), ld_oa=case["ld_oa"], logit_col=case["logit_col"], ref=ref.data_ptr(),
                vr=vr.data_ptr(), out=out.ptr(), B=B, S=S, M=M, D=D, L=L, Q=Q, P=P, dtype=_native.dtype_code(case["T"]), st=_st()), keep


def run_fused(case, label=None):
    T, B, Q, M, D, L, P = (case[k] for k in ("T", "B", "Q", "M", "D", "L", "P"))
    out = Guard(B * Q, M * D, T)
    a, keep = fused_args(case, out)
    form = fused_form(T, L, P)
    with served_by(form):
        rc = _native.lib().lwdetr_msda_fused_forward(*a.values())
        assert rc == 0, rc
    y, bnd = fused_reference(case)
    assert out.guards_intact(), f"{form}: a guard row was written"
    check(out.body(), y, bnd, label or f"{form} out")
    return out.body().double().numpy().reshape(B, Q, M, D)


def teardown_module(module):
    rows = [(k, v) for k, v in sorted(R.WORST.items()) if k.startswith(PFX + ":")]
    if rows:
        print("\nworst |got - ref| / bound per (launch form, output):")
        for k, v in rows:
            print(f"  {k[len(PFX) + 1:]:<56s} {v:.3f}")


# ------------------------------------------------------------------------------------------------------------ forward operator
@pytest.mark.gpu
@pytest.mark.parametrize("T,B,Q,M,D,P,levels,form", fwd_params())
def test_msda_forward_vs_fp64(T, B, Q, M, D, P, levels, form):
    run_forward(fwd_case(T, B, Q, M, D, P, levels), form)


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,Q,M,D,P,levels,form", NONFINITE, ids=[f[-1] for f in NONFINITE])
def test_msda_forward_nonfinite_location_contributes_nothing(T, B, Q, M, D, P, levels, form):
    """loc_x = +inf, loc_y = -inf, loc = NaN on one sample of one (b, q, m) each: the float64 reference with that sample skipped (what the generic
    kernel and the reference's kernel do), within the bound - the vector kernel formed NaN * 0 there before make_corners moved an outside sample's
    coordinates to 0."""
    run_forward(fwd_case(T, B, Q, M, D, P, levels, nonfinite=True), form, label=f"{form} out (non-finite locations)")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [F32, F16, BF16], ids=lambda t: NAME[t])
@pytest.mark.parametrize("which", ["value", "out"])
def test_msda_forward_misaligned_pointer_goes_to_generic(T, which):
    """A value / out view 4 elements off an allocation is not aligned for the 8-element vector accesses: the generic kernel serves it, correctly."""
    case = fwd_case(T, 3, 37, 3, 16, 2, LV2)
    off = dict(value_off=4) if which == "value" else dict(out_off=4)
    run_forward(case, f"msda_generic_{NAME[T]}", label=f"msda_generic_{NAME[T]} out ({which} + 4 elements)", **off)


# ------------------------------------------------------------------------------------------------------------ fused
def _fused_params():
    return [pytest.param(T, *s, id=f"{NAME[T]}-l{s[4]}p{s[5]}-B{s[0]}-D{s[3]}") for T, shapes in FUSED_SHAPES.items() for s in shapes]


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,Q,M,D,L,P,levels", _fused_params())
def test_msda_fused_vs_fp64(T, B, Q, M, D, L, P, levels):
    run_fused(fused_case(T, B, Q, M, D, L, P, levels))


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,Q,M,D,L,P,levels", FUSED_NONFINITE, ids=[NAME[f[0]] for f in FUSED_NONFINITE])
def test_msda_fused_nonfinite_location_contributes_nothing(T, B, Q, M, D, L, P, levels):
    run_fused(fused_case(T, B, Q, M, D, L, P, levels, nonfinite=True), label=f"{fused_form(T, L, P)} out (non-finite locations)")


@pytest.mark.gpu
@pytest.mark.parametrize("B,Q,M,D,L,P,levels", MEASURE_SHAPES, ids=[f"l{s[4]}p{s[5]}" for s in MEASURE_SHAPES])
def test_msda_fused_softmax_weights_measured(B, Q, M, D, L, P, levels):
    """Output channel l P + p is the softmax weight of sample (l, p) (module docstring): its relative deviation from the float64 softmax of the stored
    logits, in units of 2^-23, is what TRANS_MEASURED rests on; it is printed and entered in the table."""
    case = fused_case(F32, B, Q, M, D, L, P, levels, measure=True)
    got = run_fused(case, label=f"{fused_form(F32, L, P)} out (weights)")
    _, _, a, _ = fused_locations(case)
    a = a.reshape(B, Q, M, L * P)
    dev = float((np.abs(got[..., :L * P] - a) / a).max()) / U23
    key = f"{PFX}:{fused_form(F32, L, P)} softmax weight, relative deviation / 2^-23 (measured, no bound)"
    R.WORST[key] = max(R.WORST.get(key, 0.0), dev)
    print(f"{fused_form(F32, L, P)}: softmax weight relative deviation {dev:.3f} x 2^-23")
    assert bool((got[..., L * P:] == 0).all())
    assert dev * U23 <= TRANS_MEASURED * 4, "the measured deviation exceeds TRANS_F32: TRANS_MEASURED of this module is out of date"


# ------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.gpu
@pytest.mark.parametrize("T,D,L,P,levels,full", bwd_params())
def test_msda_backward_vs_fp64(T, D, L, P, levels, full):
    case = bwd_case(T, D, L, P, levels, full)
    B, Q, M, S = case["B"], case["Q"], case["M"], case["S"]
    assert_locations_safe(wide(case["loc"]), levels, case["exempt"], "backward case", f32_exempt=False)        # the condition on the inputs, before the launch
    d = lambda k: case[k].to(_dev())
    value, loc, aw, go = d("value"), d("loc"), d("aw"), d("go")
    shapes, lsi = torch.from_numpy(case["shapes"]).to(_dev()), torch.from_numpy(case["lsi"]).to(_dev())
    gv = Guard(B * S, M * D, T)                 # (fully written: zeroed, then accumulated)
    gl, ga = Guard(B * Q * M, L * P * 2, T), Guard(B * Q * M, L * P, T)
    form = f"msda_backward_{NAME[T]}"
    with served_by(form):
        rc = _native.lib().lwdetr_msda_backward(value.data_ptr(), shapes.data_ptr(), lsi.data_ptr(), loc.data_ptr(), aw.data_ptr(), go.data_ptr(), gv.ptr(), gl.ptr(),
                                                ga.ptr(), B, S, M, D, L, Q, P, _native.dtype_code(T), _st())
        assert rc == 0, rc
    ref = bwd_reference(case)
    assert gv.guards_intact() and gl.guards_intact() and ga.guards_intact(), f"{form}: a guard row was written"
    tag = " (full-mantissa locations)" if full else ""
    check(gv.body(), ref["gv"], ref["gv_b"], f"{form} grad_value{tag}")
    check(gl.body(), ref["gl"], ref["gl_b"], f"{form} grad_loc{tag}")
    check(ga.body(), ref["ga"], ref["ga_b"], f"{form} grad_aw{tag}")


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_msda_fused_refusals():
    T, B, Q, M, D, L, P = F16, 3, 37, 3, 16, 2, 4
    case = fused_case(T, B, Q, M, D, L, P, LF2)
    out = Guard(B * Q, M * D, T)
    a, keep = fused_args(case, out)
    mlp = M * L * P

    def refused(expect, label, **over):
        before = _native.msda_path_counts()
        rc = _native.lib().lwdetr_msda_fused_forward(*{**a, **over}.values())
        assert rc == expect, f"{label}: rc {rc}, expected {expect}"
        assert _native.msda_path_counts() == before and out.untouched(), f"{label}: something was written or counted"

    refused(UNSUPPORTED, "dtype 3", dtype=3)
    for l, p in ((1, 1), (3, 2), (2, 8)):          # (columns of oa sized for the largest of them: the refusal is about the form)
        big = M * l * p
        refused(UNSUPPORTED, f"(L, P) = ({l}, {p})", L=l, P=p, logit_col=2 * big, ld_oa=3 * big)
    refused(BAD_ARG, "D % 8", D=12)
    for n in ("value", "shapes", "lsi", "oa", "ref", "vr", "out"):
        refused(BAD_ARG, f"{n} null", **{n: None})
    refused(BAD_ARG, "logit_col < 2 M L P", logit_col=2 * mlp - 1)
    refused(BAD_ARG, "logit_col < 0", logit_col=-8)
    refused(BAD_ARG, "ld_oa < logit_col + M L P", ld_oa=case["logit_col"] + mlp - 1)
    refused(BAD_ARG, "ld_oa < 0", ld_oa=-case["ld_oa"])
    refused(BAD_ARG, "value misaligned", value=a["value"] + 8)
    refused(BAD_ARG, "out misaligned", out=a["out"] + 8)


@pytest.mark.gpu
def test_msda_forward_and_backward_refusals():
    case = bwd_case(F32, 16, 2, 3, BWD_LP[1][2])
    B, Q, M, D, L, P, S = (case[k] for k in ("B", "Q", "M", "D", "L", "P", "S"))
    d = lambda k, T: case[k].to(T).to(_dev())
    shapes, lsi = torch.from_numpy(case["shapes"]).to(_dev()), torch.from_numpy(case["lsi"]).to(_dev())
    for T, expect in ((F16, UNSUPPORTED), (BF16, UNSUPPORTED)):          # the reference differentiates float / double only
        value, loc, aw, go = d("value", T), d("loc", T), d("aw", T), d("go", T)
        gv, gl, ga = Guard(B * S, M * D, T), Guard(B * Q * M, L * P * 2, T), Guard(B * Q * M, L * P, T)
        before = _native.msda_path_counts()
        rc = _native.lib().lwdetr_msda_backward(value.data_ptr(), shapes.data_ptr(), lsi.data_ptr(), loc.data_ptr(), aw.data_ptr(), go.data_ptr(), gv.ptr(), gl.ptr(),
                                                ga.ptr(), B, S, M, D, L, Q, P, _native.dtype_code(T), _st())
        assert rc == expect and _native.msda_path_counts() == before and gv.untouched() and gl.untouched() and ga.untouched(), f"backward {NAME[T]}: rc {rc}"
    value, loc, aw, go = d("value", F32), d("loc", F32), d("aw", F32), d("go", F32)
    gv, gl, ga = Guard(B * S, M * D, F32), Guard(B * Q * M, L * P * 2, F32), Guard(B * Q * M, L * P, F32)
    out = Guard(B * Q, M * D, F32)
    ptrs = dict(value=value.data_ptr(), shapes=shapes.data_ptr(), lsi=lsi.data_ptr(), loc=loc.data_ptr(), aw=aw.data_ptr())
    for n in ("value", "shapes", "lsi", "loc", "aw", "go", "gv", "gl", "ga"):
        p = dict(ptrs, go=go.data_ptr(), gv=gv.ptr(), gl=gl.ptr(), ga=ga.ptr())
        p[n] = None
        before = _native.msda_path_counts()
        rc = _native.lib().lwdetr_msda_backward(*p.values(), B, S, M, D, L, Q, P, 0, _st())
        assert rc == BAD_ARG and _native.msda_path_counts() == before and gv.untouched() and gl.untouched() and ga.untouched(), f"backward, {n} null: rc {rc}"
    for n in ("value", "shapes", "lsi", "loc", "aw", "out"):
        p = dict(ptrs, out=out.ptr())
        p[n] = None
        before = _native.msda_path_counts()
        rc = _native.lib().lwdetr_msda_forward(*p.values(), B, S, M, D, L, Q, P, 0, _st())
        assert rc == BAD_ARG and _native.msda_path_counts() == before and out.untouched(), f"forward, {n} null: rc {rc}"
    before = _native.msda_path_counts()
    assert _native.lib().lwdetr_msda_forward(*dict(ptrs, out=out.ptr()).values(), B, S, M, D, L, Q, P, 4, _st()) == UNSUPPORTED
    assert _native.msda_path_counts() == before and out.untouched()


# ------------------------------------------------------------------------------------------------------------ the record, at the end
@pytest.mark.gpu
def test_msda_every_instantiation_was_launched():
    """After this module every instantiation the record names has a non-zero count (this test runs last in the module)."""
    counts = _native.msda_path_counts()
    assert len(counts) == 9 + 4 + 12 + 2, sorted(counts)
    assert all(v > 0 for v in counts.values()), {k: v for k, v in counts.items() if v == 0}
