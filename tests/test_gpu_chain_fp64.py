"""The kernels of csrc/chain.hip (lwdetr_enc_chain, lwdetr_row_chain), called straight through the C entries at the smallest shapes at which their
row mapping, ring accounting, buffer-bounded stores and launch forms can go wrong, every launch pinned to ONE of the 24 instantiations by the
launch-form record (lwdetr_chain_path_counts, helpers.chain_served_by) and every output checked ELEMENT BY ELEMENT against float64 arithmetic on
the operands as stored. Output buffers carry guard rows / pad columns / rows of other levels filled with a sentinel that must come back
bit-identical; every launch is repeated and must give identical bits. The machinery (rounding, tie carrying, propagation, comparison) is that of
tests/test_gpu_vitblock.py; what differs is listed here.

Operands as stored. The dense float64 weights are the packed 16-bit stream UN-packed (unpack_pieces / unpack_pieces_split: the inverse of
kernels.chain_pieces / chain_pieces_split; tests/test_chain_bound_host.py walks the same stream fragment by fragment instead), the vectors are the
f32 `vec` as packed.

Rounding points (T = the storage type), read from chain.hip / chain_enc_body.h:
  * every stage output is rounded to T before it is used again (`cpack2<T>` of the accumulators): FULL stages, the SiLU output, both LayerNorms;
  * accumulators start at the bias (`bias16`); the residual is added to the bias in f32 BEFORE the MFMAs (`init[..] += v`), so the pre-rounding value is
    b + res + W x in one f32 accumulation; ReLU comes before the rounding (`fmaxf` then `cpack2`);
  * LayerNorm is two-pass f32 on the ROUNDED row: mean = sum / D, var = sum (v - mean)^2 / D, `fmaf((v - mean) * rstd, g, b)` rounded to T - nothing
    is rounded between the normalisation and the affine;
  * `T(y + qpos)` (ADDQ) is the NEXT operand, while the stored row is y; a SIDE stage reads the current operand and leaves it;
  * enc chain: SiLU is `a / (1 + __expf(-a))` on the f32 accumulator, rounded to T, then LayerNorm2d -> `memory` (rounded: the operand of everything
    after); the padding mask ZEROES THE VALUE ACCUMULATORS of rows with notpad[mm] == 0 (exact zeros are stored); rowvalid[mm] == 0 zeroes the INPUT
    operand of enc_output, so that row becomes LN(T(b_enc)); class logits are T(W_c om + b_c) over all `cols` columns (zero weights and bias
    beyond ncls: exact zeros), cls_max is the maximum of the ROUNDED logits over columns < ncls;
  * flags are indexed by the memory row mm = (m / npix) S + lsi + m % npix, not by the input row m.

Bound per element: half_ulp_T(|y| + E) + E, E built stage by stage (test_gpu_vitblock.py's docstring): one 32x32x16 MFMA step is 16 exact products
plus the accumulator, K / 16 steps: |acc^ - acc| <= U23 ((K / 16 + 2) |start| + (K / 16 + 18) S), S = sum_k |x_k w_k| of THAT element (V.acc_err);
TWO_CHAINS (enc D = 256 without cv2, and the split kernel always) adds the two partial accumulators once more: + U23 (|start| + S). LayerNorm: the
derivation of V.ln_stage (n_add = D / 2 + 2 serial additions per lane; the split form adds D / 8 per lane and four partial sums: fewer) + TRANS_F32 |z|
for `1 / sqrtf`, times |gamma|, + U23 |y| for the fmaf. SiLU: 1.1 e_a for the argument (|silu'| <= 1.0999) + |s| (2 TRANS_F32 + 3 U23 (1 + |a|)) for
__expf (the argument scaled by log2 e, v_exp_f32), 1 + e and the division. ADDQ: + U23 |y + q|. Tie deviations are carried in both modes (worst case:
every element inside; tight, Z = 4: SHARE = 1e-3 of a tensor may lie outside). No term is scaled by a tensor-wide maximum.

Hardware transcendentals: TRANS_F32 = 4 TRANS_MEASURED. How they are made visible (outputs are 16-bit, so a deviation of an f32 ulp is not visible in an
ordinary row):
  * `1 / sqrtf`: test_chain_rstd_measured runs a ONE-stage row chain whose weight is the identity (the stored pre-LayerNorm row IS the input row, bit for
    bit), gamma = 2^14 and beta_c = -fl32(2^14 z_c) of the float64 z of that row, so that fmaf((v - mean) rstd, g, b) CANCELS to 2^14 (z^ - z) before its
    only rounding: the stored number is the deviation of the kernel's f32 z from the float64 z, resolved to 2^-10 of itself. Reported per launch as
    max |z^ - z| / |z| over |z| >= 0.5 (raw) and what of it lies beyond the derived arithmetic of the two-pass statistics.
  * SiLU (`__expf`, the division): test_chain_silu_measured runs the cv2 form of the enc chain with LayerNorm2d gamma = 8, so that neighbouring T numbers
    of the SiLU output stay apart in `memory`, over rows whose arguments cover [-8, 8], and reports the largest |memory^ - memory| beyond the worst-case
    bound evaluated with TRANS_F32 = 0, relative to the element.
MEASURED (MI355X, 256 CUs, committed seeds; profiles/chain_fp64_worst_ratios.txt). 1 / sqrtf: over 8 rows per form (split f16 / bf16 at D = 256 and 384, row-per-wave
f16 / bf16) the kernel's z deviates from the float64 z of its own stored row by at most 2.158 x 2^-23 relative (row_f16_d256_res0_q0; 1.281 ... 1.689 in the
split forms) and by 0.000 x 2^-23 beyond the derived arithmetic of the two-pass statistics in every launch. SiLU: arguments in [-10.4, 10.3], 38400 elements of
`memory` per dtype, none outside the worst-case bound evaluated without a transcendental term (0.000 x 2^-23). Both measure zero beyond the arithmetic, so
TRANS_MEASURED is one f32 ulp, 2^-23 (the documented accuracy of v_rsq_f32 / v_exp_f32 / v_rcp_f32), and TRANS_F32 = 4 f32 ulps, the margin this project uses
everywhere. Everything else in the bound is derived, not measured.

cls_max, the zero columns [ncls, cols), value rows with notpad == 0, the sentinel in columns >= cols / >= ceil4(n), guard rows and the rows of other
levels, and the bits of a repeated launch are exact checks.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from lwdetr_amd import _native
from lwdetr_amd import kernels as K
from tests import test_gpu_rowops as R
from tests import test_gpu_vitblock as V
from tests.helpers import chain_served_by
from tests.test_gpu_rowops import half_ulp, U23, SENT, PADV, F16, BF16
from tests.test_gpu_vitblock import round_stage, prop, n_eff, ln_stage, bound_of, check2, fails_exactly, Buf, Z, SHARE  # noqa: F401 (ln_stage: see ln_affine)

TRANS_MEASURED = 2.0 ** -23   # one f32 ulp: both visible transcendentals measured 0 beyond the derived arithmetic (module docstring)
TRANS_F32 = 4 * TRANS_MEASURED
BAD_ARG, UNSUPPORTED = _native.ERR_BAD_ARG, _native.ERR_UNSUPPORTED
NAME = {F16: "f16", BF16: "bf16"}
SILU_LIP = 1.1
FORM_WORST, FORM_TIGHT = {}, {}
RAN, ALL_CASES = set(), set()
_CACHE = {}
ALL_FORMS = ([f"enc_{t}_{f}_{w}" for t in ("f16", "bf16") for f in ("d256_pf1", "d256_pf0", "d384_pf0") for w in ("narrow", "wide")]
             + [f"row_{t}_d256_{f}" for t in ("f16", "bf16") for f in ("k512", "res0_q0", "res1_q0", "res1_q1")]
             + [f"split_{t}_d{d}" for t in ("f16", "bf16") for d in (256, 384)])


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


def _dev():
    return torch.device("cuda:0")


def ceil4(n):
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------------------ the stream, un-packed
def unpack_pieces(flat, n, k, kslots=None):
    """The inverse of kernels.chain_pieces: flat stream of n / 32 * k / 64 pieces -> dense (n, k) float64."""
    wk = flat.double().reshape(n // 32, k // 64, 4, 2, 32, 8).permute(0, 4, 1, 2, 3, 5).reshape(n, k)
    if kslots is None:
        return wk
    w = torch.empty_like(wk)
    w[:, kslots] = wk
    return w


def unpack_pieces_split(flat, n, kslots=None):
    """The inverse of kernels.chain_pieces_split (K = 384: k-half-major inside every group of up to 4 tiles)."""
    tiles, pos = [], 0
    for g0 in range(0, n // 32, 4):
        ng = min(4, n // 32 - g0)
        a = flat[pos:pos + ng * 3 * 2048].reshape(ng, 3, 2048)
        b = flat[pos + ng * 3 * 2048:pos + ng * 6 * 2048].reshape(ng, 3, 2048)
        tiles.append(torch.cat([a, b], 1))
        pos += ng * 6 * 2048
    return unpack_pieces(torch.cat(tiles).reshape(-1), n, 384, kslots)


# ------------------------------------------------------------------------------------------------------------ arithmetic models
def acc(x, ex, sx, W, start, K_, mode, two):
    """pre = start + x W^T in one f32 accumulation over K / 16 MFMA steps: (pre, e, sg)."""
    pre = x @ W.t() + start
    S = x.abs() @ W.abs().t()
    sa = start.abs().expand_as(pre)
    e = V.acc_err(K_, sa, S, mode) + (U23 * (sa + S) if two else 0.0)
    pe, ps = prop(ex, sx, W, mode)
    return pre, e + pe, ps


def ln_affine(x, e, sg, gam, bet, eps, T, mode, trans):
    """fmaf((x - mean) rstd, g, b) of the rounded rows x that the kernel holds up to (e, sg), BEFORE its rounding to T: V.ln_stage's derivation (same
    e_ln, same first-order propagation) without the rounding of z, + trans |z| for 1 / sqrtf, times |g|, + the rounding of the fmaf."""
    C_ = x.shape[1]
    mean = x.mean(1, keepdim=True)
    dd = x - mean
    rstd = 1.0 / torch.sqrt((dd * dd).mean(1, keepdim=True) + float(np.float32(eps)))
    z = dd * rstd
    m = x.abs().mean(1, keepdim=True)
    n = C_ // 2 + 2
    e_ln = 0.5 * U23 * ((n_eff(n // 2 + 8, mode) + 2) * z.abs() + (n_eff(n + 1, mode) + 3) * m * rstd) + trans * z.abs()
    pe = 1.05 * rstd * (e + e.mean(1, keepdim=True) + z.abs() * (z.abs() * e).mean(1, keepdim=True))
    ps = 1.05 * rstd * torch.sqrt(sg * sg + (sg * sg).sum(1, keepdim=True) / C_ ** 2 + z * z * (z * z * sg * sg).sum(1, keepdim=True) / C_ ** 2)
    y = z * gam + bet
    return y, gam.abs() * (e_ln + pe) + U23 * y.abs(), gam.abs() * ps, z, e_ln


def _rec(pre, e, s):
    return pre, e + Z * s


def row_dense(stream, vec, D, k_in, stages):
    """Per stage the dense float64 operands the kernel sees: W (N, K) from the packed stream, bias / gamma / beta from vec."""
    perm = K.vb_kslot_channels(D)
    unp = (lambda f, n, k, ks: unpack_pieces_split(f, n, ks)) if D == 384 else unpack_pieces
    out, pos, off, natural = [], 0, 0, True
    vec = vec.double()
    for i, st in enumerate(stages):
        if st["kind"] == "full":
            k = k_in if i == 0 else D
            cnt = D // 32 * (k // 64) * 2048
            d = dict(W=unp(stream[pos:pos + cnt], D, k, None if natural else perm), b=vec[off:off + D])
            off += D
            if st.get("ln") is not None:
                d["g"], d["be"] = vec[off:off + D], vec[off + D:off + 2 * D]
                off += 2 * D
            natural = False
        else:
            nt = (st["n"] + 31) // 32
            cnt = nt * (D // 64) * 2048
            d = dict(W=unp(stream[pos:pos + cnt], 32 * nt, D, None if natural else perm), b=vec[off:off + 32 * nt])
            off += 32 * nt
        pos += cnt
        out.append(d)
    assert pos + 2 * 2048 == stream.numel() and not bool(stream[pos:].any()), "the stream ends with the two zero pieces of the read-ahead"
    return out


def row_reference(x, res, qpos, dense, D, k_in, stages, T, mode, two, trans=None):
    """{stage index: (value before the last rounding, E)} of every stage that stores; SIDE stages over all 32 nt columns."""
    trans = TRANS_F32 if trans is None else trans
    cur = x.double()
    ec, sc = torch.zeros_like(cur), torch.zeros_like(cur)
    out = {}
    for i, (st, d) in enumerate(zip(stages, dense)):
        if st["kind"] == "side":
            out[i] = _rec(*acc(cur, ec, sc, d["W"], d["b"], D, mode, two))
            continue
        start = d["b"] + res.double() if st.get("res") else d["b"]
        pre, e, s = acc(cur, ec, sc, d["W"], start, k_in if i == 0 else D, mode, two)
        if st.get("relu"):
            pre = pre.clamp_min(0.0)
        rec = _rec(pre, e, s)
        y, ey, sy, _ = round_stage(pre, e, s, T, mode)
        if st.get("ln") is not None:
            p2, e2, s2, _, _ = ln_affine(y, ey, sy, d["g"], d["be"], st["ln"], T, mode, trans)
            rec = _rec(p2, e2, s2)
            y, ey, sy, _ = round_stage(p2, e2, s2, T, mode)
        if st.get("store"):
            out[i] = rec
        if st.get("addq"):
            p3 = y + qpos.double()
            y, ey, sy, _ = round_stage(p3, ey + U23 * p3.abs(), sy, T, mode)
        cur, ec, sc = y, ey, sy
    return out


def enc_dense(stream, vec, D, k5, nl, cols):
    perm = K.vb_kslot_channels(D)
    ms = perm if k5 else None
    vec = vec.double()
    d, pos, off = {}, 0, 0
    if k5:
        cnt = D // 32 * (k5 // 64) * 2048
        d["w2"] = unpack_pieces(stream[pos:pos + cnt], D, k5)
        pos += cnt
        d["b2"], d["gp"], d["bp"] = vec[0:D], vec[D:2 * D], vec[2 * D:3 * D]
        off = 3 * D
    cnt = nl * D // 32 * (D // 64) * 2048
    d["wv"] = unpack_pieces(stream[pos:pos + cnt], nl * D, D, ms)
    pos += cnt
    cnt = D // 32 * (D // 64) * 2048
    d["we"] = unpack_pieces(stream[pos:pos + cnt], D, D, ms)
    pos += cnt
    cnt = cols // 32 * (D // 64) * 2048
    d["wc"] = unpack_pieces(stream[pos:pos + cnt], cols, D, perm)
    pos += cnt
    assert pos + 2 * 2048 == stream.numel() and not bool(stream[pos:].any())
    d["be"], d["ge"], d["bt"] = vec[off:off + D], vec[off + D:off + 2 * D], vec[off + 2 * D:off + 3 * D]
    d["bc"] = vec[off + 3 * D:off + 3 * D + cols]
    d["bv"] = vec[off + 3 * D + cols:off + 3 * D + cols + nl * D]
    return d


def silu64(a):
    return a / (1.0 + torch.exp(-a))


def enc_reference(x, rv, npd, d, D, k5, nl, T, mode, eps_p, eps_e, trans=None):
    """rv / npd: the flags of the MEMORY rows of the input rows (float64 0 / 1, (M,)). {name: (value before the last rounding, E)} per input row."""
    trans = TRANS_F32 if trans is None else trans
    two = D == 256 and not k5
    x = x.double()
    zero = torch.zeros_like(x)
    out = {}
    if k5:
        a, ea, sa = acc(x, zero, zero, d["w2"], d["b2"], k5, mode, two)
        s = silu64(a)
        es = SILU_LIP * ea + s.abs() * (2 * trans + 3 * U23 * (1 + a.abs()))
        v, ev, sv, _ = round_stage(s, es, SILU_LIP * sa, T, mode)
        p, e, sg, _, _ = ln_affine(v, ev, sv, d["gp"], d["bp"], eps_p, T, mode, trans)
        out["memory"] = _rec(p, e, sg)
        mem, em, sm, _ = round_stage(p, e, sg, T, mode)
    else:
        mem, em, sm = x, zero, zero
    p, e, sg = acc(mem, em, sm, d["wv"], d["bv"], D, mode, two)
    keep = npd[:, None]
    out["values"] = (p * keep, (e + Z * sg) * keep)
    keep = rv[:, None]
    p, e, sg = acc(mem * keep, em * keep, sm * keep, d["we"], d["be"], D, mode, two)
    y, ey, sy, _ = round_stage(p, e, sg, T, mode)
    p, e, sg, _, _ = ln_affine(y, ey, sy, d["ge"], d["bt"], eps_e, T, mode, trans)
    out["om"] = _rec(p, e, sg)
    om, eo, so, _ = round_stage(p, e, sg, T, mode)
    out["cls"] = _rec(*acc(om, eo, so, d["wc"], d["bc"], D, mode, two))
    return out


# ------------------------------------------------------------------------------------------------------------ comparison
def check(form, got, ref_t, ref_w, T, label):
    """check2 (every element inside the worst-case bound, at most SHARE outside the tight one) + the per-form table of worst ratios."""
    y, et = ref_t
    ew = ref_w[1]
    got, y, et, ew = got.double().flatten(), y.flatten(), et.flatten(), ew.flatten()
    if got.numel() == 0:
        return None
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


def teardown_module(module):
    if FORM_WORST:
        print("\nworst |diff| / bound per launch form (worst-case bound; tight bound among the elements inside it, elements outside / all):")
        for f in sorted(f for f in FORM_WORST if f in ALL_FORMS):
            t = FORM_TIGHT[f]
            print(f"CHAIN_WORST_FORM {f:<28s} {FORM_WORST[f]:.3f}   {t[0]:.3f} {t[1]} / {t[2]}")


# ------------------------------------------------------------------------------------------------------------ row-chain cases
def program(name, D):
    """Stage programs by name: dicts of kind / n / relu / res / ln (eps) / store / addq / ldo; (stages, k_in, uses res pointer, uses qpos pointer, strides)."""
    F = lambda **kw: dict(kind="full", **kw)
    S = lambda n, ldo=None: dict(kind="side", n=n, ldo=ldo if ldo is not None else ceil4(n))
    noa = 96 if D == 256 else 576                    # sampling_offsets | attention_weights: 3 tiles / 18 tiles (groups of 4, 4, 4, 4, 2 at D = 384)
    ld = {}
    k_in, res, q = D, False, False
    if name == "front":
        st, res, q = [F(res=True, ln=1e-5, store=True, addq=True), S(noa)], True, True
    elif name == "front_strided":                    # every stride larger than its row
        st, res, q = [F(res=True, ln=1e-5, store=True, addq=True, ldo=D + 24), S(noa, noa + 16)], True, True
        ld = dict(ld_in=D + 8, ld_res=D + 16, ld_q=D + 40)
    elif name == "back":
        st, res = [F(res=True, ln=1e-5, store=True)], True
    elif name == "heads":
        st = [S(91), F(relu=True), F(relu=True), S(4)]
    elif name == "bbox":
        st = [F(relu=True), F(relu=True), S(4)]
    elif name == "refpoint":
        st, k_in = [F(relu=True), F(store=True)], 2 * D
    elif name.startswith("side1_"):                  # one SIDE stage: a chain shorter than the ring (nt * D / 64 + 2 pieces)
        n = int(name.split("_")[1])
        st = [S(n, ceil4(n) + (8 if n == 33 else 0))]
    elif name == "sides":                            # partial groups: nt = 1, 2, 3, 5; 16-byte stores (n % 8 == 0 and ldo % 8 == 0) and 8-byte ones
        st = [F(relu=True), S(24, 24), S(40, 48), S(91, 92), S(130, 140)]
    elif name == "sides8":                           # n % 8 == 0 but ldo % 8 != 0: the 8-byte path with nothing to pad
        st = [S(32, 36), S(64, 64)]
    elif name == "fsf":                              # the operand survives the SIDE stage
        st = [F(ln=1e-5, store=True), S(33, 40), F(relu=True, store=True)]
    elif name == "res_unused":                       # a `res` pointer that no stage uses (split: has_r, never use_r; row form: res1_q0)
        st, res = [F(relu=True, store=True)], True
    elif name == "q_unused":                         # both pointers, ADDQ never used (row form: res1_q1)
        st, res, q = [F(res=True, store=True), S(4)], True, True
    elif name == "flags":                            # LN without STORE, STORE without LN, ADDQ without STORE, RELU + RES
        st, res, q = [F(ln=1e-6), F(store=True), F(addq=True), F(relu=True, res=True, store=True)], True, True
    elif name == "six":
        st, res = [F(ln=1e-5, store=True), F(relu=True), S(4), F(res=True, store=True), S(91, 96), F(ln=1e-6, store=True)], True
    else:
        raise KeyError(name)
    return st, k_in, res, q, ld


def row_case(name, D, T, M, seed=0):
    """Seeds: `seed` is chosen (0 everywhere so far) so that the f32 emulation of tests/test_chain_bound_host.py stays within SHARE of the tight bound."""
    def build():
        stages, k_in, has_res, has_q, ld = program(name, D)
        g = torch.Generator().manual_seed(7000 + seed + 13 * D + sum(map(ord, name)))
        r = lambda *s: torch.randn(*s, generator=g)
        full = []
        for i, st in enumerate(stages):
            st = dict(st)
            if st["kind"] == "full":
                k = k_in if i == 0 else D
                st["w"], st["b"] = r(D, k) / k ** 0.5, r(D) * 0.3
                if st.get("ln") is not None:
                    st["ln"] = (1 + 0.2 * r(D), 0.2 * r(D), st["ln"])
            else:
                st["w"], st["b"] = r(st["n"], D) / D ** 0.5, r(st["n"]) * 0.3
            full.append(st)
        stream, vec = K.RowChainOp.pack(D, T, k_in, full)
        gx = torch.Generator().manual_seed(7100 + seed + M + D)
        x = (torch.randn(M, k_in, generator=gx) * 1.2 + 0.1).to(T)
        res = torch.randn(M, D, generator=gx).to(T) if has_res else None
        qpos = torch.randn(M, D, generator=gx).to(T) if has_q else None
        plain = [dict(st, ln=st["ln"][2]) if st["kind"] == "full" and st.get("ln") is not None else st for st in full]
        plain = [{k: v for k, v in st.items() if k not in ("w", "b")} for st in plain]
        case = dict(name=name, D=D, T=T, M=M, k_in=k_in, stages=plain, stream=stream, vec=vec, x=x, res=res, qpos=qpos, ld=ld)
        dense = row_dense(stream, vec, D, k_in, plain)
        for two in (False, True):                    # the row-per-wave form has one accumulator chain, the split form two
            case["tight", two] = row_reference(x, res, qpos, dense, D, k_in, plain, T, "tight", two)
            case["worst", two] = row_reference(x, res, qpos, dense, D, k_in, plain, T, "worst", two)
        return case
    return cached(("row", name, D, T, M, seed), build)


def row_form(T, D, k_in, M, has_res, has_q, split_rows=16384):
    if D == 384 or (k_in == D and M <= split_rows):
        return f"split_{NAME[T]}_d{D}"
    return f"row_{NAME[T]}_d256_" + ("k512" if k_in != D else f"res{int(has_res)}_q{int(has_q)}")


class RowRun:
    """One lwdetr_row_chain call on guarded buffers, straight through the C entry."""

    def __init__(self, case, over=None):
        c, D, T, M = case, case["D"], case["T"], case["M"]
        over = over or {}
        ld = c["ld"]
        self.case = c
        self.x = Buf(M, ld.get("ld_in", c["k_in"]), T, pre=4, post=4, fill=PADV)
        self.x.load(c["x"])
        self.res = self.q = None
        res, qpos = over.get("res", c["res"]), over.get("qpos", c["qpos"])
        if res is not None:
            self.res = Buf(M, ld.get("ld_res", D), T, pre=4, post=4, fill=PADV)
            self.res.load(res)
        if qpos is not None:
            self.q = Buf(M, ld.get("ld_q", D), T, pre=4, post=4, fill=PADV)
            self.q.load(qpos)
        self.stream, self.vec = over.get("stream", c["stream"]).to(_dev()), over.get("vec", c["vec"]).to(_dev())
        d = _native.ChainDesc()
        d.inp, d.ld_in, d.k_in = self.x.ptr(), self.x.ld, c["k_in"]
        d.res, d.ld_res = (self.res.ptr(), self.res.ld) if self.res else (None, 0)
        d.qpos, d.ld_q = (self.q.ptr(), self.q.ld) if self.q else (None, 0)
        d.wstream, d.vec, d.M, d.D, d.nst = self.stream.data_ptr(), self.vec.data_ptr(), M, D, len(c["stages"])
        self.out = {}
        for i, st in enumerate(c["stages"]):
            s = d.st[i]
            if st["kind"] == "full":
                s.kind, s.n, s.eps = _native.CHAIN_FULL, D, float(st["ln"]) if st.get("ln") is not None else 0.0
                s.flags = ((_native.CHAIN_RES if st.get("res") else 0) | (_native.CHAIN_RELU if st.get("relu") else 0) | (_native.CHAIN_LN if st.get("ln") is not None else 0)
                           | (_native.CHAIN_STORE if st.get("store") else 0) | (_native.CHAIN_ADDQ if st.get("addq") else 0))
                if st.get("store"):
                    self.out[i] = Buf(M, st.get("ldo") or D, T, pre=4, post=4)
            else:
                s.kind, s.n, s.flags, s.eps = _native.CHAIN_SIDE, st["n"], 0, 0.0
                self.out[i] = Buf(M, st["ldo"], T, pre=4, post=4)
            if i in self.out:
                s.out, s.ldo = self.out[i].ptr(), self.out[i].ld
                self.out[i].freeze()
        self.desc = d
        lib = _native.lib()
        assert self.stream.numel() * 2 == lib.lwdetr_row_chain_pieces(C.byref(d)) * 4096 and self.vec.numel() == lib.lwdetr_row_chain_vec_floats(C.byref(d))

    def launch(self):
        return _native.lib().lwdetr_row_chain(C.byref(self.desc), _native.dtype_code(self.case["T"]), _native.stream_ptr())

    def width(self, i):
        st = self.case["stages"][i]
        if st["kind"] == "full":
            return self.case["D"]
        return st["n"] if (st["n"] % 8 == 0 and st["ldo"] % 8 == 0) else ceil4(st["n"])


def run_row(case, form, label, over=None, check_ref=True):
    """Launch (pinned), repeat (identical bits), guards, zero pad columns, element-wise check. Returns {stage: rows as stored (M, n)}."""
    run = RowRun(case, over)
    with chain_served_by(form):
        assert run.launch() == 0, label
    first = {i: b.buf.clone() for i, b in run.out.items()}
    with chain_served_by(form):
        assert run.launch() == 0, label
    two = form.startswith("split")
    got = {}
    for i, b in run.out.items():
        st = case["stages"][i]
        n = case["D"] if st["kind"] == "full" else st["n"]
        w = run.width(i)
        assert torch.equal(b.buf.view(torch.int16), first[i].view(torch.int16)), f"{label}: stage {i}: a repeated launch gives other bits"
        assert b.guards_intact(0, w), f"{label}: stage {i}: written outside rows [0, M) x columns [0, {w})"
        assert bool((b.body(n, w - n) == 0).all()), f"{label}: stage {i}: pad columns [{n}, {w}) are not zero"
        got[i] = b.body(0, n).cpu()
        if check_ref:
            yt, et = case["tight", two][i]
            yw, ew = case["worst", two][i]
            check(form, got[i], (yt[:, :n], et[:, :n]), (yw[:, :n], ew[:, :n]), case["T"], f"{label} stage {i}")
    return got


def _case_id(*parts):
    cid = "-".join(NAME.get(p, str(p)) for p in parts)
    ALL_CASES.add(cid)
    return cid


SPLIT_PROGRAMS = [("front", 33), ("front", 300), ("front_strided", 301), ("back", 1), ("back", 32), ("heads", 31), ("heads", 301), ("bbox", 33), ("side1_1", 1),
                  ("side1_4", 33), ("side1_31", 32), ("side1_32", 31), ("side1_33", 300), ("sides", 33), ("sides8", 31), ("fsf", 32), ("res_unused", 33),
                  ("q_unused", 31), ("flags", 301), ("six", 33)]
ROW_PROGRAMS = [("front", 33, "res1_q1"), ("front_strided", 129, "res1_q1"), ("back", 1, "res1_q0"), ("back", 127, "res1_q0"), ("heads", 300, "res0_q0"),
                ("bbox", 33, "res0_q0"), ("refpoint", 1, "k512"), ("refpoint", 129, "k512"), ("side1_1", 1, "res0_q0"), ("side1_33", 127, "res0_q0"),
                ("sides", 129, "res0_q0"), ("sides8", 33, "res0_q0"), ("fsf", 300, "res0_q0"), ("res_unused", 33, "res1_q0"), ("q_unused", 127, "res1_q1"),
                ("flags", 129, "res1_q1"), ("six", 300, "res1_q0")]


def split_params():
    return [pytest.param(T, D, name, M, id=_case_id("split", T, D, name, M)) for T in (F16, BF16) for D in (256, 384) for name, M in SPLIT_PROGRAMS]


def rowwave_params():
    return [pytest.param(T, name, M, f, id=_case_id("row", T, name, M)) for T in (F16, BF16) for name, M, f in ROW_PROGRAMS]


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,name,M", split_params())
def test_row_chain_split_vs_fp64(T, D, name, M, request):
    case = row_case(name, D, T, M)
    run_row(case, f"split_{NAME[T]}_d{D}", request.node.callspec.id)
    RAN.add(request.node.callspec.id)


@pytest.mark.gpu
@pytest.mark.parametrize("T,name,M,f", rowwave_params())
def test_row_chain_row_per_wave_vs_fp64(T, name, M, f, request):
    """The row-per-wave form at small M: CHAIN_SPLIT_ROWS = 0 sends every row count to it (k_in = 2 D goes there whatever the knob says)."""
    case = row_case(name, 256, T, M)
    _native.tuning_set("CHAIN_SPLIT_ROWS", 0)
    try:
        run_row(case, f"row_{NAME[T]}_d256_{f}", request.node.callspec.id)
    finally:
        _native.tuning_set("CHAIN_SPLIT_ROWS", None)
    RAN.add(request.node.callspec.id)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [F16, BF16], ids=lambda v: NAME[v])
def test_row_chain_routing_without_the_knob(T):
    """16 384 rows: the split form; 16 385: the row-per-wave form (a one-stage chain, which is still small); k_in = 512: row_*_k512 at any M; D = 384:
    always split."""
    for M, form in ((16384, f"split_{NAME[T]}_d256"), (16385, f"row_{NAME[T]}_d256_res0_q0")):
        run_row(row_case("side1_4", 256, T, M), form, f"routing {NAME[T]} M{M}")
    for M in (1, 33):
        run_row(row_case("refpoint", 256, T, M), f"row_{NAME[T]}_d256_k512", f"routing {NAME[T]} k512 M{M}")
    run_row(row_case("side1_4", 384, T, 16385), f"split_{NAME[T]}_d384", f"routing {NAME[T]} d384 M16385")


# ------------------------------------------------------------------------------------------------------------ enc-chain cases
ENC_FORMS = [(256, 640), (256, 0), (384, 0)]
GEO = dict(B=3, npix=50, S=87, lsi=19)               # total_rows = B S + 5: waves straddle images, a level offset applies
GEO_BIG = dict(B=3, npix=100, S=137, lsi=19)         # 300 rows: more than one workgroup
# (M, geometry, nl, index into the class counts of the width, ld_in - k, ld_cls - cols)
ENC_SHAPES = [(1, GEO, 1, 0, 0, 0), (31, GEO, 2, 1, 8, 8), (33, GEO, 3, 2, 0, 0), (127, GEO, 6, 3, 16, 8), (129, GEO, 3, 4, 0, 0), (150, GEO, 2, 5, 8, 0),
              (300, GEO_BIG, 3, 4, 8, 8)]
NCLS = {"narrow": [1, 31, 32, 33, 91, 96], "wide": [97, 366, 384, 366, 97, 384]}


def enc_form(T, D, k5, width):
    return f"enc_{NAME[T]}_d{D}_pf{int(bool(k5))}_{width}"


def enc_case(D, k5, T, width, M, geo, nl, ncls, seed=0, gp=None, xscale=None):
    """Seeds: `seed` is chosen (0 everywhere so far) so that the f32 emulation of tests/test_chain_bound_host.py stays within SHARE of the tight bound."""
    def build():
        g = torch.Generator().manual_seed(9000 + seed + D + k5 + ncls + nl)
        r = lambda *s: torch.randn(*s, generator=g)
        w_enc, b_enc, g_enc, be_enc = r(D, D) / 16, r(D) * 0.5, 1 + 0.2 * r(D), 0.2 * r(D)
        w_cls, b_cls = r(ncls, D) / 16, r(ncls)
        w_val, b_val = r(nl * D, D) / 16, r(nl * D) * 0.5
        cv2 = (r(D, k5) / 25, r(D) * 0.5, (1 + 0.2 * r(D)) if gp is None else torch.full((D,), float(gp)), 0.2 * r(D)) if k5 else None
        stream, vec = K.pack_enc_chain(D, T, w_enc, b_enc, g_enc, be_enc, w_cls, b_cls, w_val, b_val, cv2=cv2)
        cols = K.enc_chain_class_cols(ncls)
        B, npix, S, lsi = geo["B"], geo["npix"], geo["S"], geo["lsi"]
        total = B * S + 5
        gx = torch.Generator().manual_seed(9100 + seed + M + D + k5)
        x = (torch.randn(M, k5 or D, generator=gx) * ((1.0 if k5 else 1.5) if xscale is None else xscale)).to(T)
        rowvalid = (torch.rand(total, generator=gx) > 0.3).to(torch.uint8)
        notpad = (torch.rand(total, generator=gx) > 0.25).to(torch.uint8)
        rowvalid[S:2 * S] = 0                        # one image with all flags zero
        notpad[S:2 * S] = 0
        m = torch.arange(M)
        mm = (m // npix) * S + lsi + m % npix
        case = dict(D=D, k5=k5, T=T, width=width, M=M, geo=geo, nl=nl, ncls=ncls, cols=cols, total=total, stream=stream, vec=vec, x=x, rowvalid=rowvalid, notpad=notpad,
                    mm=mm, eps_p=1e-6, eps_e=1e-5)
        if M > 8 and M <= total:                     # flag[m] differs from flag[mm] on many rows: indexing by the input row is not the same thing
            assert int((rowvalid[m] != rowvalid[mm]).sum()) > M // 8 and int((notpad[m] != notpad[mm]).sum()) > M // 8
        dense = enc_dense(stream, vec, D, k5, nl, cols)
        for mode in ("tight", "worst"):
            case[mode] = enc_reference(x, rowvalid[mm].double(), notpad[mm].double(), dense, D, k5, nl, T, mode, 1e-6, 1e-5)
        return case
    return cached(("enc", D, k5, T, width, M, geo["npix"], nl, ncls, seed, gp, xscale), build)


class EncRun:
    """One lwdetr_enc_chain call on guarded (total_rows, .) buffers, straight through the C entry."""

    def __init__(self, case, ld_in_extra=0, ld_cls_extra=0, over=None):
        c, D, T = case, case["D"], case["T"]
        over = over or {}
        total, nl = c["total"], c["nl"]
        self.case = c
        self.x = Buf(c["M"], (c["k5"] or D) + ld_in_extra, T, pre=4, post=4, fill=PADV)
        self.x.load(c["x"])
        self.memory = Buf(total, D, T, pre=4, post=4) if c["k5"] else None
        self.om = Buf(total, D, T, pre=4, post=4)
        self.cls = Buf(total, c["cols"] + ld_cls_extra, T, pre=4, post=4)
        self.cmax = Buf(total, 1, torch.float32, pre=4, post=4)
        self.values = [Buf(total, D, T, pre=4, post=4) for _ in range(nl)]
        self.rv, self.npd = over.get("rowvalid", c["rowvalid"]).to(_dev()), over.get("notpad", c["notpad"]).to(_dev())
        self.stream, self.vec = over.get("stream", c["stream"]).to(_dev()), over.get("vec", c["vec"]).to(_dev())
        self.outs = dict(om=self.om, cls=self.cls, cls_max=self.cmax, **{f"values{i}": v for i, v in enumerate(self.values)})
        if self.memory:
            self.outs["memory"] = self.memory
        for b in self.outs.values():
            b.freeze()
        self._vals = (C.c_void_p * nl)(*[v.ptr() for v in self.values])
        g = c["geo"]
        self.args = (self.x.ptr(), self.x.ld, c["k5"], self.memory.ptr() if self.memory else None, self.om.ptr(), self.cls.ptr(), self.cls.ld, self.cmax.ptr(),
                     self._vals, nl, self.rv.data_ptr(), self.npd.data_ptr(), self.stream.data_ptr(), self.vec.data_ptr(), c["M"], D, g["npix"], g["S"], g["lsi"],
                     total, c["ncls"])
        lib = _native.lib()
        assert self.stream.numel() * 2 == lib.lwdetr_enc_chain_pieces_cls(D, c["k5"], nl, c["ncls"]) * 4096
        assert self.vec.numel() == lib.lwdetr_enc_chain_vec_floats_cls(D, c["k5"], c["ncls"])

    def launch(self):
        c = self.case
        lib = _native.lib()
        code = _native.dtype_code(c["T"])
        assert lib.lwdetr_enc_chain_check(*self.args, code) == 0
        return lib.lwdetr_enc_chain(*self.args, c["eps_p"], c["eps_e"], code, _native.stream_ptr())


def run_enc(case, label, ld_in_extra=0, ld_cls_extra=0, over=None, check_ref=True):
    """Launch (pinned), repeat, the exact checks, element-wise check. Returns {name: rows as stored at the launch's memory rows}."""
    T, D, cols, ncls, mm = case["T"], case["D"], case["cols"], case["ncls"], case["mm"]
    form = enc_form(T, D, case["k5"], case["width"])
    run = EncRun(case, ld_in_extra, ld_cls_extra, over)
    with chain_served_by(form):
        assert run.launch() == 0, label
    first = {n: b.buf.clone() for n, b in run.outs.items()}
    with chain_served_by(form):
        assert run.launch() == 0, label
    other = torch.ones(case["total"], dtype=torch.bool)
    other[mm] = False
    got = {}
    for n, b in run.outs.items():
        assert torch.equal(b.buf.view(torch.uint8), first[n].view(torch.uint8)), f"{label}: {n}: a repeated launch gives other bits"
        w = cols if n == "cls" else b.ld
        assert b.guards_intact(0, w), f"{label}: {n}: written outside rows [0, total_rows) x columns [0, {w})"
        body = b.body(0, w).cpu()
        snap = b.snap[b.pre:b.pre + b.rows, :w].cpu()
        assert torch.equal(body[other].view(torch.uint8), snap[other].view(torch.uint8)), f"{label}: {n}: rows of other levels / images were written"
        got[n] = body[mm]
    logits = got["cls"]
    assert bool((logits[:, ncls:] == 0).all()), f"{label}: class columns [{ncls}, {cols}) are not zero"
    assert torch.equal(got["cls_max"][:, 0], logits[:, :ncls].float().max(1).values), f"{label}: cls_max is not the maximum of the stored logits"
    npd = (over or {}).get("notpad", case["notpad"])[mm]
    vals = torch.cat([got[f"values{i}"] for i in range(case["nl"])], 1)
    assert bool((vals[npd == 0] == 0).all()) and not bool(torch.signbit(vals[npd == 0]).any()), f"{label}: value rows of padded pixels are not exact zeros"
    got["values"] = vals
    if check_ref:
        for n in ("memory", "values", "om", "cls") if case["k5"] else ("values", "om", "cls"):
            check(form, got[n], case["tight"][n], case["worst"][n], T, f"{label} {n}")
    return got


def enc_params():
    out = []
    for T in (F16, BF16):
        for D, k5 in ENC_FORMS:
            for width in ("narrow", "wide"):
                for M, geo, nl, ci, li, lc in ENC_SHAPES:
                    ncls = NCLS[width][ci]
                    out.append(pytest.param(T, D, k5, width, M, geo, nl, ncls, li, lc, id=_case_id("enc", T, D, k5, width, M, nl, ncls)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,k5,width,M,geo,nl,ncls,li,lc", enc_params())
def test_enc_chain_vs_fp64(T, D, k5, width, M, geo, nl, ncls, li, lc, request):
    run_enc(enc_case(D, k5, T, width, M, geo, nl, ncls), request.node.callspec.id, li, lc)
    RAN.add(request.node.callspec.id)


# ------------------------------------------------------------------------------------------------------------ transcendentals, made visible
def rstd_case(D, T, seed):
    return cached(("rstd", D, T, seed), lambda: _rstd_case(D, T, seed))


def _rstd_case(D, T, seed):
    """One FULL + LN + STORE stage with the identity as its weight, gamma = 2^14, beta = -fl32(2^14 z) of the float64 z of the ONE input row."""
    g = torch.Generator().manual_seed(500 + seed + D)
    x = (torch.randn(1, D, generator=g) * (0.5 + seed) + 0.3 * seed).to(T)
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    dd = xd - mean
    z = dd / torch.sqrt((dd * dd).mean(1, keepdim=True) + float(np.float32(1e-5)))
    gam = torch.full((D,), 2.0 ** 14)
    bet = (-(z[0] * 2.0 ** 14)).float()
    st = [dict(kind="full", w=torch.eye(D), b=torch.zeros(D), ln=(gam, bet, 1e-5), store=True)]
    stream, vec = K.RowChainOp.pack(D, T, D, st)
    plain = [dict(kind="full", ln=1e-5, store=True)]
    case = dict(name="rstd", D=D, T=T, M=1, k_in=D, stages=plain, stream=stream, vec=vec, x=x, res=None, qpos=None, ld={}, z=z[0])
    dense = row_dense(stream, vec, D, D, plain)
    assert torch.equal(dense[0]["W"], torch.eye(D, dtype=torch.float64))
    for two in (False, True):
        for mode in ("tight", "worst"):
            case[mode, two] = row_reference(x, None, None, dense, D, D, plain, T, mode, two)
    e_ln = ln_affine(xd, torch.zeros_like(xd), torch.zeros_like(xd), gam.double(), bet.double(), 1e-5, T, "worst", 0.0)[4]
    case["arith"] = e_ln[0] / z[0].abs().clamp_min(1e-30)               # relative, without the transcendental
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("T,D,rowform", [(F16, 256, False), (BF16, 256, False), (F16, 384, False), (BF16, 384, False), (F16, 256, True), (BF16, 256, True)],
                         ids=lambda v: NAME.get(v, str(v)))
def test_chain_rstd_measured(T, D, rowform):
    """1 / sqrtf made visible (module docstring): the deviation of the kernel's f32 z from the float64 z of its own stored row, and the check that it
    stays within the derived arithmetic + TRANS_F32."""
    form = f"row_{NAME[T]}_d256_res0_q0" if rowform else f"split_{NAME[T]}_d{D}"
    worst_raw = worst_dev = 0.0
    if rowform:
        _native.tuning_set("CHAIN_SPLIT_ROWS", 0)
    try:
        for seed in range(8):
            case = rstd_case(D, T, seed)
            got = run_row(case, form, f"rstd {form} seed {seed}")[0][0].double()
            z = case["z"]
            sel = z.abs() >= 0.5
            # stored = T(2^14 z^ + beta): z^ - z = (stored - (2^14 z + beta)) 2^-14 up to the rounding of the small stored number (2^-10 of itself)
            dz = (got - (z * 2.0 ** 14 + case["vec"][2 * D:3 * D].double())) * 2.0 ** -14
            raw = (dz.abs() / z.abs())[sel]
            dev = (raw - case["arith"][sel] - 2.0 ** -9 * raw).clamp_min(0)
            worst_raw, worst_dev = max(worst_raw, float(raw.max())), max(worst_dev, float(dev.max()))
    finally:
        if rowform:
            _native.tuning_set("CHAIN_SPLIT_ROWS", None)
    print(f"CHAIN_TRANS rstd {form}: relative deviation of z {worst_raw / U23:.3f} x 2^-23 (beyond the derived arithmetic: {worst_dev / U23:.3f} x 2^-23)")
    assert worst_dev <= TRANS_F32, f"{form}: 1 / sqrtf deviates by {worst_dev / U23:.3f} x 2^-23 beyond the arithmetic, TRANS_F32 is {TRANS_F32 / U23:.0f} x 2^-23"


@pytest.mark.gpu
@pytest.mark.parametrize("T", [F16, BF16], ids=lambda v: NAME[v])
def test_chain_silu_measured(T):
    """SiLU made visible (module docstring): LayerNorm2d gamma = 8 keeps neighbouring T numbers of the SiLU output apart in `memory`; input rows scaled so
    that the arguments cover [-8, 8]. Reports the largest |memory^ - memory| beyond the worst-case bound with TRANS_F32 = 0."""
    case = enc_case(256, 640, T, "narrow", 150, GEO, 1, 91, gp=8.0, xscale=2.5)
    got = run_enc(case, f"silu {NAME[T]}")
    dense = enc_dense(case["stream"], case["vec"], 256, 640, 1, case["cols"])
    mm = case["mm"]
    ref0 = enc_reference(case["x"], case["rowvalid"][mm].double(), case["notpad"][mm].double(), dense, 256, 640, 1, T, "worst", 1e-6, 1e-5, trans=0.0)
    y, e = ref0["memory"]
    err = (got["memory"].double() - y).abs()
    excess = ((err - bound_of(y, e, T)).clamp_min(0) / y.abs().clamp_min(2.0 ** -14))
    a = case["x"].double() @ dense["w2"].t() + dense["b2"]
    print(f"CHAIN_TRANS silu {NAME[T]}: arguments in [{float(a.min()):.2f}, {float(a.max()):.2f}]; |memory^ - memory| beyond the bound without a transcendental term: "
          f"{float(excess.max()) / U23:.3f} x 2^-23 relative ({int((excess > 0).sum())} of {excess.numel()} elements)")
    # The printed excess is a MEASUREMENT (what TRANS_MEASURED rests on), not what this test asserts. What it asserts is run_enc's comparison above: every
    # element inside the worst-case bound WITH the transcendental term (TRANS_F32 = 4 TRANS_MEASURED), at most SHARE outside the tight one.


# ------------------------------------------------------------------------------------------------------------ refusals (nothing launched)
@pytest.mark.gpu
def test_chain_refusals_launch_nothing():
    """Every refusal of the two entries (tests/test_chain_refusals_host.py: the same calls, which need no GPU), in a process that has the GPU open: no
    counter of the record moves and the device reports no error afterwards."""
    from tests import test_chain_refusals_host as H
    before = _native.chain_path_counts()
    for fn in (H.test_row_chain_refuses_strides_shorter_than_the_row_whatever_m_is, H.test_row_chain_stage_rules_come_after_the_m0_return,
               H.test_row_chain_unsupported_forms_launch_nothing, H.test_enc_chain_refuses_an_input_stride_shorter_than_the_row,
               H.test_enc_chain_compares_the_largest_memory_row_with_total_rows, H.test_enc_chain_check_answers_for_the_values_array_as_the_entry_does,
               H.test_enc_chain_keeps_its_older_refusals):
        fn()
    torch.cuda.synchronize()
    assert _native.chain_path_counts() == before


# ------------------------------------------------------------------------------------------------------------ sensitivity
SENS_ROW = ("front", 256, F16, 33)
SENS_ENC = (256, 0, F16, "narrow", 129, GEO, 2, 91)


def _row_alt(case, stream=None, vec=None, res=None, qpos=None):
    stream, vec = case["stream"] if stream is None else stream, case["vec"] if vec is None else vec
    dense = row_dense(stream, vec, case["D"], case["k_in"], case["stages"])
    return row_reference(case["x"], case["res"] if res is None else res, case["qpos"] if qpos is None else qpos, dense, case["D"], case["k_in"], case["stages"],
                         case["T"], "tight", True)


def _sens_row(label, dependent, **over):
    """Launch the split form with ONE operand altered; the comparison with the ORIGINAL reference must fail on exactly the dependent elements."""
    case = row_case(*SENS_ROW)
    D, T = case["D"], case["T"]
    got = run_row(case, f"split_{NAME[T]}_d{D}", label, over=over, check_ref=False)
    alt = _row_alt(case, **over)
    noa = case["stages"][1]["n"]
    cut = lambda ref: {"out": ref[0], "side": (ref[1][0][:, :noa], ref[1][1][:, :noa])}
    dep = {"out": dependent[0].expand(case["M"], D), "side": dependent[1].expand(case["M"], noa)}
    fails_exactly({"out": got[0], "side": got[1]}, {"tight": cut(case["tight", True])}, cut(alt), T, label, dep)


def _mask(shape, rows=None, cols=None):
    m = torch.zeros(shape, dtype=torch.bool)
    m[slice(None) if rows is None else rows, slice(None) if cols is None else cols] = True
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["side bias", "gamma", "weight", "pieces", "res", "qpos"])
def test_row_chain_sensitivity(what):
    case = row_case(*SENS_ROW)
    D, M = case["D"], case["M"]
    noa = case["stages"][1]["n"]
    vec, stream = case["vec"].clone(), case["stream"].clone()
    none, every = torch.zeros(1, 1, dtype=torch.bool), torch.ones(1, 1, dtype=torch.bool)
    full_pieces = D // 32 * (D // 64)                # pieces of stage 0; the SIDE stage follows
    if what == "side bias":                          # one bias entry of one tile: column 37 of the SIDE output
        vec[3 * D + 37] += 0.05
        _sens_row(what, (none, _mask((1, noa), cols=[37])), vec=vec)
    elif what == "gamma":                            # one gamma entry: that column of the stored row, and every SIDE element through the operand
        vec[D + 5] *= 1.25
        _sens_row(what, (_mask((1, D), cols=[5]), every), vec=vec)
    elif what == "weight":                           # one element inside the packed stream (SIDE stage, tile 1): one output column
        p = (full_pieces + 1 * (D // 64) + 2) * 2048 + 777
        stream[p] = stream[p] + 0.25
        w0, w1 = (row_dense(s, case["vec"], D, D, case["stages"])[1]["W"] for s in (case["stream"], stream))
        cols = (w0 != w1).any(1).nonzero().flatten().tolist()
        assert len(cols) == 1 and cols[0] // 32 == 1
        _sens_row(what, (none, _mask((1, noa), cols=[c for c in cols if c < noa])), stream=stream)
    elif what == "pieces":                           # two exchanged pieces of one tile (SIDE stage, tile 2): its 32 columns
        a, b = (full_pieces + 2 * (D // 64) + 0) * 2048, (full_pieces + 2 * (D // 64) + 3) * 2048
        pa = stream[a:a + 2048].clone()
        stream[a:a + 2048] = stream[b:b + 2048]
        stream[b:b + 2048] = pa
        _sens_row(what, (none, _mask((1, noa), cols=list(range(64, 96)))), stream=stream)
    elif what == "res":                              # one residual element: its row, through the LayerNorm, and that row of the SIDE output
        res = case["res"].clone()
        res[M - 2, 40] += 1.0
        _sens_row(what, (_mask((M, D), rows=[M - 2]), _mask((M, noa), rows=[M - 2])), res=res)
    else:                                            # one qpos element: the stored row is y (unchanged), the SIDE output of that row moves
        qpos = case["qpos"].clone()
        qpos[9, 200] += 1.0
        _sens_row(what, (torch.zeros(M, D, dtype=torch.bool), _mask((M, noa), rows=[9])), qpos=qpos)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["rowvalid", "notpad"])
def test_enc_chain_sensitivity_one_flag(what):
    """One flag of one MEMORY row flipped, at a row whose input-row flag differs from its memory-row flag: exactly that row's outputs move."""
    case = enc_case(*SENS_ENC)
    T, D, nl, mm, M = case["T"], case["D"], case["nl"], case["mm"], case["M"]
    flags = case[what].clone()
    r = next(i for i in range(M) if case[what][mm[i]] == 1 and case[what][i] == 0)          # flag[mm] set, flag[m] clear: the two indexings disagree here
    flags[mm[r]] = 0
    got = run_enc(case, f"sens {what}", over={what: flags}, check_ref=False)
    dense = enc_dense(case["stream"], case["vec"], D, 0, nl, case["cols"])
    rv = (flags if what == "rowvalid" else case["rowvalid"])[mm].double()
    npd = (flags if what == "notpad" else case["notpad"])[mm].double()
    alt = enc_reference(case["x"], rv, npd, dense, D, 0, nl, T, "tight", 1e-6, 1e-5)
    names = ("values", "om", "cls")
    moved = {"rowvalid": ("om", "cls"), "notpad": ("values",)}[what]
    dep = {n: _mask(tuple(case["tight"][n][0].shape), rows=[r]) if n in moved else torch.zeros(tuple(case["tight"][n][0].shape), dtype=torch.bool) for n in names}
    fails_exactly({n: got[n] for n in names}, {"tight": {n: case["tight"][n] for n in names}}, {n: alt[n] for n in names}, T, f"sens {what}", dep)


# ------------------------------------------------------------------------------------------------------------ the record
@pytest.mark.gpu
def test_chain_every_instantiation_was_launched():
    """All 24 names of the record were launched by this module's element-wise cases. Meaningful only when all of them ran in this process."""
    if not ALL_CASES <= RAN:
        pytest.skip(f"{len(ALL_CASES - RAN)} of the {len(ALL_CASES)} element-wise cases did not run in this process")
    counts = _native.chain_path_counts()
    assert sorted(counts) == sorted(ALL_FORMS)
    missing = [f for f in ALL_FORMS if f not in FORM_WORST]
    assert not missing, f"never launched and checked: {missing}"
    assert all(counts[f] > 0 for f in ALL_FORMS)
