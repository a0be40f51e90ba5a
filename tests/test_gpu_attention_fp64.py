"""The kernels of csrc/attention.hip (lwdetr_attention: attn_kernel, attn_win_kernel, the LDS-ring kernel attn_lds_kernel, attn_wtile_kernel in
LWDETR_EXPERIMENTS builds), called directly through K.AttnOp at the smallest shapes at which their key masks, ragged tiles, clamped loads, query
tiling, work split and launch forms can go wrong. Every launch is pinned to ONE instantiation by the launch-form record (lwdetr_attn_path_counts,
helpers.attn_served_by) and every output is checked ELEMENT BY ELEMENT against a float64 evaluation of the same operation on the operands as
stored. Outputs live in larger buffers (guard rows before and after, ldo > heads hd, seq_tok_stride > keys_per_seq) filled with a sentinel: every
element outside rows q < keys_per_seq x columns [0, heads hd) must come back bit-identical. Every launch runs twice, with the K rows / V^T columns
that no sequence may use (pad rows inside a sequence, keys behind sub_len, rows between and behind the sequences) at 0 and at +-30000: the two
outputs must be bit-identical. tests/test_gpu_kernels.py keeps its norm-wise attention tests as the cross-check.

Reference. Q is stored pre-scaled (hd^-0.5 log2 e: the kernels work in the log2 domain), K and V^T are widened exactly. Real keys
R = {j < keys_per_seq : j % sub_stride < sub_len}; s_k = q . k, M = max_R s, p_k = 2^(s_k - M), a_k = p_k / sum_R p, y_c = sum_R a_k v_kc, for EVERY
row q < keys_per_seq of every sequence - pad rows are queries like any other, every kernel computes and stores them.

Bound. The stored number may differ from y by half_ulp_T(|y| + E) + E (half_ulp of test_gpu_rowops), E = E_W + E_ACC per element from the
reference's own numbers; u = 2^-24 is one f32 rounding, U23 = 2 u, u_T = 2^-11 (f16), 2^-8 (bf16), 0 (f32 forms: P stays f32).
  Weights. The kernel's weight of key k is p_k (1 + r_k) up to a factor common to the row, |r_k| <= R_k. A common factor cancels in the
    normalisation, so y' - y = sum a_k r_k (v_kc - y_c) / (1 + sum a_k r_k) and
        E_W = sum_R a_k R_k |v_kc - y_c| / (1 - sum_R a_k R_k),        R_k = u_T + rho_k:
    E_P: P is rounded to T before the P V MFMA, |delta_k| <= u_T, and the denominator sums the same rounded P (attn_kernel: an MFMA against a ones
      operand; ring kernel: the ones row of the V^T image at hd 16, v_dot2 on the packed P above; attn_win at hd 16 and wtile: the ones row) - the
      u_T above. f16 only: a weight with 2^(s_k - M) < 2^-14 may be a subnormal f16 or lost whole (the kernels' lazy reference is never above M,
      so every larger weight is a normal f16 number): R_k = 1 for such a key.
      attn_win_kernel at hd 32 adds the UNROUNDED exponential into its denominator, so there nothing cancels: R_k = rho_k only and
        E_P = (u_T sum_R a_k (1 + rho_k) |v_kc| + sum_lost a_k |v_kc|) / (1 - sum_R a_k rho_k)      is added instead.
    E_S: the f32 score s' = fl(-m + sum_d q_d k_d) (m: the running reference, the C operand of the score MFMA) differs from s_k - m by at most
      eps_k = U23 ((hd + 1) sum_d |q_d k_d| + (n_resc + 2) S), S = max_R |s| of that row >= |m|: hd + 1 accumulations (a 16-bit product is exact
      in f32; an f32 one rounds, U23 = 2 u covers product and sum), the subtraction of a new reference from the scores (one rounding at
      <= |s| + |m|), and n_resc roundings of the reference itself, fl(negm - mx), one per step that may move it (attn_kernel: a step is 32 keys;
      ring: 2 per 64-key block; attn_win / wtile take the exact row maximum: none). exp2 is the hardware's: TRANS_F32. Rescale factors alpha
      multiply O and l alike and cancel (their product roundings are in E_ACC). rho_k = 1.01 ln 2 eps_k + TRANS_F32.
  E_ACC = n_acc U23 sum_R a_k |v_kc| + (n_acc U23 + TRANS_F32 + U23) |y_c|: f32 accumulation of O over the P V MFMAs (one rounding per k-slot and
    one per rescale, on the safe side: the MFMA's internal summation is not documented), the same for the denominator l, then 1.f / l (TRANS_F32)
    and the product. n_acc = 33 ceil(keys / 32) + 2 (attn_kernel: one K = 32 MFMA and at most one rescale per step), 66 ceil(keys / 64) + 2 (ring:
    two K = 16 MFMAs per 32-key group), 16 ceil(min(sub_len, keys) / 16) + 2 (attn_win / wtile: one K = 16 MFMA per 16-key chunk).
No term is scaled by a tensor-wide maximum, and no share of elements is exempt: every element must meet its bound.

Hardware transcendentals: TRANS_F32 = 4 TRANS_MEASURED (the project's margin). u_T hides them in the 16-bit forms; in the f32 forms they are the
bound, so they are measured: test_attn_softmax_weights_measured runs the f32 forms on a V whose column k is 1 at channel k for the first hd keys
and 0 elsewhere - output channel c then IS the softmax weight of key c - with logits within a few units. TRANS_MEASURED is the larger of the worst
relative deviation of such a weight from the float64 one and one f32 ulp. Measured on an MI355X over 200 keys x 2 heads (the raw figure: the f32
accumulation of the denominator over 200 keys is in it and is counted again in E_ACC, on the safe side; the scores themselves are exact by
construction): 7.327 (hd 16, qt2 and qt4), 5.580 (hd 32, both), 6.782 (hd 64) x 2^-23, so TRANS_MEASURED = 7.327 x 2^-23
(profiles/r9b_attention_fp64_worst_ratios.txt, which also lists the worst |diff| / bound per launch form).

Inputs. N(0, 1) values rounded to T, plus weight on the keys whose handling can go wrong (k = c q for a designated query, c chosen so that the key
holds a visible share of its row): the first and last key of a 32-key step and of a 64-key block, the last real key, the keys before and after a
hole, the first key of the ragged last tile and of the last 4-key run; spread over queries of different waves, query tiles, heads and images,
the last query of the sequence and the first of the last workgroup among them. Three rows per chosen sequence hold the rescale regimes: a late
key just under 2^8 above the running reference (no rescale, P near 200), one further above (a rescale late in the sequence), and one row whose
other weights fall to f16 subnormals. tests/test_attention_bound_host.py shows on the CPU, on exactly these cases, that an independent f32
evaluation stays inside this bound and that each of twelve planted mistakes leaves it.
"""
import math

import pytest
import torch

from lwdetr_amd import _native
from tests import test_gpu_rowops as R
from tests.helpers import attn_served_by
from tests.test_gpu_rowops import U23, SENT, F16, BF16, F32

NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
UT = {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}
LOG2E = math.log2(math.e)
# the larger of the measured relative deviation of an f32 softmax weight (test_attn_softmax_weights_measured; module docstring) and one f32 ulp
TRANS_MEASURED = 7.327 * 2.0 ** -23
TRANS_F32 = 4 * TRANS_MEASURED
BIG = 30000.0                 # second fill of the rows no sequence may use: finite in every type
GUARD = 4                     # sentinel rows before and after the output
BAD_ARG, UNSUPPORTED = _native.ERR_BAD_ARG, _native.ERR_UNSUPPORTED
RING_CFGS = [102, 103, 104, 105, 106, 108, 110, 204, 205, 208, 1104, 1105, 1108, 1110, 3108, 1208]      # the switch of launch_lds_cfg
WORST = {}                    # launch form -> largest |diff| / bound seen
RAN = set()                   # the element-wise cases that ran to their end in this process

_CACHE = {}


def cached(key, fn):
    """Cases and references are computed once and shared between the tests that need them; nothing modifies them."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def ref_device():
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


# ------------------------------------------------------------------------------------------------------------ geometry and inputs
def geo(keys, spi=1, gap=4, sub=None, B=1, heads=2, slack=False):
    """A descriptor geometry: spi sequences of `keys` rows, keys + gap rows apart, 4 more rows behind the last one."""
    sub_stride, sub_len = sub or (keys, keys)
    stride = keys + gap
    return dict(keys=keys, spi=spi, stride=stride, sub_stride=sub_stride, sub_len=sub_len, B=B, heads=heads, slack=slack,
                Tp=(spi - 1) * stride + keys + 4)


def real_keys(g):
    j = torch.arange(g["keys"])
    return (j % g["sub_stride"]) < g["sub_len"]


def structural_keys(g):
    """The real keys whose handling can go wrong (module docstring), in order."""
    n, ss, sl = g["keys"], g["sub_stride"], g["sub_len"]
    real = real_keys(g)
    last_real = int(real.nonzero().max())
    want = [0, 31, 32, 63, 64, 127, 128, last_real, (n - 1) // 32 * 32, (n - 1) // 64 * 64, n - 4, n - 8, 15, 16]
    if sl < ss:
        want += [sl - 1, ss, ss + sl - 1, 2 * ss, (last_real // ss) * ss]          # before / after the first holes, the first key of the last run
    out = []
    for k in want:
        if 0 <= k < n and bool(real[k]) and k not in out:
            out.append(k)
    return out


def structural_queries(g):
    """Queries of different waves and query tiles: the last of the sequence, the first of the last 128- / 256-query workgroup, neighbours of
    positions that idle waves or clamped rows would take. Pad rows are among them where the geometry has any."""
    n = g["keys"]
    want = [n - 1, (n - 1) // 128 * 128, 0, 15, 16, 33, 63, 64, 97, 127, 129, (n - 1) // 256 * 256, n // 2, n - 2, (n - 1) // 32 * 32, n - 5]
    out = []
    for q in want:
        if 0 <= q < n and q not in out:
            out.append(q)
    return out


def attn_case(T, hd, gname, g, seed=0):
    return cached(("case", T, hd, gname), lambda: _attn_case(T, hd, gname, g, seed))


def seq_rows(g, ext=0):
    """(spi, keys + ext) token rows of the sequences."""
    return torch.arange(g["spi"])[:, None] * g["stride"] + torch.arange(g["keys"] + ext)[None, :]


def seq_views(g, X, ext=0):
    """(B, heads, Tp, hd) -> (B, heads, spi, keys + ext, hd)."""
    return X[:, :, seq_rows(g, ext)]


def _attn_case(T, hd, gname, g, seed):
    B, H, Tp, n, W = g["B"], g["heads"], g["Tp"], g["keys"], g["spi"]
    real = real_keys(g)
    skeys, squeries = structural_keys(g), structural_queries(g)
    free_real = [k for k in range(n) if bool(real[k]) and k not in skeys]
    specials = len(free_real) >= 8 and max(free_real) >= 32          # a key in a later step than the first exists
    for attempt in range(32):
        gen = torch.Generator().manual_seed(1000003 * seed + 7919 * attempt + 31 * hd + n)
        q = torch.randn(B, H, Tp, hd, generator=gen, dtype=torch.float64)
        k = torch.randn(B, H, Tp, hd, generator=gen, dtype=torch.float64).to(T)
        v = torch.randn(B, H, Tp, hd, generator=gen, dtype=torch.float64).to(T)
        qs = (q * (hd ** -0.5 * LOG2E)).to(T)
        # the share a designated key gets: its score is log2(real keys) + 1 above 0, the level of an ordinary score
        target = math.log2(int(real.sum())) + 1.0
        pid = 0
        rows = []               # (b, h, w, kind, query, keys): the rescale-regime rows
        for b in range(B):
            for h in range(H):
                for w in range(W):
                    t0 = w * g["stride"]
                    for j, kj in enumerate(skeys):
                        qi = squeries[(j + pid) % len(squeries)]
                        qv = qs[b, h, t0 + qi].double()
                        k[b, h, t0 + kj] = (qv * (target / float(qv @ qv))).to(T)
                    if specials and pid in (0, B * H * W - 1):
                        taken = set(squeries)
                        pick = lambda near: next(r for d in range(n) for r in (near + d, near - d) if 0 <= r < n and r not in taken)
                        early = [e for e in free_real if e < 32][:3]
                        late = [e for e in reversed(free_real) if e >= 32][:2]
                        if len(early) == 3 and len(late) == 2:
                            for kind, near, ek, lk, rise in (("under8", 5, early[0], late[0], 7.5), ("over8", n // 2 + 1, early[1], late[1], 12.0),
                                                             ("subnormal", n - 3, early[2], None, 18.0)):
                                r = pick(near)
                                taken.add(r)
                                qv = qs[b, h, t0 + r].double()
                                kk = k[b, h, t0:t0 + n].double()
                                others = [x for x in range(n) if bool(real[x]) and x not in (ek, lk)]
                                m0 = float((kk[others] @ qv).max())
                                if kind == "subnormal":
                                    k[b, h, t0 + ek] = (qv * ((m0 + rise) / float(qv @ qv))).to(T)
                                else:
                                    k[b, h, t0 + ek] = (qv * ((m0 + 2.0) / float(qv @ qv))).to(T)
                                    k[b, h, t0 + lk] = (qv * ((m0 + 2.0 + rise) / float(qv @ qv))).to(T)
                                rows.append((b, h, w, kind, r, ek, lk))
                    pid += 1
        case = dict(T=T, hd=hd, g=g, gname=gname, qs=qs, k=k, v=v, real=real, skeys=skeys, squeries=squeries, rows=rows)
        if _regimes_ok(case):
            return case
    raise AssertionError(f"no seed gave the rescale regimes for {gname} hd {hd} {NAME[T]}")


def _regimes_ok(case):
    """The three regime rows are what they are meant to be, judged on the stored operands in float64 (32-key steps, as attn_kernel takes them)."""
    g, real, n = case["g"], case["real"], case["g"]["keys"]
    for b, h, w, kind, r, ek, lk in case["rows"]:
        t0 = w * g["stride"]
        s = case["k"][b, h, t0:t0 + n].double() @ case["qs"][b, h, t0 + r].double()
        s = s.masked_fill(~real, -math.inf)
        if kind == "subnormal":
            d = s - s.max()
            if not bool(((d < -14) & (d > -24)).any()):
                return False
            continue
        before = float(s[:lk // 32 * 32].max())                  # the largest score of the steps before the late key's
        rise = float(s[lk]) - before
        if kind == "under8" and not (6.5 < rise < 7.9 and float(s.max()) == float(s[lk])):
            return False
        if kind == "over8" and not rise > 8.5:
            return False
    return True


def free_rows(g):
    """(Tp,) bool: the token rows that are no real key of any sequence."""
    free = torch.ones(g["Tp"], dtype=torch.bool)
    rows = seq_rows(g)
    free[rows[:, real_keys(g)].flatten()] = False
    return free


def operands(case, fill=0.0):
    """(Q, K, V) as stored, (B, heads, Tp, hd) of T on the CPU, the K rows / V rows that no sequence may use at +-fill."""
    g = case["g"]
    free = free_rows(g)
    sign = torch.where(torch.arange(g["Tp"]) % 2 == 0, 1.0, -1.0)[:, None].expand(g["Tp"], case["hd"])
    k, v = case["k"].clone(), case["v"].clone()
    k[:, :, free] = (fill * sign[free]).to(case["T"])
    v[:, :, free] = (-fill * sign[free]).to(case["T"])
    return case["qs"], k, v


# ------------------------------------------------------------------------------------------------------------ float64 reference and bound
def family(form):
    return form.split("_")[1]           # wave, win, ring, wtile


def counts(fam, g):
    """(n_resc, n_acc) of the module docstring."""
    n = g["keys"]
    if fam == "wave":
        steps = -(-n // 32)
        return steps, 33 * steps + 2
    if fam == "ring":
        nblk = -(-n // 64)
        return 2 * nblk, 66 * nblk + 2
    return 0, 16 * -(-min(g["sub_len"], n) // 16) + 2


def reference(case, fam):
    """y and its bound, (B, spi, keys, heads hd) float64 on the CPU. fam: wave / ring / win (wtile = win at hd 16)."""
    fam = "win" if fam == "wtile" else fam
    return cached(("ref", id(case), fam), lambda: _reference(case, fam))


def _reference(case, fam):
    T, hd, g = case["T"], case["hd"], case["g"]
    dev = ref_device()
    qs, k, v = operands(case)
    q, k, v = (seq_views(g, x).double().to(dev) for x in (qs, k, v))                   # (B, H, W, n, hd)
    real = case["real"].to(dev)
    s = q @ k.transpose(-1, -2)
    aqk = q.abs() @ k.abs().transpose(-1, -2)
    s = s.masked_fill(~real, -math.inf)
    d = s - s.amax(-1, keepdim=True)
    p = torch.exp2(d)
    a = p / p.sum(-1, keepdim=True)
    y = a @ v
    smax = s.masked_fill(~real, 0.0).abs().amax(-1, keepdim=True)
    n_resc, n_acc = counts(fam, g)
    eps = U23 * ((hd + 1) * aqk + (n_resc + 2) * smax)
    rho = 1.01 * math.log(2.0) * eps + TRANS_F32
    lost = (d < -14) & real if T == F16 else torch.zeros_like(d, dtype=torch.bool)
    unrounded = fam == "win" and hd == 32
    Rk = rho if unrounded else torch.where(lost, torch.ones_like(rho), rho + UT[T])
    aR = a * Rk
    D = aR.sum(-1, keepdim=True)
    assert float(D.max()) < 0.5
    n = g["keys"]
    N = torch.empty_like(y)
    pairs = y.numel() // (n * hd)
    chunk = max(1, (1 << 22) // (pairs * n * hd))
    for q0 in range(0, n, chunk):
        q1 = min(n, q0 + chunk)
        N[..., q0:q1, :] = (aR[..., q0:q1, :, None] * (v[..., None, :, :] - y[..., q0:q1, None, :]).abs()).sum(-2)
    E = N / (1 - D)
    av = v.abs()
    if unrounded:
        E = E + (UT[T] * ((a * (1 + rho)) @ av) + (a * lost) @ av) / (1 - D)
    E = E + n_acc * U23 * (a @ av) + (n_acc * U23 + TRANS_F32 + U23) * y.abs()
    bound = R.half_ulp(y.abs() + E, T) + E
    lay = lambda t: t.permute(0, 2, 3, 1, 4).reshape(g["B"], g["spi"], n, g["heads"] * hd).cpu()
    return lay(y), lay(bound)


# ------------------------------------------------------------------------------------------------------------ launching and checking
def out_rows(g):
    """(B, spi, keys) rows of the guarded output buffer that a launch writes."""
    return GUARD + torch.arange(g["B"])[:, None, None] * g["Tp"] + seq_rows(g)[None]


def launch(case, form, fill=0.0, launches=1):
    """One launch through K.AttnOp into a sentinel-filled buffer with guard rows and guard columns; the whole buffer, on the CPU."""
    from lwdetr_amd import kernels as K
    T, hd, g = case["T"], case["hd"], case["g"]
    qs, k, v = (x.cuda() for x in operands(case, fill))
    B, H, Tp = g["B"], g["heads"], g["Tp"]
    vt_store = torch.zeros(v.numel() + 8, dtype=T, device="cuda")              # 16 readable bytes behind V^T (vt_slack)
    vt = vt_store[:v.numel()].view(B, H, hd, Tp)
    vt.copy_(v.transpose(2, 3))
    ldo = H * hd + 8
    buf = torch.full((GUARD + B * Tp + GUARD, ldo), SENT, dtype=T, device="cuda")
    with attn_served_by(form, launches):
        K.AttnOp(qs, k, vt, buf[GUARD:], B=B, heads=H, hd=hd, Tp=Tp, ldo=ldo, seqs_per_img=g["spi"], seq_tok_stride=g["stride"],
                 keys_per_seq=g["keys"], sub_stride=g["sub_stride"], sub_len=g["sub_len"], kind=0, vt_slack=g["slack"])()
    return buf.cpu()


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def check(case, form, label):
    """Two launches (fills 0 and +-30000): bit-identical; the guard untouched; every element of every row inside its bound."""
    g, C = case["g"], case["g"]["heads"] * case["hd"]
    buf = launch(case, form, 0.0)
    buf2 = launch(case, form, BIG)
    assert torch.equal(bits(buf), bits(buf2)), f"{label}: the output depends on K / V^T values of keys that no sequence may use"
    rows = out_rows(g)
    rest = buf.clone()
    rest[rows.flatten(), :C] = SENT
    assert torch.equal(bits(rest), bits(torch.full_like(rest, SENT))), f"{label}: something outside the sequences' rows and channels was written"
    got = buf[rows.flatten(), :C].reshape(*rows.shape, C)
    y, bnd = reference(case, family(form))
    ok, worst, nbad = R.compare(got, y, bnd)
    WORST[form] = max(WORST.get(form, 0.0), worst)
    print(f"ATTN_WORST {form} {label} {worst:.3f}")
    assert ok, f"{label} ({form}): {nbad} elements outside their bound, worst |diff| / bound {worst:.3f}"
    return buf


@pytest.fixture
def routes(knobs):
    """The process-wide overrides of attention.hip, back to their defaults after the test (the knobs fixture clears the switches)."""
    lib = _native.lib()
    yield lib
    lib.lwdetr_attention_tuning(-1)
    lib.lwdetr_attention_tuning_cfg(0)


# ------------------------------------------------------------------------------------------------------------ case tables
WAVE_GEOS = {
    "k8": geo(8, B=2, heads=2), "k12": geo(12, B=2, heads=2), "k44": geo(44, B=2, heads=3),
    "win100": geo(100, spi=16, B=1, heads=2),                        # 16 windows, seq_tok_stride 104
    "dec300": geo(300, B=2, heads=2),                                 # the decoder: 300 % 8 == 4
    "holes192": geo(192, sub=(12, 9), B=1, heads=2),
    "k516": geo(516, B=1, heads=2), "k544": geo(544, B=1, heads=2),  # the >= 512 unconditional-prefetch branch, ragged and even
    "qt200": geo(200, B=1, heads=2),                                  # ATTN_QT=4: clamped query rows, whole query tiles past the end (hd 64: an idle wave)
    "qt132": geo(132, B=1, heads=2),                                  # ATTN_QT=4: three 64-query waves and an idle one; 132 % 8 == 4
    "k128": geo(128, spi=3, B=1, heads=2),                            # the longest sequence of the short form
}
WIN_GEOS = {f"w{twp}_{tw}": geo(twp, spi=spi, sub=(twp, tw), B=1, heads=heads)
            for twp, tw, spi, heads in ((8, 5, 5, 3), (28, 25, 16, 2), (36, 36, 16, 2), (100, 97, 16, 2), (128, 126, 3, 3))}
RING_GEOS = {
    "r708": geo(708, B=1, heads=3, slack=True),                       # 11 blocks + 4 keys: a ragged block, % 8 == 4
    "r64": geo(64, B=1, heads=2),                                     # one block
    "rwin228": geo(228, spi=16, sub=(228, 225), B=1, heads=1, slack=True),
    "rmask512": geo(512, sub=(64, 5), B=1, heads=2),                  # 32-key groups with every key masked
    "r320": geo(320, sub=(80, 77), B=2, heads=1),                     # 5 blocks: the last ring step of the U = 2 forms holds one
}
ALL_GEOS = {**WAVE_GEOS, **WIN_GEOS, **RING_GEOS}


def wave_runs(T, hd, gname):
    """[(form, switches)] of one attn_kernel case: which instantiations it pins and the switches that route there."""
    n = WAVE_GEOS[gname]["keys"]
    if gname in ("qt200", "qt132"):
        return [(f"attn_wave_{NAME[T]}_hd{hd}_qt{4 if hd <= 32 else 2}", {"ATTN_QT": 4})]
    runs = []
    if T != F32 and n <= 128:
        runs.append((f"attn_wave_{NAME[T]}_hd{hd}_qt2_short", {}))
    runs.append((f"attn_wave_{NAME[T]}_hd{hd}_qt2", {"ATTN_SHORT": 0}))
    return runs


def cfg_parts(cfg):
    return cfg % 1000 // 100, cfg % 100, cfg // 1000 + 1            # QT, NW, U


def ring_form(T, hd, cfg):
    return "attn_ring_%s_hd%d_q%dw%du%d" % ((NAME[T], hd) + cfg_parts(cfg))


def ring_fits(hd, cfg):
    """launch_lds: three ring steps of U 64-key K / V^T images and the dummy landing area fit 64 KB (two workgroups per CU)."""
    return 3 * cfg_parts(cfg)[2] * (64 * hd * 2 + max(hd // 32, 1) * 32 * 128) + 1024 <= 65536


def ring_geos(cfg):
    """Every cfg meets the ragged geometry and the all-masked groups; the others are spread over the cfgs."""
    qt, nw, u = cfg_parts(cfg)
    names = ["r708", "rmask512"]
    if u == 2:
        names.append("r320")
    if nw in (3, 5, 10) or cfg == 208:
        names.append("rwin228")
    if cfg in (102, 104, 208, 1104):
        names.append("r64")
    return names


WAVE_PARAMS = [pytest.param(T, hd, gn, id=f"{NAME[T]}-hd{hd}-{gn}") for T in (F32, F16, BF16) for hd in (16, 32, 64) for gn in WAVE_GEOS]
WIN_PARAMS = [pytest.param(T, hd, gn, id=f"{NAME[T]}-hd{hd}-{gn}") for T in (F16, BF16) for hd in (16, 32) for gn in WIN_GEOS]
RING_PARAMS = [pytest.param(T, hd, cfg, id=f"{NAME[T]}-hd{hd}-{cfg}") for T in (F16, BF16) for hd in (16, 32, 64) for cfg in RING_CFGS if ring_fits(hd, cfg)]
RING_REFUSED = [(T, hd, cfg) for T in (F16, BF16) for hd in (16, 32, 64) for cfg in RING_CFGS if not ring_fits(hd, cfg)]


def pinned_forms(experiments):
    """The module's own case table: every form an element-wise test pins."""
    forms = {f for p in WAVE_PARAMS for f, _ in wave_runs(*p.values)}
    forms |= {f"attn_win_{NAME[p.values[0]]}_hd{p.values[1]}" for p in WIN_PARAMS}
    forms |= {ring_form(*p.values) for p in RING_PARAMS}
    if experiments:
        forms |= {"attn_wtile_f16", "attn_wtile_bf16"}
    return forms


def all_cases():
    """(label, case, family) of every distinct (case, bound) the element-wise tests use (tests/test_attention_bound_host.py)."""
    out = []
    for p in WAVE_PARAMS:
        T, hd, gn = p.values
        out.append((f"wave {NAME[T]} hd{hd} {gn}", (T, hd, gn), "wave"))
    for p in WIN_PARAMS:
        T, hd, gn = p.values
        out.append((f"win {NAME[T]} hd{hd} {gn}", (T, hd, gn), "win"))
    for T in (F16, BF16):
        for hd in (16, 32, 64):
            for gn in RING_GEOS:
                out.append((f"ring {NAME[T]} hd{hd} {gn}", (T, hd, gn), "ring"))
    return out


def case_of(T, hd, gn):
    return attn_case(T, hd, gn, ALL_GEOS[gn])


# ------------------------------------------------------------------------------------------------------------ the element-wise tests
@pytest.mark.gpu
@pytest.mark.parametrize("T,hd,gname", WAVE_PARAMS)
def test_attn_wave_vs_fp64(T, hd, gname, routes, knobs):
    """attn_kernel: 8 and 12 keys (load_v clamps to nkeys - 8, shift4 with a run start of 4), 44 keys, windows, the decoder's 300, holes, the
    >= 512 prefetch branch, 64 queries per wave with idle waves, the short form against ATTN_SHORT=0 - each against float64."""
    case = case_of(T, hd, gname)
    knobs.set("ATTN_WIN", 0)
    routes.lwdetr_attention_tuning(0)
    for form, switches in wave_runs(T, hd, gname):
        for name in ("ATTN_QT", "ATTN_SHORT"):
            if name in switches:
                knobs.set(name, switches[name])
            else:
                _native.tuning_set(name, None)
        check(case, form, f"wave {NAME[T]} hd{hd} {gname}")
    RAN.add(("wave", T, hd, gname))


@pytest.mark.gpu
@pytest.mark.parametrize("T,hd,gname", WIN_PARAMS)
def test_attn_win_vs_fp64(T, hd, gname, routes, knobs):
    """attn_win_kernel (one wave per (sequence, head)): pad rows behind the real tokens, ragged key and query tiles, 8 keys, a last workgroup with
    idle waves; in LWDETR_EXPERIMENTS builds attn_wtile_kernel is pinned too and bit-identical at hd 16."""
    case = case_of(T, hd, gname)
    knobs.set("ATTN_WIN", 1)
    knobs.set("ATTN_WTILE", 0)
    buf = check(case, f"attn_win_{NAME[T]}_hd{hd}", f"win {NAME[T]} hd{hd} {gname}")
    if hd == 16 and _native.lib().lwdetr_has_experiments():
        knobs.set("ATTN_WTILE", 1)
        buf2 = check(case, f"attn_wtile_{NAME[T]}", f"wtile {NAME[T]} {gname}")
        assert torch.equal(bits(buf), bits(buf2)), "attn_wtile_kernel and attn_win_kernel differ"
    RAN.add(("win", T, hd, gname))


@pytest.mark.gpu
@pytest.mark.parametrize("T,hd,cfg", RING_PARAMS)
def test_attn_ring_vs_fp64(T, hd, cfg, routes, knobs):
    """Every launchable (dtype, hd, cfg) of the LDS-ring kernel: a ragged last block with a straddling V^T run on a grid that is no multiple of 8
    workgroups, 32-key groups with every key masked, a last ring step with fewer than U blocks, windows with pad rows, one block."""
    routes.lwdetr_attention_tuning(3)
    routes.lwdetr_attention_tuning_cfg(cfg)
    knobs.set("ATTN_WIN", 0)
    for gn in ring_geos(cfg):
        check(case_of(T, hd, gn), ring_form(T, hd, cfg), f"ring {NAME[T]} hd{hd} {gn}")
    RAN.add(("ring", T, hd, cfg))


@pytest.mark.gpu
def test_attn_ring_hd16_and_hd32_in_one_process(routes, knobs):
    """The hd 16 ring kernels live in a second object: its launches and the main object's land in the same record."""
    routes.lwdetr_attention_tuning(3)
    knobs.set("ATTN_WIN", 0)
    before = _native.attn_path_counts()
    launch(case_of(F16, 16, "r64"), "attn_ring_f16_hd16_q1w4u1")
    launch(case_of(F16, 32, "r64"), "attn_ring_f16_hd32_q1w4u1")
    after = _native.attn_path_counts()
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {"attn_ring_f16_hd16_q1w4u1": 1, "attn_ring_f16_hd32_q1w4u1": 1}


@pytest.mark.gpu
def test_attn_ring_forms_that_do_not_fit_are_refused(routes, knobs):
    """U = 2 at hd 64 and U = 4 everywhere: LWDETR_ERR_UNSUPPORTED, nothing counted, nothing written."""
    from lwdetr_amd import kernels as K
    routes.lwdetr_attention_tuning(3)
    knobs.set("ATTN_WIN", 0)
    assert len(RING_REFUSED) == 2 * (1 + 1 + 6)
    for T, hd, cfg in RING_REFUSED:
        routes.lwdetr_attention_tuning_cfg(cfg)
        g = RING_GEOS["r64"]
        q, k = (torch.zeros(g["B"], g["heads"], g["Tp"], hd, dtype=T, device="cuda") for _ in range(2))
        vt = torch.zeros(g["B"], g["heads"], hd, g["Tp"], dtype=T, device="cuda")
        out = torch.full((g["B"] * g["Tp"], g["heads"] * hd), SENT, dtype=T, device="cuda")
        op = K.AttnOp(q, k, vt, out, B=g["B"], heads=g["heads"], hd=hd, Tp=g["Tp"], ldo=g["heads"] * hd, seqs_per_img=1, seq_tok_stride=g["stride"],
                      keys_per_seq=g["keys"], sub_stride=g["keys"], sub_len=g["keys"], kind=1)
        before = _native.attn_path_counts()
        rc = _native.lib().lwdetr_attention(op._ref, op.dtype, _native.stream_ptr())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED, f"{ring_form(T, hd, cfg)}: rc {rc}"
        assert _native.attn_path_counts() == before and bool((out == SENT).all()), f"{ring_form(T, hd, cfg)}: something was counted or written"


# ------------------------------------------------------------------------------------------------------------ default routing
def _plain(keys, spi=1, sub=None, B=1, heads=12, slack=False):
    g = geo(keys, spi=spi, gap=0, sub=sub, B=B, heads=heads, slack=slack)
    g["Tp"] = spi * keys                                              # the engine's buffers: no gap, nothing behind
    return g


# The descriptor shapes the engine builds (engine.py: windows with vt_slack, global blocks and the decoder without) and the form `launch` of
# attention.hip documents for them, read off the dispatcher; no knob, no override. Rows marked (threshold) are not engine shapes: they sit just
# below a grid-fill threshold of lds_path_applies / of the 64-query form.
DEFAULT_ROUTES = [
    ("window 100 hd16", F16, 16, _plain(100, spi=16, B=2, slack=True), "attn_wave_f16_hd16_qt2_short"),       # ATTN_WIN default: hd 32 only; < 192 keys: no ring
    ("window 100 hd32", BF16, 32, _plain(100, spi=16, B=2, slack=True), "attn_win_bf16_hd32"),
    ("global 1600 hd16 B1", F16, 16, _plain(1600, sub=(100, 100)), "attn_ring_f16_hd16_q1w4u1"),              # 13 x 12 = 156 >= 128 workgroups: B = 1 fills
    ("global 1600 hd16 9 heads (threshold)", F16, 16, _plain(1600, sub=(100, 100), heads=9), "attn_wave_f16_hd16_qt2"),   # 117 < 128
    ("global 1600 hd32 B1", F16, 32, _plain(1600, sub=(100, 100)), "attn_wave_f16_hd32_qt2"),                 # 7 x 12 = 84 < 256
    ("global 1600 hd32 B3 (threshold)", BF16, 32, _plain(1600, sub=(100, 100), B=3), "attn_wave_bf16_hd32_qt2"),          # 252 < 256
    ("global 1600 hd32 B4", BF16, 32, _plain(1600, sub=(100, 100), B=4), "attn_ring_bf16_hd32_q1w8u1"),       # 336 >= 256: the smallest B that fills
    ("global 3648 hd64 B1", F16, 64, _plain(3648, sub=(228, 225)), "attn_wave_f16_hd64_qt2"),                 # 15 x 12 = 180 < 256
    ("global 3648 hd64 B2", F16, 64, _plain(3648, sub=(228, 225), B=2), "attn_ring_f16_hd64_q2w8u1"),         # 360 >= 256; hd 64, >= 512 keys: cfg 208
    ("decoder 300 hd32", F16, 32, _plain(300, B=2, heads=8), "attn_wave_f16_hd32_qt2"),                       # 300 % 8 == 4 without vt_slack: no ring
    ("global 1604 hd32 B4, no slack (threshold)", F16, 32, _plain(1604, B=4), "attn_wave_f16_hd32_qt4"),      # no ring; >= 1024 keys, 336 >= 256: 64 queries per wave
    ("window 100 f32", F32, 16, _plain(100, spi=16, B=1, slack=True), "attn_wave_f32_hd16_qt2"),
    ("global 1600 f32", F32, 32, _plain(1600, sub=(100, 100)), "attn_wave_f32_hd32_qt2"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("label,T,hd,g,form", DEFAULT_ROUTES, ids=[r[0].replace(" ", "_") for r in DEFAULT_ROUTES])
def test_attn_default_routing(label, T, hd, g, form):
    """Record only: with no switch set, the engine's descriptor shapes go to the kernels the dispatcher documents. Outputs are checked finite."""
    from lwdetr_amd import kernels as K
    B, H, Tp = g["B"], g["heads"], g["Tp"]
    gen = torch.Generator().manual_seed(5)
    q, k = ((torch.randn(B, H, Tp, hd, generator=gen) * s).to(T).cuda() for s in (hd ** -0.5 * LOG2E, 1.0))
    vt_store = torch.zeros(B * H * hd * Tp + 8, dtype=T, device="cuda")
    vt = vt_store[:B * H * hd * Tp].view(B, H, hd, Tp)
    vt.copy_(torch.randn(B, H, hd, Tp, generator=gen).to(T))
    out = torch.full((B * Tp, H * hd), math.nan, dtype=T, device="cuda")
    with attn_served_by(form):
        K.AttnOp(q, k, vt, out, B=B, heads=H, hd=hd, Tp=Tp, ldo=H * hd, seqs_per_img=g["spi"], seq_tok_stride=g["stride"], keys_per_seq=g["keys"],
                 sub_stride=g["sub_stride"], sub_len=g["sub_len"], kind=0 if g["spi"] > 1 else 1, vt_slack=g["slack"])()
    assert bool(torch.isfinite(out).all()), f"{label}: non-finite or unwritten output rows"


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_attn_bad_arguments_are_refused():
    """Each LWDETR_ERR_BAD_ARG condition of lwdetr_attention (and an unknown head size / dtype) leaves the record and the output untouched."""
    from lwdetr_amd import kernels as K
    B, H, hd, Tp, T = 2, 2, 16, 48, F16
    q, k = (torch.zeros(B, H, Tp, hd, dtype=T, device="cuda") for _ in range(2))
    vt = torch.zeros(B, H, hd, Tp, dtype=T, device="cuda")
    out = torch.full((B * Tp, H * hd), SENT, dtype=T, device="cuda")
    good = dict(B=B, heads=H, hd=hd, Tp=Tp, ldo=H * hd, seqs_per_img=2, seq_tok_stride=24, keys_per_seq=20, sub_stride=20, sub_len=17, kind=0)
    lib = _native.lib()

    def refused(expect, label, dtype=None, null=None, **over):
        op = K.AttnOp(q, k, vt, out, **{**good, **over})
        if null:
            setattr(op.desc, null, None)
        before = _native.attn_path_counts()
        rc = lib.lwdetr_attention(op._ref, op.dtype if dtype is None else dtype, _native.stream_ptr())
        torch.cuda.synchronize()
        assert rc == expect, f"{label}: rc {rc}, expected {expect}"
        assert _native.attn_path_counts() == before and bool((out == SENT).all()), f"{label}: something was counted or written"

    before = _native.attn_path_counts()
    assert lib.lwdetr_attention(None, _native.dtype_code(T), _native.stream_ptr()) == BAD_ARG and _native.attn_path_counts() == before
    for name in ("Q", "K", "VT", "out"):
        refused(BAD_ARG, f"{name} null", null=name)
    for label, over in (("B 0", dict(B=0)), ("heads 0", dict(heads=0)), ("Tp 0", dict(Tp=0)), ("Tp % 4", dict(Tp=46)), ("seqs_per_img 0", dict(seqs_per_img=0)),
                        ("keys 4", dict(keys_per_seq=4, sub_stride=4, sub_len=4)), ("keys % 4", dict(keys_per_seq=18)), ("sub_stride 0", dict(sub_stride=0)),
                        ("sub_len 0", dict(sub_len=0)), ("sub_len > sub_stride", dict(sub_len=21)), ("sequences past Tp", dict(seq_tok_stride=32)),
                        ("seq_tok_stride % 4", dict(seq_tok_stride=22)), ("ldo % 4", dict(ldo=H * hd + 2)), ("B seqs > 65535", dict(B=32768)),
                        ("heads > 65535", dict(heads=65536))):
        refused(BAD_ARG, label, **over)
    refused(UNSUPPORTED, "hd 48", hd=48)
    refused(UNSUPPORTED, "dtype 3", dtype=3)


# ------------------------------------------------------------------------------------------------------------ the transcendentals, measured
@pytest.mark.gpu
@pytest.mark.parametrize("hd,qt", [(16, 2), (32, 2), (64, 2), (16, 4), (32, 4)])
def test_attn_softmax_weights_measured(hd, qt, routes, knobs):
    """The f32 forms on a V that is 1 at (key c, channel c), c < hd, and 0 elsewhere: output channel c IS the softmax weight of key c. Prints the
    worst relative deviation from the float64 weight (TRANS_MEASURED, module docstring) and holds it against TRANS_F32."""
    from lwdetr_amd import kernels as K
    B, H, n = 1, 2, 200
    gen = torch.Generator().manual_seed(11)
    # multiples of 2^-6: products and their sums are exact in f32, so the scores carry no rounding of their own into the figure
    q = ((torch.randn(B, H, n, hd, generator=gen) * (hd ** -0.5 * LOG2E)).clamp(-1, 1) * 64).round() / 64
    k = (torch.randn(B, H, n, hd, generator=gen).clamp(-2, 2) * 64).round() / 64
    s = q.double() @ k.double().transpose(-1, -2)
    assert float(s.abs().max()) < 12                                  # logits within a few units: the exponent's own roundings stay small
    v = torch.zeros(B, H, n, hd)
    v[:, :, :hd] = torch.eye(hd)
    a = torch.softmax(s * math.log(2.0), -1)[..., :hd]               # (B, H, n, hd): the weights of keys 0 .. hd - 1
    out = torch.full((B * n, H * hd), SENT, dtype=F32, device="cuda")
    knobs.set("ATTN_QT", qt)
    routes.lwdetr_attention_tuning(0)
    form = f"attn_wave_f32_hd{hd}_qt{qt}"
    with attn_served_by(form):
        K.AttnOp(q.cuda(), k.cuda(), v.transpose(2, 3).contiguous().cuda(), out, B=B, heads=H, hd=hd, Tp=n, ldo=H * hd, seqs_per_img=1, seq_tok_stride=n,
                 keys_per_seq=n, sub_stride=n, sub_len=n, kind=1)()
    got = out.cpu().double().reshape(B, n, H, hd).permute(0, 2, 1, 3)
    worst = float(((got - a).abs() / a).max())
    print(f"ATTN_TRANS {form} worst relative deviation of a weight {worst * 2 ** 23:.3f} x 2^-23")
    assert worst <= TRANS_F32, f"{form}: a softmax weight deviates by {worst * 2 ** 23:.3f} x 2^-23, TRANS_F32 is {TRANS_F32 * 2 ** 23:.3f} x 2^-23"


# ------------------------------------------------------------------------------------------------------------ the record, enumerated
def test_attn_case_table_covers_every_name_of_the_rule():
    """The rule of the names (include/lwdetr_hip.h), restated: every name is pinned by an element-wise case of this module or asserted refused."""
    refused = {ring_form(*r) for r in RING_REFUSED}
    pinned = pinned_forms(False)
    assert not (pinned & refused)
    rule = {f"attn_wave_{t}_hd{hd}_qt2" for t in NAME.values() for hd in (16, 32, 64)}
    rule |= {f"attn_wave_{t}_hd{hd}_qt4" for t in NAME.values() for hd in (16, 32)}
    rule |= {f"attn_wave_{t}_hd{hd}_qt2_short" for t in ("f16", "bf16") for hd in (16, 32, 64)}
    rule |= {f"attn_win_{t}_hd{hd}" for t in ("f16", "bf16") for hd in (16, 32)}
    rule |= {ring_form(T, hd, cfg) for T in (F16, BF16) for hd in (16, 32, 64) for cfg in RING_CFGS}
    assert pinned | refused == rule, sorted((pinned | refused) ^ rule)


@pytest.mark.gpu
def test_attn_every_name_is_pinned_or_refused():
    """Every name of lwdetr_attn_path_name is pinned by at least one element-wise case of this module's table or asserted to be refused; no
    refused form has ever been launched, and when all element-wise cases ran before this test (it is the module's last) every pinned one has."""
    counts = _native.attn_path_counts()
    experiments = bool(_native.lib().lwdetr_has_experiments())
    refused = {ring_form(*r) for r in RING_REFUSED}
    pinned = pinned_forms(experiments)
    assert set(counts) == pinned | refused, sorted(set(counts) ^ (pinned | refused))
    assert all(counts[f] == 0 for f in refused), {f: counts[f] for f in refused if counts[f]}
    for form in sorted(WORST):
        print(f"ATTN_WORST_FORM {form} {WORST[form]:.3f}")
    assert set(WORST) <= pinned and all(counts[f] > 0 for f in WORST)
    if len(RAN) == len(WAVE_PARAMS) + len(WIN_PARAMS) + len(RING_PARAMS):      # not a selection of the module
        assert pinned == set(WORST), sorted(pinned - set(WORST))
