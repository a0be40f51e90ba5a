"""The element bounds of tests/test_gpu_mlp_fp64.py, met on the CPU by a correct implementation other than the code under test: an independent
FLOAT32 evaluation of the mlp.hip arithmetic in numpy (the same rounding points; the k-chunks of every product summed in REVERSE order, so not the
reference's summation order; the f32 expressions of common.h for LayerNorm, gelu_fast16 and fast_erf) against the float64 reference of that module,
element by element - inside the worst-case bound everywhere and outside the tight (statistical) bound on no more than the stated share, with the
committed seeds. Each of a list of planted mistakes in that evaluation leaves the bound. Also: the GELU models against one another, and Python models of
launch_mlp_p's tile dealing and launch_ffn's split over every row count up to 70000."""
import numpy as np
import pytest
import torch

from tests import test_gpu_mlp_fp64 as G
from tests import vitblock_sim as sim
from tests.test_gpu_rowops import F16, BF16, F32

f32 = np.float32


def _r(v, T):
    """f32 array -> nearest T, as f32."""
    return v if T == F32 else torch.from_numpy(np.ascontiguousarray(v)).to(T).float().numpy()


def _mm(a, w, start=None):
    """a (M, K) @ w (N, K)^T in f32, 32 columns of K at a time from the LAST chunk to the first, on top of `start`."""
    acc = np.zeros((a.shape[0], w.shape[0]), f32) if start is None else np.broadcast_to(start.astype(f32), (a.shape[0], w.shape[0])).copy()
    for k in reversed(range(0, a.shape[1], 32)):
        acc = acc + a[:, k:k + 32] @ w[:, k:k + 32].T
    return acc


def _ln(x, eps, T, stats_of=None):
    s = x if stats_of is None else stats_of
    C = x.shape[1]
    mean = s.sum(1, keepdims=True, dtype=f32) * f32(1.0 / C)
    d = s - mean
    rstd = f32(1.0) / np.sqrt((d * d).sum(1, keepdims=True, dtype=f32) * f32(1.0 / C) + f32(eps))
    return _r((x - mean) * rstd, T)


def _gelu16(x):
    x2 = np.minimum(x * x, f32(36.0))
    p = (x2 * f32(0.0010142630555) + f32(-0.1067757240036)) * x2 + f32(-2.3011213394584)
    return x / (f32(1.0) + np.exp2(x * p))


def _gelu_erf(x):
    """common.h:gelu_erf / fast_erf in f32."""
    v = x * f32(0.70710678118654752440)
    ax = np.abs(v)
    t = f32(1.0) / (f32(1.0) + f32(0.3275911) * ax)
    poly = t * (f32(0.254829592) + t * (f32(-0.284496736) + t * (f32(1.421413741) + t * (f32(-1.453152027) + t * f32(1.061405429)))))
    e = f32(1.0) - poly * np.exp(-ax * ax)
    return f32(0.5) * x * (f32(1.0) + np.where(v < 0, -e, e))


def mlp_f32(case, T, proj, qkv, wrong=None):
    """The arithmetic of mlp_kernel / mlp_small_kernel / vit_block_few384_kernel in f32. wrong: one planted mistake."""
    D = {k: v.numpy().astype(f32) for k, v in case["D"].items()}
    x, att = case["x"].float().numpy(), case["att"].float().numpy()
    C = x.shape[1]
    if wrong in ("b2", "bp", "b1"):
        ch = {"b2": int(np.abs(D["g2"] * D["b2"]).argmax()), "bp": int(np.abs(D["g1"] * D["bp"]).argmax()), "b1": int(np.abs(D["b1"]).argmax())}[wrong]
        D[wrong] = D[wrong].copy()
        D[wrong][ch] = 0
    if wrong == "kslot":
        D["w2"] = D["w2"].copy()
        D["w2"][:, [8, 9]] = D["w2"][:, [9, 8]]
    x1u = x + D["g1"] * (_mm(att, D["wp"]) + D["bp"]) if proj else x
    x1 = x1u if wrong == "x1 unrounded" else _r(x1u, T)
    z = _ln(x1, G.EPS, T, stats_of=x1u if wrong == "stats unrounded" else None)
    hpre = _mm(z, D["w1"], D["b1"])
    h = _r(_gelu_erf(hpre) if T == F32 else _gelu16(hpre), T)
    outu = x1 + D["g2"] * (_mm(h, D["w2"]) + D["b2"])
    out = _r(outu, T)
    res = {"x": torch.from_numpy(out).double()}
    so = outu if wrong == "stats unrounded" else out                  # the statistics output: mean', rstd' (eps_next) of the new rows
    mean = so.sum(1, dtype=f32) * f32(1.0 / C)
    d = so - mean[:, None]
    res["stats"] = torch.from_numpy(np.stack([mean, f32(1.0) / np.sqrt((d * d).sum(1, dtype=f32) * f32(1.0 / C) + f32(G.EPS_NEXT))], 1))
    if qkv:
        z2 = _ln(out, G.EPS if wrong == "eps_next" else G.EPS_NEXT, T, stats_of=outu if wrong == "stats unrounded" else None)
        y = _mm(z2, D["wq"], D["bq"])
        qs = f32(G.QSCALE)
        res.update(q=torch.from_numpy(_r(y[:, :C] * qs, T)).double(), k=torch.from_numpy(_r(y[:, C:2 * C] * (qs if wrong == "qscale on k" else f32(1)), T)).double(),
                   v=torch.from_numpy(_r(y[:, 2 * C:], T)).double())
    return res


def ffn_f32(case, T, S, wrong=None):
    D = {k: v.numpy().astype(f32) for k, v in case["w"]["D"].items()}
    x = case["x"].float().numpy()
    h = _r(np.maximum(_mm(x, D["w1"], D["b1"]), f32(0)), T)
    n = D["w1"].shape[0] // S
    out = []
    for s in range(S):
        t = (s + 1) % S if wrong == "neighbour" else s
        out.append(_mm(h[:, t * n:t * n + n], D["w2"][:, t * n:t * n + n]))
    return torch.from_numpy(np.concatenate(out)).double()


def _check_all(got, case, T, label):
    for n in got:
        if n != "stats":
            G.check("host", got[n], case["tight"][n], case["worst"][n], T, f"host {label} {n}")
    G.check_stats(got["stats"], got["x"].to(T), f"host {label}")


CASES = [(192, 4, F16), (192, 36, F16), (192, 40, F16), (192, 40, BF16), (192, 40, F32), (192, 24, BF16), (384, 20, F16), (384, 40, BF16), (192, 48, F32)]


@pytest.mark.parametrize("C,M,T", CASES, ids=lambda v: str(v).split(".")[-1])
def test_mlp_bounds_are_met_by_an_f32_evaluation(C, M, T):
    """Both bounds - the tight one within its 1e-3 share - on the GPU module's own small cases (same seeds, same operands), with and without the
    projection and the chained QKV."""
    for proj, qkv in ((True, True), (True, False), (False, False)):
        case = G.mlp_case(C, M, T, proj, qkv)
        _check_all(mlp_f32(case, T, proj, qkv), case, T, f"{G.NAME[T]} C{C} M{M} proj{int(proj)} qkv{int(qkv)}")


@pytest.mark.parametrize("T", [F16, BF16], ids=lambda v: str(v).split(".")[-1])
@pytest.mark.parametrize("C,hid,M,S", [(256, 64, 33, 1), (256, 1024, 40, 4), (256, 2048, 300, 16), (384, 2048, 17, 2)])
def test_ffn_bounds_are_met_by_an_f32_evaluation(C, hid, M, S, T):
    case = G.ffn_case(C, hid, M, T, S)
    G.check_ffn("host", ffn_f32(case, T, S), case, f"host ffn {G.NAME[T]} C{C} hid{hid} M{M} S{S}")


def _small_rows_case(T):
    """Rows whose variance is of the order of eps_next: LayerScale of 1e-3 and inputs of 3e-3, so that a wrong eps moves the chained LayerNorm."""
    def build():
        C, M = 192, 40
        W = dict(G.make_weights(C, 0))
        W["g1"], W["g2"] = W["g1"] * 1e-3, W["g2"] * 1e-3
        x = G.make_rows(M, C, T, 0, scale=3e-3, shift=0.0)
        att = G.make_rows(M, C, T, 7, scale=1.0, shift=0.0)
        D = G.dense_weights(W, T)
        return dict(W=W, x=x, att=att, D=D, tight=G.mlp_reference(x, att, D, T, "tight", True, True), worst=G.mlp_reference(x, att, D, T, "worst", True, True))
    return G.cached(("host small rows", T), build)


@pytest.mark.parametrize("wrong", ["b2", "bp", "b1", "x1 unrounded", "stats unrounded", "kslot", "eps_next", "qscale on k"])
def test_planted_mistakes_leave_the_bound(wrong):
    """One mistake in the f32 evaluation - a bias entry never added, x1 kept unrounded, the statistics (of both LayerNorms and the statistics output, which is where it shows) taken of the unrounded rows, two hidden units of W2
    exchanged, eps instead of eps_next, qscale on k as well - and the comparison with the reference fails; the unaltered evaluation passes it."""
    T = F16
    case = _small_rows_case(T) if wrong == "eps_next" else G.mlp_case(192, 40, T, True, True)
    _check_all(mlp_f32(case, T, True, True), case, T, f"unaltered ({wrong})")
    with pytest.raises(AssertionError):
        _check_all(mlp_f32(case, T, True, True, wrong=wrong), case, T, f"planted {wrong}")


def test_planted_neighbouring_slab_leaves_the_bound():
    T, (C, hid, M, S) = F16, (256, 1024, 40, 4)
    case = G.ffn_case(C, hid, M, T, S)
    with pytest.raises(AssertionError):
        G.check_ffn("host", ffn_f32(case, T, S, wrong="neighbour"), case, "planted neighbouring slab")


def test_gelu_models():
    """gelu16 of the GPU module is vitblock_sim.gelu_fast16 (= common.h:gelu_fast16) up to the f32 rounding of the coefficients; it is NOT the two-term
    gelu_vb16 of vitblock.hip; both 16-bit forms and fast_erf stay within their documented distance of the erf GELU."""
    x = torch.linspace(-9, 9, 36001, dtype=torch.float64)
    a, _ = G.gelu16(x)
    b = torch.from_numpy(sim.gelu_fast16(x.numpy()))
    assert float((a - b).abs().max()) < 2e-6
    assert float((a - torch.from_numpy(sim.gelu_vb16(x.numpy()))).abs().max()) > 1e-4
    erf = G.gelu_erf64(x)
    assert float((a - erf).abs().max()) < 4e-5
    g32 = torch.from_numpy(_gelu_erf(x.numpy().astype(f32)).astype(np.float64))
    x32 = torch.from_numpy(x.numpy().astype(f32).astype(np.float64))
    e32 = G.gelu_erf64(x32)
    assert bool(((g32 - e32).abs() <= G.gelu_erf_bound(x32, e32) + G.half_ulp(e32, F32)).all())


# ------------------------------------------------------------------------------------------------------------ host formulas of the launches
def deal(ntiles, n_cu, tpw):
    """launch_mlp_p: workgroups of a launch; mlp_kernel: (tb, tr)."""
    blocks = min(ntiles, n_cu)
    if ntiles > blocks * tpw:
        blocks = -(-ntiles // tpw)
    return blocks, ntiles // blocks, ntiles % blocks


@pytest.mark.parametrize("n_cu", [64, 256, 304])
@pytest.mark.parametrize("tt,tpw", [(2, 7), (2, 8), (1, 8)])
def test_tile_dealing_over_every_row_count(n_cu, tt, tpw):
    """For every M up to 70000: workgroup b owns tiles [tile0, tile0 + my) with my = tb + (b < tr) <= TPW, wave w < my owns tile0 + w; the runs are
    disjoint, in order and cover [0, ntiles) - every tile has exactly one (workgroup, wave)."""
    M = np.arange(1, 70001, dtype=np.int64)
    ntiles = -(-M // (16 * tt))
    blocks = np.minimum(ntiles, n_cu)
    more = ntiles > blocks * tpw
    blocks = np.where(more, -(-ntiles // tpw), blocks)
    tb, tr = ntiles // blocks, ntiles % blocks
    assert bool((blocks >= 1).all()) and bool((tb >= 1).all())
    assert bool((tb + (tr > 0) <= tpw).all()), "a workgroup is dealt more tiles than it can take"
    assert bool((more == (ntiles > n_cu * tpw)).all()) and (int(more.sum()) > 0) == (70000 > 16 * tt * n_cu * tpw)      # 304 CUs x 8 tiles x 32 rows hold them all
    for lo in range(0, len(M), 2000):
        nt, bl, b_, r_ = (a[lo:lo + 2000, None] for a in (ntiles, blocks, tb, tr))
        b = np.arange(int(bl.max()))[None, :]
        live = b < bl
        my = b_ + (b < r_)
        tile0 = b * b_ + np.minimum(b, r_)
        nxt = (b + 1) * b_ + np.minimum(b + 1, r_)
        assert bool(((tile0 + my == nxt) | ~live).all()) and bool((tile0[:, 0] == 0).all())
        assert bool((np.where(b == bl - 1, tile0 + my, nt) == nt).all())
        assert bool(((my >= 1) & (my <= tpw) | ~live).all())
    for m in (1, 16 * tt, 16 * tt + 1, 16 * tt * (n_cu + 1) + 4, 16 * tt * n_cu * tpw, 16 * tt * (n_cu * tpw + 1)):      # the scalar form agrees
        i = min(m, len(M)) - 1
        assert deal(int(ntiles[i]), n_cu, tpw) == (int(blocks[i]), int(tb[i]), int(tr[i]))
    m = 16 * tt * (n_cu + 1) + 4                                          # case (d) of the GPU module
    assert deal(-(-m // (16 * tt)), n_cu, tpw)[1:] == (1, 2)
    m = 16 * tt * (n_cu * tpw + 1)                                        # case (e): the extra-rounds branch
    assert deal(m // (16 * tt), n_cu, tpw)[0] == n_cu + 1


@pytest.mark.parametrize("n_cu", [64, 256, 304])
def test_ffn_split_model_over_every_row_count(n_cu):
    """launch_ffn for every tile count that M <= 70000 gives: the slices cover the hidden chunks, a slice's bias fits the 4 C floats of LDS, no
    workgroup is dealt more than its eight waves can take, and LWDETR_FFN_SPLITS caps only the optional doubling."""
    for C in (256, 384):
        for hid in (64, 1024, 2048):
            nch = hid // 32
            for s_max in (1, 4, 16):
                for ntiles in range(1, -(-70000 // (16 * G.ffn_tt(C))) + 1):
                    M = ntiles * 16 * G.ffn_tt(C)
                    S, blocks = G.ffn_splits_model(M, C, hid, n_cu, s_max)
                    assert S >= 1 and nch % S == 0 and (nch // S) * 32 <= 4 * C
                    assert S <= max(s_max, 2 if hid == 2048 else 1)
                    assert blocks * 8 >= ntiles and blocks <= ntiles
                    tb, tr = ntiles // blocks, ntiles % blocks
                    assert tb + (tr > 0) <= 8
    assert G.ffn_splits_model(300, 256, 2112, n_cu)[0] == G.UNSUPPORTED
    assert G.ffn_splits_model(300, 256, 2048, n_cu, 1)[0] == 2              # the forced first split
