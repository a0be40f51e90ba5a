"""The element bounds of tests/test_gpu_vitblock.py, met on the CPU by a correct implementation other than the code under test: an independent
FLOAT32 evaluation of the block / QKV / stem arithmetic (torch on the CPU: the same rounding points, torch's own summation order, the f32 expressions of
the kernel for LayerNorm and GELU) against the float64 reference of that module, element by element - inside the worst-case bound everywhere, and
outside the tight (statistical) bound on no more than the stated share. Also: the reference builder against the plain dense formulation of the
block from the f32 master weights (no folding, erf-free: the kernel's GELU expression), against the lane-level emulation of the packed stream
(tests/vitblock_sim.py), and the host formula of launch_vb's grid."""
import numpy as np
import pytest
import torch

from tests import test_gpu_vitblock as V
from tests import vitblock_sim as sim
from tests.test_gpu_rowops import F16, BF16


def _f32(D):
    return {k: v.float() for k, v in D.items()}


def _gelu_f32(h, T, gelu):
    if gelu == "packed_f16":
        return torch.from_numpy(sim.gelu_vb16_packed(h.to(torch.float16).double().numpy())).float()
    c0, c1 = torch.tensor(-2.3087653, dtype=torch.float32), torch.tensor(-0.10012561, dtype=torch.float32)
    return (h * (1.0 / (1.0 + torch.exp2(h * (h * h * c1 + c0))))).to(T).float()


def _ln_f32(x, eps, T):
    mean = x.sum(1, keepdim=True) * np.float32(1.0 / x.shape[1])
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) * np.float32(1.0 / x.shape[1]) + np.float32(eps))
    return (x * rstd + (-mean * rstd)).to(T).float()


def _qkv_f32(rows, D, T, eps, chained, qscale_factor=1.0):
    C = rows.shape[1]
    z = _ln_f32(rows, eps, T)
    qs = torch.cat([torch.full((C,), float(np.float32(np.float32(V.QSCALE) * np.float32(qscale_factor)))), torch.ones(2 * C)])
    y = (z @ D["wq"].t() + D["bq"]) * qs
    y = y.to(T).double()
    return dict(q=y[:, :C], k=y[:, C:2 * C], v=y[:, 2 * C:])


def block_f32(x, att, D, T, gelu, qscale_factor=1.0):
    D = _f32(D)
    x, att = x.float(), att.float()
    x1 = (D["g1"] * (x * D["rg1"] + D["bp"] + att @ D["wp"].t())).to(T).float()
    z = _ln_f32(x1, V.EPS, T)
    h = _gelu_f32(z @ D["w1"].t() + D["b1"], T, gelu)
    out = (D["g2"] * (x1 * D["rg2"] + D["b2"] + h @ D["w2"].t())).to(T).float()
    res = _qkv_f32(out, D, T, V.EPS_NEXT, True, qscale_factor)
    res["x"] = out.double()
    return res


@pytest.mark.parametrize("what", ["b2", "bp", "bq", "swap wp", "swap w2", "qscale", "att"])
def test_sensitivity_cases_fail_exactly_on_the_f32_evaluation(what):
    """The sensitivity cases of the GPU module on the CPU: the f32 evaluation with ONE altered operand fails the comparison with the reference of
    the original operands on the elements that depend on it, and on no other."""
    T = F16
    case = V.block_case(V.SENS_C, V.SENS_M, T, "f32")
    D, att = dict(case["D"]), case["att"]
    scale = 1.0
    if what in ("b2", "bp", "bq"):
        idx, val, alt, dep = V.sens_bias(case, T, what)
        D[what] = D[what].clone()
        D[what][idx - V._vec_section(V.SENS_C, what)] = val
    elif what.startswith("swap"):
        (a, b), alt, dep = V.sens_swap(case, T, what[5:])
        C = V.SENS_C
        if what == "swap wp":
            w = D["wp"].clone(); w[0:32, 0:16], w[0:32, 16:32] = D["wp"][0:32, 16:32], D["wp"][0:32, 0:16]; D["wp"] = w
        else:
            w = D["w2"].clone(); w[0:32, :16], w[32:64, :16] = D["w2"][32:64, :16], D["w2"][0:32, :16]; D["w2"] = w
    elif what == "qscale":
        qs2, alt, dep = V.sens_qscale(case, T)
        scale = float(np.float32(qs2)) / float(np.float32(V.QSCALE))
    else:
        att, alt, dep = V.sens_att(case, T)
    got = block_f32(case["x"], att, D, T, "f32", qscale_factor=scale)
    V.fails_exactly(got, case, alt, T, f"host sensitivity {what}", dep)


def _check_all(got, case, T, label, names="xqkv"):
    for n in names:
        V.check2(got[n], case["tight"][n][0], case["tight"][n][1], case["worst"][n][1], T, f"host {label} {n}")


@pytest.mark.parametrize("T", [F16, BF16], ids=V._name)
@pytest.mark.parametrize("C,M", [(192, 40), (192, 136), (384, 264)])
def test_block_bound_is_met_by_an_f32_evaluation(C, M, T):
    for gelu in (("f32", "packed_f16") if T == F16 else ("f32",)):
        case = V.block_case(C, M, T, gelu)
        _check_all(block_f32(case["x"], case["att"], case["D"], T, gelu), case, T, f"block {V._name(T)} C{C} M{M} {gelu}")
        fl = case["tight"]["flags"]
        print(f"flagged (within their f32 error of a tie): x1 {fl['x1']:.3f}, z {fl['z']:.3f}, h {fl['h']:.3f}")


@pytest.mark.parametrize("T", [F16, BF16], ids=V._name)
def test_qkv_and_stem_bounds_are_met_by_an_f32_evaluation(T):
    C, M = 192, 40
    case = V.qkv_case(C, M, T)
    _check_all(_qkv_f32(case["x"].float(), _f32(case["D"]), T, V.EPS_NEXT, False), case, T, f"qkv {V._name(T)}", "qkv")
    geom = (3, 12, 8, 7)
    case = V.stem_case(C, geom, T)
    D = _f32(case["D"])
    B, Hp, Wp, Twp = geom
    b, y, x, valid = V.stem_tokens(B, Hp, Wp, Twp)
    patches = case["img"].float().reshape(B, 3, Hp, 16, Wp, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, Hp, Wp, 768)
    P = torch.zeros(case["M"], 768)
    P[valid] = patches[b[valid], y[valid], x[valid]]
    x0 = ((case["pos"].float().repeat(B, 1) + D["bpe"]) + P @ D["wpe"].t()).to(T).float()
    got = _qkv_f32(x0, D, T, V.EPS_NEXT, False)
    got["x"] = x0.double()
    _check_all(got, case, T, f"stem {V._name(T)}")
    assert bool((~valid).any())                                 # this geometry has pad rows, and they are compared like every other row


def test_bound_is_about_an_output_ulp():
    """What the bound buys: the median tight bound of the new rows is within 1.25 half-ulps of the value's own half ulp (f16, f32-arithmetic GELU),
    where the norm-wise 6e-3 max|ref| of test_vit_block allows 0.064 on every element."""
    case = V.block_case(192, 136, F16, "f32")
    y, e = case["tight"]["x"]
    b = V.bound_of(y, e, F16)
    r = (b / V.half_ulp(y, F16))
    print(f"tight bound / half ulp: median {float(r.median()):.2f}, 99th percentile {float(r.flatten().kthvalue(int(0.99 * r.numel())).values):.2f}")
    assert float(r.median()) < 1.25
    assert float(b.median()) < 0.064 / 50


def test_reference_against_the_dense_formulation():
    """The reference (folded 16-bit weights, rounding points) against the unfolded float64 formulation from the f32 masters: they differ by what the
    16-bit roundings cost, a few 1e-3 of each row's scale - a wrong fold, bias, section offset or transposition would cost far more."""
    for C in (192, 384):
        T, M = F16, 40
        case = V.block_case(C, M, T, "f32")
        W = {k: v.double() for k, v in case["W"].items()}
        x, att = case["x"].double(), case["att"].double()
        ln = lambda t, w, b, eps: (t - t.mean(1, keepdim=True)) / torch.sqrt(t.var(1, unbiased=False, keepdim=True) + eps) * w + b
        x1 = x + W["g1"] * (att @ W["wp"].t() + W["bp"])
        h = torch.from_numpy(sim.gelu_vb16((ln(x1, W["ln2_w"], W["ln2_b"], V.EPS) @ W["w1"].t() + W["b1"]).numpy()))
        out = x1 + W["g2"] * (h @ W["w2"].t() + W["b2"])
        y = ln(out, W["ln1_w"], W["ln1_b"], V.EPS_NEXT) @ W["wqkv"].t() + torch.cat([W["qb"], torch.zeros(C, dtype=torch.float64), W["vb"]])
        ref = case["tight"]
        dense = dict(x=out, q=y[:, :C] * V.QSCALE, k=y[:, C:2 * C], v=y[:, 2 * C:])
        for n in "xqkv":
            rel = (ref[n][0] - dense[n]).norm(dim=1) / dense[n].norm(dim=1)
            assert float(rel.max()) < 4e-3, (C, n, float(rel.max()))


def test_reference_weights_are_what_the_packed_stream_holds(monkeypatch):
    """One wave of the lane-level emulation on the PACKED stream (no activation rounding) against the same arithmetic on the reference's dense
    weights: the reference builder and kernels.pack_vit_block agree on every weight, permutation and vector section."""
    C, M, T, nvalid, heads, Tp = 192, 40, F16, 24, 6, 8
    case = V.block_case(C, M, T, "f32")
    D = case["D"]
    stream, vec = V.packed_block(case["W"], T, True)
    monkeypatch.setattr(sim, "gelu_fast16", sim.gelu_vb16)
    x, att = case["x"].double().numpy(), case["att"].double().numpy()
    out, writes = sim.simulate_wave(stream.double().numpy(), vec.double().numpy(), x, att, 8, nvalid, C, 1, V.EPS, V.EPS_NEXT,
                                    qkv=dict(heads=heads, hd=C // heads, Tp=Tp, qscale=V.QSCALE))
    xs, as_ = torch.from_numpy(x[8:8 + nvalid]), torch.from_numpy(att[8:8 + nvalid])
    ln = lambda t, eps: (t - t.mean(1, keepdim=True)) / torch.sqrt(t.var(1, unbiased=False, keepdim=True) + eps)
    x1 = D["g1"] * (xs * D["rg1"] + D["bp"] + as_ @ D["wp"].t())
    h = torch.from_numpy(sim.gelu_vb16((ln(x1, V.EPS) @ D["w1"].t() + D["b1"]).numpy()))
    o = D["g2"] * (x1 * D["rg2"] + D["b2"] + h @ D["w2"].t())
    assert float((torch.from_numpy(out) - o).abs().max()) < 1e-9 * float(o.abs().max())
    y = ln(o, V.EPS_NEXT) @ D["wq"].t() + D["bq"]
    y[:, :C] *= V.QSCALE
    nb = M // Tp
    full = torch.zeros(M, 3 * C, dtype=torch.float64)
    full[8:8 + nvalid] = y
    for name, sl, tr in (("q", slice(0, C), False), ("k", slice(C, 2 * C), False), ("v", slice(2 * C, 3 * C), True)):
        flat = V.heads_layout(full[:, sl], nb, Tp, heads, C // heads, tr)
        idx = [i for (n, i) in writes if n == name]
        assert len(idx) == nvalid * C
        got = torch.tensor([writes[(name, i)] for i in idx])
        assert float((got - flat[idx]).abs().max()) < 1e-9 * float(flat.abs().max()), name


def test_launch_vb_grid_never_needs_the_bump():
    """launch_vb: with grid = need = ceil(M / (128 NH)) no wave gets more than 32 NH tokens (the `while (...) ++grid` loop is never entered),
    for every M % 8 == 0 up to 4096 and both NH; the dealing itself (floor) gives every wave at most ceil(U / waves) units."""
    for nh in (1, 2):
        for M in range(8, 4097, 8):
            U, need = M // 8, -(-M // (128 * nh))
            assert -(-U // (need * 4)) * 8 <= 32 * nh, (nh, M)
            nwv = need * 4
            assert max((w + 1) * U // nwv - w * U // nwv for w in range(nwv)) * 8 <= 32 * nh
