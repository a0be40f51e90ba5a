"""CPU-only checks of the bound of tests/test_gpu_msda_fp64.py, on exactly that module's cases (its case builders are imported; no GPU is touched):
  * not too tight: an independent float32 evaluation - levels, samples and corners summed in another order, the corner weights formed in another
    order, the location expression re-associated, np.exp and a division for the softmax, the result rounded to the storage type - stays inside
    the bound on every element of every case;
  * not too loose: each of twelve planted mistakes in the float64 reference leaves the bound on at least one element of at least one case; the
    test prints which."""
import numpy as np
import pytest

from tests import test_gpu_msda_fp64 as G
from tests.test_gpu_msda_fp64 import F32, F64, wide, store


def _ft(T):
    return np.float64 if T == F64 else np.float32


def sample_lowp(value, levels, loc, a, ft):
    """sum_{l, p} a bilinear(value) in `ft` arithmetic: levels last to first, points last to first, corners 4 ... 1, weights as (a lh) lw."""
    B, S, M, D = value.shape
    Q = loc.shape[1]
    _, lsi, _ = G.level_table(levels)
    bI, mI = np.arange(B).reshape(B, 1, 1, 1), np.arange(M).reshape(1, 1, M, 1)
    acc = np.zeros((B, Q, M, D), dtype=ft)
    one, half = ft(1), ft(0.5)
    for l in reversed(range(len(levels))):
        H, W = levels[l]
        with np.errstate(invalid="ignore", over="ignore"):
            h_im = (loc[:, :, :, l, :, 1] * ft(H) - half).astype(ft)
            w_im = (loc[:, :, :, l, :, 0] * ft(W) - half).astype(ft)
            inside = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
        hs, ws = np.where(inside, h_im, ft(0)), np.where(inside, w_im, ft(0))
        hl, wl = np.floor(hs), np.floor(ws)
        lh, lw = hs - hl, ws - wl
        hh, hw = one - lh, one - lw
        hl, wl = hl.astype(np.int64), wl.astype(np.int64)
        al = np.where(inside, a[:, :, :, l, :], ft(0))
        for p in reversed(range(loc.shape[4])):
            for (dh, dw), (wy, wx) in reversed(list(zip(((0, 0), (0, 1), (1, 0), (1, 1)), ((hh, hw), (hh, lw), (lh, hw), (lh, lw))))):
                hi, wi = hl[..., p] + dh, wl[..., p] + dw
                valid = inside[..., p] & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
                i = int(lsi[l]) + np.clip(hi, 0, H - 1) * W + np.clip(wi, 0, W - 1)
                v = value[bI[..., 0], i, mI[..., 0]]
                wgt = np.where(valid, (al[..., p] * wy[..., p]) * wx[..., p], ft(0)).astype(ft)
                acc = (acc + wgt[..., None] * v).astype(ft)
    return acc.reshape(B, Q, M * D)


def forward_lowp(kind, case):
    T = case["T"]
    ft = _ft(T)
    value = wide(case["value"]).astype(ft)
    if kind == "fwd":
        return sample_lowp(value, case["levels"], wide(case["loc"]).astype(ft), wide(case["aw"]).astype(ft), ft)
    B, Q, M, L, P = (case[k] for k in "BQMLP")
    mlp = M * L * P
    oa = wide(case["oa"]).astype(ft).reshape(B, Q, -1)
    off = oa[:, :, :2 * mlp].reshape(B, Q, M, L, P, 2)
    lg = oa[:, :, case["logit_col"]:case["logit_col"] + mlp].reshape(B, Q, M, L * P)
    e = np.exp((lg - lg.max(-1, keepdims=True)).astype(ft)).astype(ft)
    a = (e / e.sum(-1, keepdims=True, dtype=ft)).astype(ft).reshape(B, Q, M, L, P)
    ref, vr = case["ref"].astype(ft), case["vr"].astype(ft)
    loc = np.zeros((B, Q, M, L, P, 2), dtype=ft)
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            for k in (0, 1):
                c = (ref[:, :, k] * vr[:, None, l, k])[:, :, None, None]
                bw = (ref[:, :, 2 + k] * vr[:, None, l, k] * ft(0.5 / P))[:, :, None, None]       # (re-associated: the box scaled first)
                loc[:, :, :, l, :, k] = (off[:, :, :, l, :, k] * bw + c).astype(ft)
    return sample_lowp(value, case["levels"], loc, a, ft)


FORWARD = list(G.all_forward_cases())


@pytest.mark.parametrize("label,kind,case,form", FORWARD, ids=[f[0].replace(" ", "_") for f in FORWARD])
def test_independent_f32_evaluation_is_inside_the_bound(label, kind, case, form):
    y, bnd = G.fwd_reference(case, form) if kind == "fwd" else G.fused_reference(case)
    got = wide(store(forward_lowp(kind, case).astype(np.float64), case["T"]))
    err = np.abs(got - y)
    ratio = err / np.maximum(bnd, 1e-300)
    assert bool((err <= bnd).all()), f"{label}: {int((~(err <= bnd)).sum())} elements outside, worst err/bound {float(ratio.max()):.3f}"
    assert float(ratio.max()) > 1e-3 or case["T"] == F64, f"{label}: the bound is orders of magnitude above an f32 evaluation's error"


def backward_lowp(case):
    """The three gradients in the case's arithmetic type, channels summed last to first, the products associated differently."""
    T, B, Q, M, D, L, P, S = (case[k] for k in ("T", "B", "Q", "M", "D", "L", "P", "S"))
    ft = _ft(T)
    value, loc, aw = (wide(case[k]).astype(ft) for k in ("value", "loc", "aw"))
    tg = wide(case["go"]).astype(ft).reshape(B, Q, M, 1, D)
    gv = np.zeros((B, S, M, D), dtype=ft)
    gl, ga = np.zeros((B, Q, M, L, P, 2), dtype=ft), np.zeros((B, Q, M, L, P), dtype=ft)
    bI = np.broadcast_to(np.arange(B).reshape(B, 1, 1, 1), (B, Q, M, P))
    mI = np.broadcast_to(np.arange(M).reshape(1, 1, M, 1), (B, Q, M, P))
    _, lsi, _ = G.level_table(case["levels"])
    for l, (H, W) in enumerate(case["levels"]):          # (its own geometry, in `ft`: nothing of the reference's sample_parts)
        h_im, w_im = (loc[:, :, :, l, :, 1] * ft(H) - ft(0.5)).astype(ft), (loc[:, :, :, l, :, 0] * ft(W) - ft(0.5)).astype(ft)
        ins = ~((h_im <= -1) | (w_im <= -1) | (h_im >= H) | (w_im >= W))
        hs, ws = np.where(ins, h_im, ft(0)), np.where(ins, w_im, ft(0))
        top, left = np.floor(hs).astype(np.int64), np.floor(ws).astype(np.int64)
        lh, lw = (hs - top.astype(ft)).astype(ft)[..., None], (ws - left.astype(ft)).astype(ft)[..., None]
        hh, hw = ft(1) - lh, ft(1) - lw
        idx, oks, vs = [], [], []
        for r, c in ((top, left), (top, left + 1), (top + 1, left), (top + 1, left + 1)):
            ok = ins & (r >= 0) & (r < H) & (c >= 0) & (c < W)
            i = int(lsi[l]) + np.where(ok, r * W + c, 0)
            idx.append(i)
            oks.append(ok)
            vs.append(np.where(ok[..., None], value[bI, i, mI], ft(0)))
        v1, v2, v3, v4 = vs
        a = aw[:, :, :, l, :, None]
        for (wy, wx), i, ok in reversed(list(zip(((hh, hw), (hh, lw), (lh, hw), (lh, lw)), idx, oks))):
            np.add.at(gv, (bI, i, mI), np.where(ok[..., None], ((wy * a) * tg) * wx, ft(0)).astype(ft))
        val = ((lh * lw) * v4 + (lh * hw) * v3 + (hh * lw) * v2 + (hh * hw) * v1).astype(ft)
        g_w = (lh * (v4 - v3) + hh * (v2 - v1)).astype(ft)
        g_h = (lw * (v4 - v2) + hw * (v3 - v1)).astype(ft)
        rsum = lambda t: t[..., ::-1].sum(-1, dtype=ft)
        z = np.zeros(ins.shape, dtype=ft)
        ga[:, :, :, l] = np.where(ins, rsum(tg * val), z)
        gl[:, :, :, l, :, 0] = np.where(ins, rsum((g_w * ft(W)) * (tg * a)), z)
        gl[:, :, :, l, :, 1] = np.where(ins, rsum((g_h * ft(H)) * (tg * a)), z)
    return gv, gl, ga


BACKWARD = G.bwd_params()


@pytest.mark.parametrize("T,D,L,P,levels,full", BACKWARD)
def test_independent_backward_evaluation_is_inside_the_bound(T, D, L, P, levels, full):
    case = G.bwd_case(T, D, L, P, levels, full)
    ref = G.bwd_reference(case)
    for got, k in zip(backward_lowp(case), ("gv", "gl", "ga")):
        err = np.abs(got.astype(np.float64) - ref[k])
        b = ref[k + "_b"]
        assert bool((err <= b).all()), f"{k}: {int((~(err <= b)).sum())} elements outside, worst err/bound {float(np.nanmax(err / np.maximum(b, 1e-300))):.3f}"


def _caught(y, bnd, ym):
    err = np.abs(ym - y)
    bad = ~(err <= bnd)
    if not bool(bad.any()):
        return None
    i = int(np.argmax(np.where(bad, err / np.maximum(bnd, 1e-300), 0.0)))
    return i, int(bad.sum()), float(err.reshape(-1)[i] / max(bnd.reshape(-1)[i], 1e-300))


FORWARD_MUTANTS = {          # planted mistake -> which cases can show it
    "swap_lhlw": lambda kind, c: True,
    "no_half": lambda kind, c: True,
    "replicate": lambda kind, c: True,
    "level_start_plus1": lambda kind, c: c["L"] > 1,
    "transpose_head_group": lambda kind, c: c["D"] % 8 == 0 and c["D"] > 8,
    "image_plus8": lambda kind, c: c["B"] == 16,
    "vx_vy": lambda kind, c: kind == "fused",
    "div_LP": lambda kind, c: kind == "fused" and c["L"] > 1,
    "softmax_P": lambda kind, c: kind == "fused" and c["L"] > 1,
    "logit_col_minus8": lambda kind, c: kind == "fused",
}


@pytest.mark.parametrize("mutant", sorted(FORWARD_MUTANTS))
def test_planted_forward_mistake_leaves_the_bound(mutant):
    """lh / lw swapped in the corner weights; the -0.5 dropped; edge replication instead of zero padding; the last level's start off by one pixel;
    head and channel group transposed in the output index; image b reading image (b + 8) % B's map; vx / vy swapped; off / (L P) instead of
    off / P; softmax over P instead of L P; logits read from logit_col - 8."""
    seen = []
    for label, kind, case, form in FORWARD:
        if not FORWARD_MUTANTS[mutant](kind, case):
            continue
        y, bnd = G.fwd_reference(case, form) if kind == "fwd" else G.fused_reference(case)
        with np.errstate(over="ignore", invalid="ignore"):
            ym, _ = G.fwd_reference(case, form, (mutant,)) if kind == "fwd" else G.fused_reference(case, (mutant,))
        hit = _caught(y, bnd, ym)
        seen.append(label)
        if hit:
            print(f"{mutant}: caught by {label}: {hit[1]} of {y.size} elements outside, element {hit[0]} at {hit[2]:.3g} x its bound")
            assert hit[2] > 4, f"{mutant}: only {hit[2]:.2f} x the bound on {label}"
            return
    raise AssertionError(f"{mutant} survived {seen}")


@pytest.mark.parametrize("mutant,key", [("swap_xy", "gl"), ("swap_WH", "gl")])
def test_planted_backward_mistake_leaves_the_bound(mutant, key):
    """grad_loc x and y swapped; the W / H scales swapped."""
    for p in BACKWARD:
        case = G.bwd_case(*p.values)
        ref, alt = G.bwd_reference(case), G.bwd_reference(case, (mutant,))
        hit = _caught(ref[key], ref[key + "_b"], alt[key])
        if hit:
            print(f"{mutant}: caught by backward {p.id}: {hit[1]} of {ref[key].size} elements outside, element {hit[0]} at {hit[2]:.3g} x its bound")
            assert hit[2] > 4
            return
    raise AssertionError(f"{mutant} survived every backward case")


def test_edge_replication_is_far_outside_on_every_border_case():
    """The border samples carry weights large enough that replicating the edge is far outside the bound in every case that carries engineered
    border samples (the non-finite variants repeat the same builders and are left out)."""
    for label, kind, case, form in FORWARD:
        if "non-finite" in label:
            continue
        y, bnd = G.fwd_reference(case, form) if kind == "fwd" else G.fused_reference(case)
        ym, _ = G.fwd_reference(case, form, ("replicate",)) if kind == "fwd" else G.fused_reference(case, ("replicate",))
        hit = _caught(y, bnd, ym)
        assert hit and hit[2] > 4, f"{label}: edge replication stays within {0 if not hit else hit[2]:.2f} x the bound"


def _planted(levels, where):
    """Locations (1, 1, 1, L, 1, 2) in the middle of a cell, with ONE coordinate moved to 7e-9 behind a cell edge, the -1 border or the H / W border."""
    loc = np.zeros((1, 1, 1, len(levels), 1, 2))
    for l, (H, W) in enumerate(levels):
        loc[0, 0, 0, l, 0] = ((0.5 + 0.3) / W, (0.5 + 0.3) / H)
    H, W = levels[-1]
    k, n = (0, W) if where.endswith("x") else (1, H)
    im = {"edge": 0.0 if n == 1 else 1.0, "low": -1.0, "high": float(n)}[where[:-2]] + 7e-9
    loc[0, 0, 0, -1, 0, k] = (im + 0.5) / n
    return loc


@pytest.mark.parametrize("where", ["edge_x", "edge_y", "low_x", "low_y", "high_x", "high_y"])
@pytest.mark.parametrize("form", ["forward", "fused", "backward"])
def test_input_condition_rejects_a_planted_near_edge_sample(form, where):
    """assert_locations_safe, called as each case builder (and the backward test before its launch) calls it, raises on one non-engineered sample
    7e-9 from a cell edge / border, accepts the same locations without it, and accepts it once the sample is marked engineered. For the fused and
    backward forms there is no exemption by f32 exactness: a sample exactly ON an edge (f32-exact) is rejected there too, and accepted by the
    forward form."""
    levels = G.LV2
    kw = dict(forward=dict(f32_exempt=True, unit=G.urt(F32)), fused=dict(f32_exempt=False), backward=dict(f32_exempt=False))[form]
    loc = _planted(levels, where)
    none = np.zeros(loc.shape[:5], dtype=bool)
    clean = _planted(levels, where)
    clean[0, 0, 0, -1, 0] = clean[0, 0, 0, 0, 0] * np.array(levels[0][::-1]) / np.array(levels[-1][::-1])
    G.assert_locations_safe(clean, levels, none, form, **kw)
    with pytest.raises(AssertionError, match="cell edge"):
        G.assert_locations_safe(loc, levels, none, form, **kw)
    G.assert_locations_safe(loc, levels, ~none, form, **kw)
    on = np.array(loc)
    on[0, 0, 0, 0, 0, 0] = 3.5 / levels[0][1]           # w_im = 3 exactly on the (5, 7) level: exact in f32
    on[0, 0, 0, -1, 0] = clean[0, 0, 0, -1, 0]
    if form == "forward":
        on32 = np.float64(np.float32(on))
        on32[0, 0, 0, 0, 0, 0] = 0.5                    # 0.5 * 7 - 0.5 = 3: an f32-exact sample on an edge is the forward form's exemption
        G.assert_locations_safe(on32, levels, none, form, **kw)
    else:
        on[0, 0, 0, 0, 0, 0] = 0.5
        with pytest.raises(AssertionError, match="cell edge"):
            G.assert_locations_safe(on, levels, none, form, **kw)


def test_record_names_follow_the_cases():
    """Every launch form the GPU module pins is one of the names the issue fixes (the library's own list is checked on the GPU)."""
    names = {f"msda_vec8_{t}_p{p}" for t in ("f32", "f16", "bf16") for p in ("2", "4", "n")} | {f"msda_generic_{t}" for t in ("f32", "f16", "bf16", "f64")} | \
            {f"msda_fused_{t}_l{l}p{p}" for t in ("f32", "f16", "bf16") for l in (1, 2) for p in (2, 4)}
    used = {form for _, _, _, form in FORWARD}
    assert used == names, sorted(names ^ used)
