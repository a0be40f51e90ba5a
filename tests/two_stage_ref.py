"""Cases, float64 restatement and bounds for the two-stage selection under training (csrc/two_stage_train.hip, lwdetr_amd.ops.two_stage).

Scores. The restatement evaluates, for group g and row r, in float64 on inputs stored in T and widened exactly:
    x = rowvalid ? memory[r] : 0,   h = x W_eo[g]^T + b_eo[g],   y = (h - mean h) / sqrt(var h + 1e-5) * ln_w[g] + ln_b[g]   (y NOT rounded),
    l_c = y W_cls[g, c] + b_cls[g, c],   score = max_c l_c.
Bound of every score element:  |got - ref64| <= max_c [ 4 C 2^-24 M_c + R_c ]  (valid for the maximum: |max a - max b| <= max |a - b|).
  M_c  the sum of the absolute values of the terms of l_c, with LayerNorm's sensitivity carried through: with A_j = sum_k |W_eo[j,k] x_k| +
       |b_eo[j]| the term sum of h_j, n_j = (h_j - mean) rstd, an error e_j in h moves y_j by rstd |ln_w_j| (e_j + mean e + |n_j| mean(|n| e))
       to first order, so  Ay_j = rstd |ln_w_j| (A_j + mean A + |n_j| mean(|n| A)) + 2 |n_j ln_w_j| + |ln_b_j|  (the last two: the roundings of the
       statistics and of y's own two operations), and  M_c = sum_j |W_cls[c,j]| (Ay_j + |y_j|) + |b_cls[c]|.
  C    MEASURED: the worst |score32 - score64| / (2^-24 max_c M_c) of this same restatement run in float32 on the CPU, over all cases and
       dtypes' inputs (C_SCORES below; tests/test_two_stage_host.py measures it again). 4 is the project's margin over a measured reference.
  R_c  DERIVED, 16-bit types only: y is rounded to T once, as the operand of the class GEMM, and the kernel's f32 y may sit on either side of
       a rounding boundary of y64:  R_c = sum_j |W_cls[c,j]| 2 half_ulp_T(y64_j).  0 for float32.

Whole operator (float32). Given the operator's own indices the restatement yields memory_ts, boxes_ts and, by autograd with fixed cotangents,
the gradients of memory and of every parameter, in float64. Per tensor, max |got - ref64| / max |ref64| must be <= 4 x the same figure of the
restatement run in float32 on the CPU, pinned in F32_FIGURE (measured with the restatement's own float64 top-k; the host test measures it
again). The figure is a float32 one, so the whole-operator check runs in float32 - the 16-bit types are covered by the score cases and by
the exact gather / scatter tests.
"""
import math

import torch
import torch.nn.functional as F

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
NAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
EPS = 1e-5
U24 = 2.0 ** -24
MARGIN = 4.0
SENT = 12345.0

# name, d, ncls, G, B, levels, validity: "all" | "random" | "pad1" (image 1 padded to 5/9 of every level's width) | "allpad0" (image 0 all padding)
SCORE_CASES = [
    dict(name="one_row", d=256, ncls=1, G=1, B=1, levels=[(1, 1)], valid="all"),
    dict(name="r63_d384", d=384, ncls=91, G=2, B=1, levels=[(7, 9)], valid="all"),
    dict(name="r65_g13", d=256, ncls=97, G=13, B=1, levels=[(5, 13)], valid="random"),
    dict(name="two_levels_198_pad", d=384, ncls=366, G=2, B=2, levels=[(9, 9), (3, 6)], valid="pad1"),
    dict(name="all_padding_image", d=256, ncls=91, G=2, B=2, levels=[(5, 13)], valid="allpad0"),
    dict(name="three_tiles_g13", d=384, ncls=17, G=13, B=1, levels=[(10, 13)], valid="all"),
]
FALLBACK_CASE = dict(name="fallback_d128", d=128, ncls=5, G=2, B=1, levels=[(3, 11)], valid="random")
ALL_SCORE_CASES = SCORE_CASES + [FALLBACK_CASE]

# measured by measure_c() on the CPU (units of 2^-24 max_c M_c); see the module docstring
C_SCORES = 0.4924

# whole-operator cases (float32)
OP_CASES = [
    dict(name="reparam_pad_g13", d=256, ncls=91, G=13, B=2, levels=[(9, 9), (3, 6)], valid="pad1", nq=17, reparam=True),
    dict(name="unsigmoid_g2", d=384, ncls=97, G=2, B=1, levels=[(5, 7)], valid="all", nq=8, reparam=False),
]
OP_TENSORS = ("memory_ts", "boxes_ts", "g_memory", "g_W_eo", "g_b_eo", "g_ln_w", "g_ln_b", "g_W_box0", "g_b_box0", "g_W_box1", "g_b_box1",
              "g_W_box2", "g_b_box2")
# measured by measure_f32_figure() on the CPU: max |restatement32 - restatement64| / max |restatement64| per tensor over OP_CASES
F32_FIGURE = dict(memory_ts=5.579e-07, boxes_ts=1.115e-07, g_memory=3.765e-07, g_W_eo=2.653e-07, g_b_eo=1.675e-07, g_ln_w=3.219e-07,
                  g_ln_b=1.063e-07, g_W_box0=5.426e-07, g_b_box0=4.100e-07, g_W_box1=3.444e-07, g_b_box1=2.254e-07, g_W_box2=4.891e-07,
                  g_b_box2=2.466e-07)

# the configuration recorded from the unmodified reference Transformer (tools/gen_golden_two_stage.py -> tests/golden/two_stage_train.npz)
GOLDEN_CASE = dict(name="golden", d=256, ncls=91, G=2, B=2, levels=[(9, 11)], valid="pad1", nq=8, reparam=True)
GOLDEN_SCALE = 2.0 ** -7

# gather / scatter cases (exact): S, nq, G, B, d, masked image
SELECT_CASES = [
    dict(name="every_token_many_groups", S=20, nq=17, G=13, B=2, d=40, masked=False),
    dict(name="s_equals_nq", S=9, nq=9, G=3, B=1, d=256, masked=False),
    dict(name="nq1", S=70, nq=1, G=16, B=3, d=384, masked=False),
    dict(name="masked_image", S=33, nq=12, G=5, B=2, d=72, masked=True),
]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def mask_of(case):
    """(B, S) bool padding mask, True = padding, or None."""
    B, S = case["B"], sum(h * w for h, w in case["levels"])
    if case["valid"] in ("all", "random"):
        return None
    m = torch.zeros(B, S, dtype=torch.bool)
    cur = 0
    for h, w in case["levels"]:
        lv = torch.zeros(B, h, w, dtype=torch.bool)
        if case["valid"] == "pad1":
            lv[1, :, max(1, (w * 5) // 9):] = True
            lv[1, max(1, (h * 7) // 9):, :] = True
        else:
            lv[0] = True
        m[:, cur:cur + h * w] = lv.flatten(1)
        cur += h * w
    return m


def proposals64(B, levels, mask, unsigmoid):
    """gen_encoder_output_proposals (transformer.py:71-125) in float32 as the reference, returned with validity; from Python ints."""
    props, cur = [], 0
    for lvl, (h, w) in enumerate(levels):
        gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        grid = torch.stack([gx, gy], -1)[None].expand(B, -1, -1, -1)
        if mask is None:
            scale = torch.tensor([w, h], dtype=torch.float32).view(1, 1, 1, 2)
        else:
            m = mask[:, cur:cur + h * w].view(B, h, w)
            scale = torch.stack([(~m[:, 0, :]).sum(1), (~m[:, :, 0]).sum(1)], 1).view(B, 1, 1, 2).float()
        grid = (grid + 0.5) / scale
        props.append(torch.cat([grid, torch.ones_like(grid) * 0.05 * (2.0 ** lvl)], -1).view(B, -1, 4))
        cur += h * w
    props = torch.cat(props, 1)
    valid = ((props > 0.01) & (props < 0.99)).all(-1)
    if mask is not None:
        valid = valid & ~mask
    if unsigmoid:
        props = torch.log(props / (1 - props)).masked_fill(~valid.unsqueeze(-1), float("inf"))
    else:
        props = props.masked_fill(~valid.unsqueeze(-1), 0.0)
    return props, valid


def make_case(case, dtype, seed=0):
    """Inputs stored in `dtype`: memory (B, S, d), rowvalid (B, S) bool, stacked weights, the box head, mask, proposals."""
    g = _gen(1000 * seed + 17 * case["d"] + case["ncls"] + 7 * case["G"] + sum(h * w for h, w in case["levels"]))
    B, d, ncls, G = case["B"], case["d"], case["ncls"], case["G"]
    S = sum(h * w for h, w in case["levels"])
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dtype)
    inp = dict(case=case, dtype=dtype, S=S)
    inp["memory"] = r(B, S, d)
    inp["W_eo"], inp["b_eo"] = r(G, d, d, scale=d ** -0.5), r(G, d, scale=0.1)
    inp["ln_w"], inp["ln_b"] = (1 + 0.1 * torch.randn(G, d, generator=g)).to(dtype), r(G, d, scale=0.1)
    inp["W_cls"], inp["b_cls"] = r(G, ncls, d, scale=d ** -0.5), r(G, ncls, scale=0.5)
    inp["W_box"] = [r(G, d, d, scale=d ** -0.5), r(G, d, d, scale=d ** -0.5), r(G, 4, d, scale=0.5 * d ** -0.5)]
    inp["b_box"] = [r(G, d, scale=0.1), r(G, d, scale=0.1), r(G, 4, scale=0.1)]
    mask = mask_of(case)
    props, valid = proposals64(B, case["levels"], mask, unsigmoid=not case.get("reparam", True))
    if case["valid"] == "random":
        valid = valid & (torch.rand(B, S, generator=g) > 0.25)
        props = props.masked_fill(~valid.unsqueeze(-1), 0.0 if case.get("reparam", True) else float("inf"))
    inp["mask"], inp["props"], inp["rowvalid"] = mask, props, valid
    if "nq" in case:
        inp["go_mem"] = torch.randn(B, G * case["nq"], d, generator=g)
        inp["go_box"] = torch.randn(B, G * case["nq"], 4, generator=g)
    return inp


def half_ulp(v, dtype):
    """Half an ulp of T at |v| (float64 tensor); 0 for float32 (no rounding to T happens there)."""
    if dtype == torch.float32:
        return torch.zeros_like(v)
    p, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.frexp(v.abs().clamp_min(2.0 ** -140))[1].to(torch.float64) - 1      # floor(log2 |v|)
    return torch.exp2(e.clamp_min(emin) - p - 1)


def scores_ref(inp, ct=torch.float64, mutate=None):
    """-> (scores (G, B, S) in ct, M (G, B, S) = max_c M_c, R (G, B, S) = max_c-compatible rounding term: returned per class-maximum below).
    `mutate` plants a mistake: "swap_groups" (group 0 scored with group 1's W_eo), "no_eps" (LayerNorm eps dropped)."""
    dt = inp["dtype"]
    x = inp["memory"].to(ct) * inp["rowvalid"].unsqueeze(-1).to(ct)
    G = inp["W_eo"].shape[0]
    eps = 0.0 if mutate == "no_eps" else EPS
    S_, M_, B_ = [], [], []
    for g in range(G):
        gw = (g + 1) % G if mutate == "swap_groups" else g
        W, b = inp["W_eo"][gw].to(ct), inp["b_eo"][g].to(ct)
        lw, lb = inp["ln_w"][g].to(ct), inp["ln_b"][g].to(ct)
        Wc, bc = inp["W_cls"][g].to(ct), inp["b_cls"][g].to(ct)
        h = x @ W.T + b
        A = x.abs() @ W.abs().T + b.abs()
        mu = h.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((h - mu) ** 2).mean(-1, keepdim=True) + eps)
        n = (h - mu) * rstd
        y = n * lw + lb
        Ay = rstd * lw.abs() * (A + A.mean(-1, keepdim=True) + n.abs() * (n.abs() * A).mean(-1, keepdim=True)) + 2 * (n * lw).abs() + lb.abs()
        logits = y @ Wc.T + bc
        Mc = (Ay + y.abs()) @ Wc.abs().T + bc.abs()
        Rc = (2 * half_ulp(y.double(), dt)).to(ct) @ Wc.abs().T
        S_.append(logits.amax(-1)); M_.append(Mc); B_.append(Rc)
    return torch.stack(S_), torch.stack(M_), torch.stack(B_)


def score_bound(M, R, c=None):
    """max_c [ 4 C 2^-24 M_c + R_c ] per score element."""
    c = C_SCORES if c is None else c
    return (MARGIN * c * U24 * M + R).amax(-1)


def stable_topk(scores, k):
    """Descending, ties by ascending index - the documented order of lwdetr_topk."""
    return torch.sort(scores, dim=-1, descending=True, stable=True)[1][..., :k]


def measure_c():
    worst = 0.0
    for case in ALL_SCORE_CASES:
        for dt in DTYPES:
            inp = make_case(case, dt)
            s64, M, _ = scores_ref(inp)
            s32, _, _ = scores_ref(inp, torch.float32)
            worst = max(worst, float(((s32.double() - s64).abs() / (U24 * M.amax(-1))).max()))
    return worst


# ------------------------------------------------------------------------------------------------------------------- whole operator
def operator_ref(inp, idx, ct=torch.float64, mutate=None):
    """The block after the top-k on the selected rows, as the reference computes it on all rows and gathers (transformer.py:231-264), in ct,
    with autograd: -> {tensor name: value}. idx (G, B, nq). `mutate`: "descending_g" sums the row gradients of memory in descending g (only
    float32 / 16-bit sums can tell - used by the exact scatter test's planted mistake)."""
    case = inp["case"]
    B, d, G, nq = case["B"], case["d"], case["G"], case["nq"]
    leaf = lambda t: t.to(ct).clone().requires_grad_(True)
    mem = leaf(inp["memory"])
    P = dict(W_eo=leaf(inp["W_eo"]), b_eo=leaf(inp["b_eo"]), ln_w=leaf(inp["ln_w"]), ln_b=leaf(inp["ln_b"]))
    for i in range(3):
        P[f"W_box{i}"], P[f"b_box{i}"] = leaf(inp["W_box"][i]), leaf(inp["b_box"][i])
    x = mem * inp["rowvalid"].unsqueeze(-1).to(ct)
    props = inp["props"].to(ct)
    mts, bts = [], []
    for g in range(G):
        xs = torch.gather(x, 1, idx[g].unsqueeze(-1).expand(B, nq, d))
        ps = torch.gather(props, 1, idx[g].unsqueeze(-1).expand(B, nq, 4))
        y = F.layer_norm(F.linear(xs, P["W_eo"][g], P["b_eo"][g]), (d,), P["ln_w"][g], P["ln_b"][g], EPS)
        h = y
        for i in range(3):
            h = F.linear(h, P[f"W_box{i}"][g], P[f"b_box{i}"][g])
            if i < 2:
                h = F.relu(h)
        if case["reparam"]:
            box = torch.cat([h[..., :2] * ps[..., 2:] + ps[..., :2], h[..., 2:].exp() * ps[..., 2:]], -1)
        else:
            box = h + ps
        mts.append(y); bts.append(box)
    memory_ts, boxes_ts = torch.cat(mts, 1), torch.cat(bts, 1)
    finite = torch.isfinite(boxes_ts)
    loss = (memory_ts * inp["go_mem"].to(ct)).sum() + (torch.where(finite, boxes_ts, torch.zeros_like(boxes_ts)) * inp["go_box"].to(ct)).sum()
    names = list(P)
    grads = torch.autograd.grad(loss, [mem] + [P[k] for k in names])
    out = dict(memory_ts=memory_ts.detach(), boxes_ts=boxes_ts.detach(), g_memory=grads[0])
    out.update({f"g_{k}": v for k, v in zip(names, grads[1:])})
    return out


def figure(got, ref):
    """max |got - ref| / max |ref| over the finite reference entries (non-finite ones - the un-sigmoided form's inf boxes of invalid rows - must
    sit in the same places)."""
    ref = ref.double()
    got = got.double()
    fin = torch.isfinite(ref)
    if not torch.equal(fin, torch.isfinite(got)) or not torch.equal(ref[~fin], got[~fin]):
        return math.inf
    if not fin.any():
        return 0.0
    den = float(ref[fin].abs().max())
    return float((got[fin] - ref[fin]).abs().max()) / den if den > 0 else float((got[fin] - ref[fin]).abs().max())


def own_idx(inp):
    """The restatement's own float64 selection (used where no operator is at hand: the host measurements)."""
    s64, _, _ = scores_ref(inp)
    return stable_topk(s64, inp["case"]["nq"])


def measure_f32_figure():
    fig = {t: 0.0 for t in OP_TENSORS}
    for case in OP_CASES:
        inp = make_case(case, torch.float32)
        idx = own_idx(inp)
        r64, r32 = operator_ref(inp, idx), operator_ref(inp, idx, torch.float32)
        for t in OP_TENSORS:
            fig[t] = max(fig[t], figure(r32[t], r64[t]))
    return fig


# ------------------------------------------------------------------------------------------------------------------- gather / scatter
def make_select_case(case, dtype, seed=0):
    g = _gen(seed + case["S"] * 131 + case["nq"])
    B, S, G, nq, d = case["B"], case["S"], case["G"], case["nq"], case["d"]
    memory = torch.randn(B, S, d, generator=g).to(dtype)
    rowvalid = torch.ones(B, S, dtype=torch.bool)
    if case["masked"]:
        rowvalid[1, S // 3:] = False
    idx = torch.stack([torch.stack([torch.randperm(S, generator=g)[:nq] for _ in range(B)]) for _ in range(G)])
    props = torch.rand(B, S, 4, generator=g)
    # magnitudes spread over 2^-10 .. 2^10, so that the f32 sum of a row's groups rounds - and depends on its order - in the 16-bit types too
    grad = (torch.randn(B, G, nq, d, generator=g) * torch.exp2(torch.randint(-10, 11, (B, G, nq, d), generator=g).float())).to(dtype)
    return dict(memory=memory, rowvalid=rowvalid, idx=idx, props=props, grad=grad)


def gather_ref(sc):
    mem = sc["memory"] * sc["rowvalid"].unsqueeze(-1).to(sc["memory"].dtype)
    G, B, nq = sc["idx"].shape
    x = torch.stack([torch.stack([mem[b, sc["idx"][g, b]] for g in range(G)]) for b in range(B)])
    p = torch.stack([torch.stack([sc["props"][b, sc["idx"][g, b]] for g in range(G)]) for b in range(B)])
    return x, p


def scatter_ref(sc, descending=False):
    """The loop of the contract: f32 accumulator, groups in ascending g, one rounding. `descending` is the planted mistake."""
    G, B, nq = sc["idx"].shape
    S, d = sc["memory"].shape[1:]
    acc = torch.zeros(B, S, d, dtype=torch.float32)
    gr = sc["grad"].float()
    for g in (range(G - 1, -1, -1) if descending else range(G)):
        for b in range(B):
            acc[b, sc["idx"][g, b]] = acc[b, sc["idx"][g, b]] + gr[b, g]
    acc = acc * sc["rowvalid"].unsqueeze(-1).float()
    return acc.to(sc["memory"].dtype)


# ------------------------------------------------------------------------------------------------------------------- golden
def golden_floats(q):
    """The golden's int8 inputs {name: int8 tensor} as float32: value * 2^-7, LayerNorm weights 1 + value * 2^-7."""
    out = {k: v.float() * GOLDEN_SCALE for k, v in q.items()}
    out["ln_w"] = 1.0 + q["ln_w"].float() * GOLDEN_SCALE
    return out


def golden_inputs(f):
    """The golden configuration in the shape the restatement takes (f: golden_floats)."""
    case = GOLDEN_CASE
    mask = mask_of(case)
    props, valid = proposals64(case["B"], case["levels"], mask, unsigmoid=False)
    inp = dict(case=case, dtype=torch.float32, S=props.shape[1], memory=f["src"].flatten(2).transpose(1, 2).contiguous(), mask=mask, props=props,
               rowvalid=valid, W_box=[f["W_box0"], f["W_box1"], f["W_box2"]], b_box=[f["b_box0"], f["b_box1"], f["b_box2"]])
    for k in ("W_eo", "b_eo", "ln_w", "ln_b", "W_cls", "b_cls"):
        inp[k] = f[k]
    g = _gen(5)
    inp["go_mem"] = torch.randn(case["B"], case["G"] * case["nq"], case["d"], generator=g)
    inp["go_box"] = torch.randn(case["B"], case["G"] * case["nq"], 4, generator=g)
    return inp


def load_golden(path):
    import numpy as np
    z = np.load(path)
    q = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in_")}
    rest = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if not k.startswith("in_")}
    return q, rest
