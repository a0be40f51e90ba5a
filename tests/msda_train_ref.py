"""Shared by test_msda_train_host.py (CPU) and test_gpu_msda_train.py (GPU): the cases, a float64 restatement (torch, with autograd) of the
differentiable deformable cross-attention (csrc/msda_train.hip), the per-element magnitudes and the bound.

Operation, per (row = b Q + q, head m), level l of H x W pixels starting at value row level_start[l], point p:
    loc = ref_xy[row, l] + off / P * ref_wh[row, l] * 0.5,   a = softmax over the L P logits of (row, m),
    (w_im, h_im) = loc * (W, H) - 0.5;  a sample counts iff h_im > -1, w_im > -1, h_im < H, w_im < W;  corners outside the map and masked
    value rows read as zero;   out[b, q, m D + c] = sum_{l,p} a bilinear(value[b, level l, m, c]).
The gradients are those of torch autograd on this restatement in float64 (floor has no derivative); inputs are stored in T and widened exactly.

Bound, for EVERY element e of out, grad_value, grad_offsets, grad_logits, grad_ref:
    |got - ref64| <= 4 C[tensor] 2^-24 M_e + half_ulp_T(|ref64_e|)
M_e is the sum of the absolute values of the element's terms in the float64 evaluation (evaluate(absolute=True) below: every product of the chain with
|value|, |grad_out|, |off| and the non-negative weights, summed without cancellation; for the softmax backward a_i (G_i + sum_j a_j G_j)).
C[tensor] (C_MEASURED) is the worst (|f32 - f64| - half_ulp_f32)+ / (2^-24 M_e) of this same restatement run in float32 under CPU autograd on the cases below,
over the inputs of all three dtypes; test_msda_train_host.py measures it again and pins the table. The factor 4 is the project's margin over a
measured reference (attn_train_ref.py, test_gpu_vitblock.py). The kernel uses expf and a true division - no hardware approximation - so the
bound carries no transcendental term. T of grad_ref is float32 (the kernel writes it in f32), T of the others the input dtype.

Condition on the inputs, asserted by make_case: grad_loc is discontinuous where h_im or w_im is an integer, so every sample that is not
engineered stays at least 8 2^-23 max(H, W) away from every integer h_im / w_im (the distance condition of tests/test_gpu_msda_fp64.py).
The cases keep 2^-5 where that is more: a corner weight is the distance d to a cell edge, its error in f32 is that of the coordinate, about
2^-24 |h_im|, and M_e has no term for it - an element that a single corner feeds (a grad_value pixel, an out element of a sample in the border
cell) then carries a relative error of 2^-24 |h_im| / d, in the reference and in the kernel alike. With d >= 2^-5 that stays at a few hundred
units and C describes the arithmetic; at d = 10^-5 one sample in 10^5 would set C to 10^5 for everything else.
Near-edge case (NEAR_EDGE_CASES): samples between twice the issue's distance and 2^-5 from a cell edge, so that the cells next to an edge are
exercised too. Its bound adds 4 E_e, E_e (coordinate_terms()) being the first-order effect of the coordinate's own f32 roundings - 2^-24 (2 |t| H +
2 |loc| H + |h_im|) per coordinate, one rounding per operation of the chain - on the element, summed without a sign; the margin 4 is the one of
the first term. C is not measured on this case and the other cases' bound has no such term.
Engineered samples (their h_im / w_im are exact in f32 and f64 alike, by construction: boxes of size 0 with dyadic centres): exactly at -1 and at
H / W (no contribution), and the zero-size boxes.
"""
import torch

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = (F32, F16, BF16)
NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
PREC = {F32: 24, F16: 11, BF16: 8}
EMIN = {F32: -126, F16: -14, BF16: -126}
U32 = 2.0 ** -24
TENSORS = ("out", "grad_value", "grad_offsets", "grad_logits", "grad_ref")
OUT_DTYPE = {"grad_ref": F32}
SENT = 1234.0
GUARD = 3
SLAB_FLOATS = 2048              # msda_train.hip: f32 elements of one band of the pixel kernel (band = SLAB_FLOATS / D value rows)
CHUNK = 512                     # records the pixel kernel reads per step
MIN_DIST = 2.0 ** -5            # see "Condition on the inputs"

# Worst (|f32 - f64| - half_ulp_f32)+ / (2^-24 M_e) of the restatement in float32 over CASES x DTYPES (measure_constants(); pinned by
# test_msda_train_host.py)
C_MEASURED = {"out": 317.4, "grad_value": 260.7, "grad_offsets": 129.8, "grad_logits": 130.5, "grad_ref": 38.80}


def _case(name, B, Q, M, D, levels, P, gap=0, strided=False, mask=None, collide=False, near_edge=False):
    return dict(name=name, B=B, Q=Q, M=M, D=D, levels=levels, P=P, gap=gap, strided=strided, mask=mask, collide=collide, near_edge=near_edge)


# the smallest shapes at which work split and indexing can go wrong: Q around the item group (256 / (D / 8) / M queries per workgroup), the wave
# and the workgroup; S above one band of the pixel kernel (D = 64: 32 rows, D = 32: 64, D = 16: 128) with a band edge inside a level; Q P above one chunk
# of records; level_start with a gap; L P = 16; strided views; both model pairs ((L, P) = (1, 2) with 16 heads, (2, 4) with 24) at few queries
CASES = [
    _case("q1_m1_d8_p1", 1, 1, 1, 8, [(3, 5)], 1),
    _case("q3_m3_d16_p2_gap", 2, 3, 3, 16, [(2, 2), (1, 7)], 2, gap=3),
    _case("q17_m3_d64_p4_gap_maskpx", 1, 17, 3, 64, [(8, 8), (4, 4), (2, 2)], 4, gap=5, mask="pixel"),
    _case("q65_m1_d64_p2_strided", 1, 65, 1, 64, [(3, 5)], 2, strided=True),
    _case("q257_m3_d8_p1_maskimg", 3, 257, 3, 8, [(2, 2), (1, 7)], 1, gap=1, mask="image"),
    _case("q17_m3_d16_lp16", 1, 17, 3, 16, [(8, 8), (4, 4), (2, 2), (3, 5)], 4, gap=2),
    _case("q65_m16_d32_p2_2lvl_strided", 2, 65, 16, 32, [(8, 8), (9, 9)], 2, gap=7, strided=True, mask="pixel"),
    _case("small_pair_m16_l1p2", 2, 65, 16, 16, [(5, 5)], 2, strided=True),
    _case("large_pair_m24_l2p4", 1, 33, 24, 16, [(8, 8), (2, 2)], 4),
    _case("collide_q257_m3_d16_l1p2", 1, 257, 3, 16, [(3, 5)], 2, collide=True),
]
# Samples between the issue's own distance (8 2^-23 max(H, W)) and 2^-5 from a cell edge: not part of CASES (C is not measured on it), checked
# under the bound plus the coordinate term E_e of coordinate_terms() - see "Near-edge case" in the module docstring
NEAR_EDGE_CASES = [_case("near_edge_q65_m3_d16_p2", 1, 65, 3, 16, [(8, 8), (5, 7)], 2, gap=1, near_edge=True)]
ALL_CASES = CASES + NEAR_EDGE_CASES
GOLDEN_CASES = ("q3_m3_d16_p2_gap", "q17_m3_d64_p4_gap_maskpx", "q257_m3_d8_p1_maskimg", "small_pair_m16_l1p2")


def form(case):
    L, P = len(case["levels"]), case["P"]
    return "l1p2" if (L, P) == (1, 2) else "l2p4" if (L, P) == (2, 4) else "gen"


def half_ulp(v, dtype):
    """Half the spacing of `dtype` at |v| (float64 tensor)."""
    _, e = torch.frexp(v.abs().double())
    e = (e - 1).clamp_min(EMIN[dtype])
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - PREC[dtype])


_CACHE = {}


def cached(key, fn):
    """Cases and references are computed once and shared between the tests that need them; nothing modifies them."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def level_layout(case):
    """-> shapes (L, 2) int64, level_start (L,) int64 (with the case's gap before every level), S."""
    starts, s = [], 0
    for (h, w) in case["levels"]:
        s += case["gap"]
        starts.append(s)
        s += h * w
    return torch.tensor(case["levels"], dtype=torch.int64), torch.tensor(starts, dtype=torch.int64), s + case["gap"]


def _im_coords(off, ref, shapes, P):
    """float64 (w_im, h_im) of every sample: (B, Q, M, L, P) each."""
    loc = ref[:, :, None, :, None, :2] + off / P * ref[:, :, None, :, None, 2:] * 0.5
    wh = torch.stack((shapes[:, 1], shapes[:, 0]), -1).double()[None, None, None, :, None, :]
    im = loc * wh - 0.5
    return im[..., 0], im[..., 1]


def make_case(case, dtype):
    """-> dict of CPU tensors: value (B, S, M, D), off (B, Q, M, L, P, 2), lg (B, Q, M, L P), go (B, Q, M D) in `dtype`, ref (B, Q, L, 4) f32,
    mask (B, S) bool or None, shapes, lsi, and `engineered` (B, Q) bool: rows whose samples are exempt from the distance condition."""
    def build():
        B, Q, M, D, P = case["B"], case["Q"], case["M"], case["D"], case["P"]
        shapes, lsi, S = level_layout(case)
        L = shapes.shape[0]
        g = torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(case["name"])) + PREC[dtype])
        rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
        value = torch.randn(B, S, M, D, generator=g, dtype=torch.float64).to(dtype)
        go = torch.randn(B, Q, M * D, generator=g, dtype=torch.float64).to(dtype)
        lg = (torch.randn(B, Q, M, L * P, generator=g, dtype=torch.float64) * 2).to(dtype)
        # boxes: centres inside the map, sizes up to the whole map so that samples leave the map on every side
        ref = torch.cat((rnd(B, Q, 1, 2).expand(B, Q, L, 2) * 1.2 - 0.1, rnd(B, Q, 1, 2).expand(B, Q, L, 2) * 1.5 + 0.05), -1).float().contiguous()
        if L > 1:                                           # per-level boxes differ, as with valid ratios below 1
            ref = (ref * (1.0 - 0.1 * torch.arange(L, dtype=torch.float32)[None, None, :, None])).contiguous()
        off = ((rnd(B, Q, M, L, P, 2) * 2 - 1) * 1.5 * P).to(dtype)
        engineered = torch.zeros(B, Q, dtype=torch.bool)
        if case["collide"]:                                 # every query of every head aims at the cell (1, 2) of the 3 x 5 map
            H, W = case["levels"][0]
            ref[..., 0], ref[..., 1], ref[..., 2], ref[..., 3] = 3.0 / W, 2.0 / H, 0.5 / W, 0.5 / H      # w_im in 2.5 +- 0.375, h_im in 1.5 +- 0.375
            off = ((rnd(B, Q, M, L, P, 2) * 2 - 1) * 1.4 * P).to(dtype)
        # engineered rows (from the end, so that Q = 1 keeps a plain row only when there is nothing to spare)
        # with boxes of size 0 and dyadic centres, every coordinate of these rows is exact in f32 and in f64, on every level. Where the first
        # level's H / W is a power of two (8 x 8, 2 x 2) they sit exactly at w_im = -1 and at h_im = H; elsewhere they are plain zero-size boxes
        H0, W0 = (n if n & (n - 1) == 0 else 4 for n in case["levels"][0])
        eng = []
        if Q >= 3 and not case["collide"]:
            eng = [(Q - 1, (-0.5 / W0, 0.5 / H0, 0.0, 0.0)),                                              # w_im = -1 exactly
                   (Q - 2, (0.5, (H0 + 0.5) / H0, 0.0, 0.0)),                                             # h_im = H exactly
                   (Q - 3, (1.0 / W0, 1.0 / H0, 0.0, 0.0))]                                               # a zero-size box in the map
        for (q, box) in eng:
            ref[:, q, :, :] = torch.tensor(box, dtype=torch.float32)
            engineered[:, q] = True
        if Q >= 5 and not case["collide"]:
            lg[:, 0, :, :] = torch.linspace(0.0, -60.0, L * P, dtype=torch.float64).to(dtype) if L * P > 1 else 0.0     # one key dominates
            lg[:, 1, :, :] = 0.0                                                                                          # all equal
            # outside the map on every side: head 0 of row 2
            ref[:, 2, :, :] = torch.tensor([0.5, 0.5, 1.0, 1.0])
            far = torch.tensor([[-1.7, 0.1], [1.7, 0.1], [0.1, -1.7], [0.1, 1.7]], dtype=torch.float64) * P
            for i in range(L * P):
                off[:, 2, 0, i // P, i % P, :] = far[i % 4].to(dtype)
        # the distance condition: move every sample that is too near an integer coordinate (evaluated on the stored numbers)
        eps = torch.tensor([max(8 * 2.0 ** -23 * max(h, w), MIN_DIST) for (h, w) in case["levels"]], dtype=torch.float64)[None, None, None, :, None]
        plain = ~engineered[:, :, None, None, None]
        wh = torch.stack((shapes[:, 1], shapes[:, 0]), -1).double()[None, None, None, :, None, :]
        per_px = P / (ref.double()[:, :, None, :, None, 2:].clamp_min(1e-3) * 0.5 * wh)          # offset units per pixel
        for _ in range(200):
            x, y = _im_coords(off.double(), ref.double(), shapes, P)
            near = lambda t: (t - t.round()).abs() < eps
            bad = (near(x) | near(y)) & plain
            if not bool(bad.any()):
                break
            off = torch.where(bad[..., None], (off.double() + (rnd(*off.shape) - 0.5) * 0.5 * per_px).to(dtype), off)    # up to a quarter pixel
        x, y = _im_coords(off.double(), ref.double(), shapes, P)
        assert not bool((((x - x.round()).abs() < eps) | ((y - y.round()).abs() < eps))[plain.expand_as(x)].any()), "distance condition"
        if case["collide"]:
            assert bool(((x > 2) & (x < 3) & (y > 1) & (y < 2)).all()), "collision case: every sample in one cell"
        if case.get("near_edge"):
            # 70 % of the coordinates go to a distance d from their nearest cell edge, log-uniform between twice the issue's minimum and 2^-5
            lo = torch.tensor([16 * 2.0 ** -23 * max(h, w) for (h, w) in case["levels"]], dtype=torch.float64)[None, None, None, :, None, None]
            im = torch.stack((x, y), -1)
            side = torch.where(im >= im.round(), 1.0, -1.0)
            d = torch.exp(torch.log(lo) + rnd(*im.shape) * (torch.log(torch.tensor(MIN_DIST, dtype=torch.float64)) - torch.log(lo)))
            move = (rnd(*im.shape) < 0.7) & plain[..., None]
            off = torch.where(move, (off.double() + (im.round() + side * d - im) * per_px).to(dtype), off)
            for _ in range(200):                            # the stored offset is rounded to T: push back what fell below the minimum
                x, y = _im_coords(off.double(), ref.double(), shapes, P)
                im = torch.stack((x, y), -1)
                bad = ((im - im.round()).abs() < lo) & plain[..., None]
                if not bool(bad.any()):
                    break
                side = torch.where(im >= im.round(), 1.0, -1.0)
                off = torch.where(bad, (off.double() + side * rnd(*im.shape) * MIN_DIST * per_px).to(dtype), off)
            x, y = _im_coords(off.double(), ref.double(), shapes, P)
            dist = torch.stack((x - x.round(), y - y.round()), -1).abs()[plain.expand_as(x)]
            assert bool((dist >= lo.min() / 2).all()) and not bool((dist < (lo / 2).expand(B, Q, M, L, P, 2)[plain.expand_as(x)]).any()), "distance condition"
            near = float((dist < MIN_DIST).double().mean())
            assert near > (0.4 if dtype == F32 else 0.05), near          # 16-bit offsets cannot be placed that finely; what lands there counts
        mask = None
        if case["mask"] is not None:
            mask = torch.zeros(B, S, dtype=torch.bool)
            if case["mask"] == "image":
                mask[B - 1] = True                          # one image fully masked
                mask[0, int(lsi[0])] = True
            # a masked pixel under a sample: the top-left corner of the first in-map sample of image 0, and every 7th row
            mask[0, ::7] = True
            inside = (y[0] > 0) & (x[0] > 0) & (y[0] < shapes[:, 0].double()[None, None, :, None] - 1) & (x[0] < shapes[:, 1].double()[None, None, :, None] - 1)
            q, m, l, p = (int(t[0]) for t in torch.nonzero(inside, as_tuple=True))
            mask[0, int(lsi[l]) + int(y[0, q, m, l, p].floor()) * int(shapes[l, 1]) + int(x[0, q, m, l, p].floor())] = True
        return dict(value=value, off=off, lg=lg, go=go, ref=ref, mask=mask, shapes=shapes, lsi=lsi, S=S, engineered=engineered, case=case, dtype=dtype)
    return cached(("case", case["name"], dtype), build)


# ----------------------------------------------------------------------------------------------------------------------- the restatement
def _gather(v, idx):
    """v (B, S, M, D), idx (B, Q, M, P) int64 rows -> (B, Q, M, P, D)."""
    B, Q, M, P = idx.shape
    bi = torch.arange(B, device=idx.device)[:, None, None, None].expand_as(idx)
    mi = torch.arange(M, device=idx.device)[None, None, :, None].expand_as(idx)
    return v[bi, idx, mi]


def _level_pieces(v, x, y, H, W, start):
    """Corner values (validity applied) and fractions of one level: x, y (B, Q, M, P) -> vk list of 4 (B, Q, M, P, D), lw, lh, inside, idx, valid."""
    inside = (y > -1) & (x > -1) & (y < H) & (x < W)
    y0, x0 = torch.floor(y).detach(), torch.floor(x).detach()
    lh, lw = y - y0, x - x0
    vk, idxs, valids = [], [], []
    for k in range(4):
        yy, xx = y0 + (k >> 1), x0 + (k & 1)
        valid = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (start + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()
        vk.append(_gather(v, idx) * valid[..., None].to(v.dtype))
        idxs.append(idx); valids.append(valid)
    return vk, lw, lh, inside, idxs, valids


def core(value, off, lg, ref, mask, shapes, lsi, P):
    """The definition in torch, in the dtype of its operands, differentiable: -> out (B, Q, M D)."""
    B, S, M, D = value.shape
    Q, L = ref.shape[1], shapes.shape[0]
    v = value if mask is None else value.masked_fill(mask[:, :, None, None], 0.0)
    loc = ref[:, :, None, :, None, :2] + off / P * ref[:, :, None, :, None, 2:] * 0.5
    e = (lg - lg.amax(-1, keepdim=True).detach()).exp()      # the softmax written out: exp of the shifted logits (the shift has no derivative), one division
    a = (e / e.sum(-1, keepdim=True)).reshape(B, Q, M, L, P)
    out = 0
    for l in range(L):
        H, W = int(shapes[l, 0]), int(shapes[l, 1])
        x, y = loc[:, :, :, l, :, 0] * W - 0.5, loc[:, :, :, l, :, 1] * H - 0.5
        vk, lw, lh, _, _, _ = _level_pieces(v, x, y, H, W, int(lsi[l]))
        hh, hw = 1 - lh, 1 - lw
        bil = (hh * hw)[..., None] * vk[0] + (hh * lw)[..., None] * vk[1] + (lh * hw)[..., None] * vk[2] + (lh * lw)[..., None] * vk[3]
        out = out + (a[:, :, :, l, :, None] * bil).sum(3)
    return out.reshape(B, Q, M * D)


def restate(inp, ct):
    """The restatement in compute type `ct` under autograd: out and the four gradients."""
    def build():
        value, off, lg, ref = (inp[n].detach().to(ct, copy=True).requires_grad_(True) for n in ("value", "off", "lg", "ref"))
        out = core(value, off, lg, ref, inp["mask"], inp["shapes"], inp["lsi"], inp["case"]["P"])
        out.backward(inp["go"].to(ct))
        return dict(out=out.detach(), grad_value=value.grad, grad_offsets=off.grad, grad_logits=lg.grad, grad_ref=ref.grad)
    return cached(("restate", inp["case"]["name"], inp["dtype"], ct), build)


def evaluate(inp, ct=torch.float64, mistake=None, absolute=False):
    """An explicit evaluation of the forward and of the chain rule the kernels implement (no autograd), in compute type `ct`.
    absolute=True: the magnitudes - every product with |value|, |grad_out|, |off|, |ref_wh| and the non-negative weights, summed without a sign.
    mistake: one of MISTAKES, planted in the backward."""
    case = inp["case"]
    P, shapes, lsi, mask = case["P"], inp["shapes"], inp["lsi"], inp["mask"]
    value, off, lg, ref, go = (inp[n].to(ct) for n in ("value", "off", "lg", "ref", "go"))
    B, S, M, D = value.shape
    Q, L = ref.shape[1], shapes.shape[0]
    A = (lambda t: t.abs()) if absolute else (lambda t: t)
    sg = 1.0 if absolute else -1.0
    v = value if mask is None else value.masked_fill(mask[:, :, None, None], 0.0)
    v, tg = A(v), A(go).reshape(B, Q, M, 1, D)
    loc = ref[:, :, None, :, None, :2] + off / P * ref[:, :, None, :, None, 2:] * 0.5
    a = lg.softmax(-1).reshape(B, Q, M, L, P)
    out = torch.zeros(B, Q, M, D, dtype=ct)
    gv = torch.zeros(B, S, M, D, dtype=ct)
    g_a = torch.zeros(B, Q, M, L, P, dtype=ct)
    g_off = torch.zeros(B, Q, M, L, P, 2, dtype=ct)
    g_ref = torch.zeros(B, Q, L, 4, dtype=ct)
    bi = torch.arange(B)[:, None, None, None].expand(B, Q, M, P)
    mi = torch.arange(M)[None, None, :, None].expand(B, Q, M, P)
    for l in range(L):
        H, W = int(shapes[l, 0]), int(shapes[l, 1])
        start = int(lsi[(l + 1) % L]) if mistake == "neighbour_level_start" else int(lsi[l])
        x, y = loc[:, :, :, l, :, 0] * W - 0.5, loc[:, :, :, l, :, 1] * H - 0.5
        vk, lw, lh, inside, idxs, valids = _level_pieces(v, x, y, H, W, min(start, S - H * W))
        hh, hw = 1 - lh, 1 - lw
        if mistake == "lh_hh_swapped":
            cw = [lh * hw, lh * lw, hh * hw, hh * lw]
        else:
            cw = [hh * hw, hh * lw, lh * hw, lh * lw]
        al = a[:, :, :, l, :]
        bil = sum(cw[k][..., None] * vk[k] for k in range(4))
        out += (al[..., None] * bil).sum(3)
        g_a[:, :, :, l, :] = (tg * bil).sum(-1)
        gw = sg * hh[..., None] * vk[0] + hh[..., None] * vk[1] + sg * lh[..., None] * vk[2] + lh[..., None] * vk[3]
        gh = sg * hw[..., None] * vk[0] + sg * lw[..., None] * vk[1] + hw[..., None] * vk[2] + lw[..., None] * vk[3]
        ins = inside.to(ct)
        gx, gy = W * al * (tg * gw).sum(-1) * ins, H * al * (tg * gh).sum(-1) * ins
        for k in range(4):
            gv.index_put_((bi, idxs[k], mi), (al * cw[k] * valids[k].to(ct))[..., None] * tg, accumulate=True)
        rw, rh = A(ref[:, :, None, l, None, 2]), A(ref[:, :, None, l, None, 3])
        if mistake == "wh_swapped":
            rw, rh = rh, rw
        half = 1.0 if mistake == "no_half" else 0.5
        pd = 1.0 if mistake == "off_no_P" else float(P)
        g_off[:, :, :, l, :, 0], g_off[:, :, :, l, :, 1] = gx * rw * half / pd, gy * rh * half / pd
        ox, oy = A(off[:, :, :, l, :, 0]), A(off[:, :, :, l, :, 1])
        parts = torch.stack((gx, gy, gx * ox * half / P, gy * oy * half / P), -1)              # (B, Q, M, P, 4)
        g_ref[:, :, l, :] = parts[:, :, 0].sum(2) if mistake == "ref_not_over_heads" else parts.sum((2, 3))
    if mask is not None and mistake != "mask_ignored_gv":
        gv = gv.masked_fill(mask[:, :, None, None], 0.0)
    af, gf = a.reshape(B, Q, M, L * P), g_a.reshape(B, Q, M, L * P)
    dot = (af * gf).sum(-1, keepdim=True)
    g_lg = af * gf if mistake == "softmax_no_dot" else af * (gf + dot if absolute else gf - dot)
    return dict(out=out.reshape(B, Q, M * D), grad_value=gv, grad_offsets=g_off, grad_logits=g_lg, grad_ref=g_ref)


def coordinate_terms(inp):
    """E_<tensor>: what the rounding of a sample's coordinates in f32 can move each element by, to first order, in float64. The chain
    t = off / P * size * 0.5, loc = ref + t, h_raw = loc H, h_im = h_raw - 0.5 has one rounding each (the 0.5 is exact), so
    |delta h_im| <= 2^-24 (2 |t| H + 2 |loc| H + |h_im|) =: dy, and dx alike. A corner weight moves by dy |d w_k / d h| + dx |d w_k / d w| with
    |d w_k / d h| = hw or lw and |d w_k / d w| = hh or lh; d out / d loc_x = W a sum_c go (-hh v0 + hh v1 - lh v2 + lh v3) depends on h_im alone,
    with slope +-1 per corner, and d out / d loc_y on w_im alone. Every product is taken with |value|, |grad_out|, |off|, |size| and summed without
    a sign, as for M_e; the chain rule's factors are those of evaluate()."""
    case = inp["case"]
    P, shapes, lsi, mask = case["P"], inp["shapes"], inp["lsi"], inp["mask"]
    ct = torch.float64
    value, off, lg, ref, go = (inp[n].to(ct) for n in ("value", "off", "lg", "ref", "go"))
    B, S, M, D = value.shape
    Q, L = ref.shape[1], shapes.shape[0]
    v = (value if mask is None else value.masked_fill(mask[:, :, None, None], 0.0)).abs()
    tg = go.abs().reshape(B, Q, M, 1, D)
    t = off / P * ref[:, :, None, :, None, 2:] * 0.5
    loc = ref[:, :, None, :, None, :2] + t
    a = lg.softmax(-1).reshape(B, Q, M, L, P)
    out, gv = torch.zeros(B, Q, M, D, dtype=ct), torch.zeros(B, S, M, D, dtype=ct)
    g_a, g_off, g_ref = torch.zeros(B, Q, M, L, P, dtype=ct), torch.zeros(B, Q, M, L, P, 2, dtype=ct), torch.zeros(B, Q, L, 4, dtype=ct)
    bi = torch.arange(B)[:, None, None, None].expand(B, Q, M, P)
    mi = torch.arange(M)[None, None, :, None].expand(B, Q, M, P)
    for l in range(L):
        H, W = int(shapes[l, 0]), int(shapes[l, 1])
        x, y = loc[:, :, :, l, :, 0] * W - 0.5, loc[:, :, :, l, :, 1] * H - 0.5
        dx = U32 * (2 * t[:, :, :, l, :, 0].abs() * W + 2 * loc[:, :, :, l, :, 0].abs() * W + x.abs())
        dy = U32 * (2 * t[:, :, :, l, :, 1].abs() * H + 2 * loc[:, :, :, l, :, 1].abs() * H + y.abs())
        vk, lw, lh, inside, idxs, valids = _level_pieces(v, x, y, H, W, int(lsi[l]))
        hh, hw = 1 - lh, 1 - lw
        sens = [dy * hw + dx * hh, dy * lw + dx * hh, dy * hw + dx * lh, dy * lw + dx * lh]
        al = a[:, :, :, l, :]
        moved = sum(sens[k][..., None] * vk[k] for k in range(4))
        out += (al[..., None] * moved).sum(3)
        g_a[:, :, :, l, :] = (tg * moved).sum(-1)
        for k in range(4):
            gv.index_put_((bi, idxs[k], mi), (al * sens[k] * valids[k].to(ct))[..., None] * tg, accumulate=True)
        sv = (tg * sum(vk)).sum(-1) * inside.to(ct)
        gx, gy = W * al * sv * dy, H * al * sv * dx
        g_off[:, :, :, l, :, 0] = gx * ref[:, :, None, l, None, 2].abs() * 0.5 / P
        g_off[:, :, :, l, :, 1] = gy * ref[:, :, None, l, None, 3].abs() * 0.5 / P
        parts = torch.stack((gx, gy, gx * off[:, :, :, l, :, 0].abs() * 0.5 / P, gy * off[:, :, :, l, :, 1].abs() * 0.5 / P), -1)
        g_ref[:, :, l, :] = parts.sum((2, 3))
    if mask is not None:
        gv = gv.masked_fill(mask[:, :, None, None], 0.0)
    af, gf = a.reshape(B, Q, M, L * P), g_a.reshape(B, Q, M, L * P)
    g_lg = af * (gf + (af * gf).sum(-1, keepdim=True))
    return dict(out=out.reshape(B, Q, M * D), grad_value=gv, grad_offsets=g_off, grad_logits=g_lg, grad_ref=g_ref)


# mistake -> the tensors that depend on it, and whether a case can show it
MISTAKES = {
    "off_no_P": (("grad_offsets",), lambda c: c["P"] > 1 and c["Q"] >= 5),            # Q = 3: every box has size 0, every d off is 0
    "no_half": (("grad_ref",), lambda c: True),                                          # (and grad_offsets wherever a box has a size)
    "wh_swapped": (("grad_offsets",), lambda c: c["Q"] >= 5 or c["Q"] == 1),
    "softmax_no_dot": (("grad_logits",), lambda c: len(c["levels"]) * c["P"] > 1),
    "ref_not_over_heads": (("grad_ref",), lambda c: c["M"] > 1),
    "neighbour_level_start": (("grad_value",), lambda c: len(c["levels"]) > 1),
    "mask_ignored_gv": (("grad_value",), lambda c: c["mask"] is not None),
    "lh_hh_swapped": (("grad_value",), lambda c: c["levels"][0][0] > 1),
}


def ref64(inp):
    """float64: the autograd restatement's out and gradients, with the magnitudes M_<tensor>."""
    def build():
        r = dict(restate(inp, torch.float64))
        for t, m in evaluate(inp, torch.float64, absolute=True).items():
            r["M_" + t] = m
        if inp["case"].get("near_edge"):
            for t, e in coordinate_terms(inp).items():
                r["E_" + t] = e
        return r
    return cached(("ref64", inp["case"]["name"], inp["dtype"]), build)


def ratios(got, r64):
    """{tensor: largest (|got - ref64| - half_ulp_f32(|ref64|))+ / (2^-24 M_e)} of a float32 result; an element whose magnitude is 0 must be exact.
    The f32 result's own rounding is taken off because the bound pays for it in its second term; it only matters where an element underflows
    (a weight of e^-60 times a gradient lands below the smallest subnormal, and 2^-24 M_e with it)."""
    out = {}
    for t in TENSORS:
        d = (got[t].double().reshape(r64[t].shape) - r64[t]).abs()
        d = (d - half_ulp(r64[t], F32)).clamp_min(0.0)
        m = r64["M_" + t] * U32
        pos = m > 0
        assert bool((d[~pos] == 0).all()), t
        out[t] = float((d[pos] / m[pos]).max()) if bool(pos.any()) else 0.0
    return out


def measure_constants():
    def build():
        worst = {t: 0.0 for t in TENSORS}
        for dtype in DTYPES:
            for case in CASES:
                inp = make_case(case, dtype)
                r = ratios(restate(inp, torch.float32), ref64(inp))
                worst = {t: max(worst[t], r[t]) for t in TENSORS}
        return worst
    return cached(("C",), build)


def bound(r64, tensor, dtype, consts=None):
    C = (consts or C_MEASURED)[tensor]
    b = 4.0 * C * U32 * r64["M_" + tensor] + half_ulp(r64[tensor], OUT_DTYPE.get(tensor, dtype))
    if "E_" + tensor in r64:                                # the near-edge case only: the coordinate term, with the same margin
        b = b + 4.0 * r64["E_" + tensor]
    return b


def check(got, r64, dtype, label, worst=None, consts=None):
    """Every element of every tensor in `got` against its bound; prints the worst |diff| / bound per tensor before it asserts. -> failures."""
    fails = []
    for t in got:
        b = bound(r64, t, dtype, consts)
        d = (got[t].double().cpu().reshape(r64[t].shape) - r64[t]).abs()
        bad = ~(d <= b)
        pos = b > 0
        w = float((d[pos] / b[pos]).max()) if bool(pos.any()) else 0.0
        if worst is not None:
            worst[t] = max(worst.get(t, 0.0), w)
        print(f"{label} {t}: worst |diff| / bound {w:.4f}, {int(bad.sum())} of {bad.numel()} outside")
        if bool(bad.any()):
            fails.append((t, w, int(bad.sum())))
    return fails
