"""CPU-only checks of the bound of tests/test_gpu_attention_fp64.py, on exactly that module's cases (its case builders are imported; no GPU is
touched):
  * not too tight: an independent evaluation of the kernels' scheme - f32 scores and accumulators summed in another order (48-key steps, plain
    matrix products), the lazy rescale at 2^8, P rounded to the storage type, the denominator from the rounded P or (attn_win at hd 32) from the
    unrounded one, the result rounded to the storage type - stays inside the bound on every element of every case;
  * not too loose: each of twelve planted mistakes, made in a float64 evaluation of the same scheme (so that the mistake is its only deviation),
    leaves the bound in every case it applies to; the test prints how many elements leave. The planted runs take the operands with the rows that no
    sequence may use at +-30000 (the second fill of the GPU tests), so a key let in by mistake carries weight."""
import math

import pytest
import torch

from tests import test_gpu_attention_fp64 as G
from tests.test_gpu_attention_fp64 import F16, BF16, F32, NAME
from tests.test_gpu_rowops import SENT


def emulate(case, fam, lowp=True, mut=(), fill=0.0, step=48):
    """softmax(Q K^T) V as the kernels organise it, (B, spi, keys, heads hd) float64. lowp: f32 arithmetic, P and the result rounded to T;
    otherwise float64 throughout. mut: planted mistakes."""
    T, hd, g = case["T"], case["hd"], case["g"]
    ft = torch.float32 if lowp else torch.float64
    n, ss, sl = g["keys"], g["sub_stride"], g["sub_len"]
    ext = 4 if "neighbour_keys" in mut else 0
    qs, k, v = G.operands(case, fill)
    q = G.seq_views(g, qs).to(ft)
    k, v = G.seq_views(g, k, ext).to(ft), G.seq_views(g, v, ext).to(ft)
    j = torch.arange(n + ext)
    real = torch.cat([case["real"], torch.ones(ext, dtype=torch.bool)])
    last_real = int(case["real"].nonzero().max())
    if "drop_last_key" in mut:                      # the mask off by one at the sequence end
        real[last_real] = False
    if "hole_off_by_one" in mut:                    # ... and at a hole
        real = real & ((j % ss) < sl - 1)
    if "query_clamp" in mut:                        # the query clamp off by one: min(q, last - 1)
        q = q[..., torch.arange(n).clamp(max=n - 2), :]
    vidx = j.clone()
    if "vt_run_shifted" in mut:                     # the last 4-key run of the V^T tile shifted by one key
        vidx[n - 4:n] = n - 4 + (torch.arange(4) + 1) % 4
    if "shift4_missing" in mut:                     # a clamped run (nkeys - 8) used as it was loaded
        vidx[n - 4:n] = torch.arange(n - 8, n - 4)
    if "slice_permuted" in mut:                     # a 16-key slice's V^T permuted against its P
        vidx[16:32] = torch.arange(31, 15, -1)
    v = v[..., vidx, :]
    unrounded = fam == "win" and hd == 32
    O = torch.zeros(q.shape, dtype=ft)
    l = torch.zeros(q.shape[:-1] + (1,), dtype=ft)
    m = None
    for k0 in range(0, n + ext, step):
        k1 = min(n + ext, k0 + step)
        s = q @ k[..., k0:k1, :].transpose(-1, -2)
        if "log2e_dropped" in mut:
            s = s / G.LOG2E
        s = s.masked_fill(~real[k0:k1], -math.inf)
        rm = s.amax(-1, keepdim=True)
        if m is None:
            m = rm
        else:
            mn = torch.where(rm - m > 8, rm, m)     # lazy: the reference moves only for a score 2^8 above it
            alpha = torch.exp2(m - mn)
            O = O * alpha
            if "rescale_not_on_l" not in mut:
                l = l * alpha
            m = mn
        p = torch.exp2(s - m)
        pr = p.to(T).to(ft) if lowp else p
        lp = p if unrounded else pr
        if "denom_missing_step" in mut:             # the denominator misses the 32-key step 32 .. 63
            lp = lp * ~((j[k0:k1] >= 32) & (j[k0:k1] < 64))
        l = l + lp.sum(-1, keepdim=True)
        O = O + pr @ v[..., k0:k1, :]
    y = O / l
    B, H, W = g["B"], g["heads"], g["spi"]
    if "head_image_swapped" in mut:                 # (image, head) -> (head, image) in the output index
        src = torch.tensor([(p_ % H) * B + p_ // H for p_ in range(B * H)])
        y = y.reshape(B * H, W, n, hd)[src].reshape(B, H, W, n, hd)
    y = y.permute(0, 2, 3, 1, 4).reshape(B, W, n, H * hd)
    if lowp:
        y = y.to(T)
    y = y.double()
    if "pad_rows_not_written" in mut:
        y[:, :, ~case["real"]] = SENT
    return y


CASES = G.all_cases()


@pytest.mark.parametrize("label,key,fam", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_independent_f32_emulation_is_inside_the_bound(label, key, fam):
    case = G.case_of(*key)
    y, bnd = G.reference(case, fam)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(bnd).all())
    for fill in (0.0, G.BIG):
        err = (emulate(case, fam, fill=fill) - y).abs()
        ratio = float((err / bnd).max())
        assert bool((err <= bnd).all()), f"{label}: {int((~(err <= bnd)).sum())} elements outside, worst err/bound {ratio:.3f}"
    assert ratio > 1e-3 or case["T"] == F32, f"{label}: the bound is orders of magnitude above the emulation's error"
    exact = emulate(case, fam, lowp=False, step=32)
    assert float(((exact - y).abs() / bnd).max()) < 1e-3, f"{label}: the float64 evaluation of the scheme is not the reference"


def _applies(mut, case):
    g, real, n = case["g"], case["real"], case["g"]["keys"]
    return {
        "drop_last_key": True, "vt_run_shifted": bool(real[n - 4:].any()), "query_clamp": True, "log2e_dropped": True, "neighbour_keys": True,
        "hole_off_by_one": g["sub_len"] < g["sub_stride"], "pad_rows_not_written": g["sub_len"] < g["sub_stride"],
        "shift4_missing": n % 8 == 4 and n >= 12 and bool(real[n - 4:].any()),
        "slice_permuted": n >= 32 and bool(real[16:32].any()),
        "denom_missing_step": n >= 64 and bool(real[32:64].any()),
        "rescale_not_on_l": any(r[3] == "over8" for r in case["rows"]),
        "head_image_swapped": g["B"] >= 2 and g["heads"] >= 2,
    }[mut]


MISTAKES = ["drop_last_key", "hole_off_by_one", "vt_run_shifted", "shift4_missing", "slice_permuted", "denom_missing_step", "rescale_not_on_l",
            "head_image_swapped", "pad_rows_not_written", "query_clamp", "log2e_dropped", "neighbour_keys"]
# one case of every family, type and head size; bf16 (the widest bound) wherever a mechanism has one case only
MISTAKE_CASES = [((BF16, 16, "k12"), "wave"), ((BF16, 32, "dec300"), "wave"), ((F16, 64, "holes192"), "wave"), ((BF16, 32, "k44"), "wave"),
                 ((F32, 32, "k516"), "wave"), ((BF16, 16, "w100_97"), "win"), ((BF16, 32, "w28_25"), "win"), ((BF16, 64, "r708"), "ring"),
                 ((F16, 16, "rwin228"), "ring"), ((BF16, 32, "rmask512"), "ring"), ((BF16, 32, "r320"), "ring")]


@pytest.mark.parametrize("mut", MISTAKES)
def test_planted_mistake_leaves_the_bound(mut):
    seen = 0
    for key, fam in MISTAKE_CASES:
        case = G.case_of(*key)
        if not _applies(mut, case):
            continue
        y, bnd = G.reference(case, fam)
        err = (emulate(case, fam, lowp=False, mut=(mut,), fill=G.BIG, step=32) - y).abs()
        outside = int((~(err <= bnd)).sum())
        print(f"{mut}: {key[2]} {NAME[key[0]]} hd{key[1]}: {outside} of {err.numel()} elements outside the bound")
        assert outside > 0, f"{mut} stays inside the bound on {key}: the inputs put too little weight on that edge"
        seen += 1
    assert seen >= 2, f"{mut}: applies to {seen} case(s) only"
