"""GPU: the fused drop-path residual (csrc/drop_path.hip through lwdetr_amd.ops.drop_path) against the torch formulation and float64.

Shapes (groups, rows per group, C): (3, 5, 20) everything odd - element accesses for the 16-bit and mixed pairs (20 is no multiple of 8), five
16-byte chunks a row in f32; (4, 16, 192) 16-byte accesses; (33, 100, 384) 207 workgroups of partials; (2, 7, 2048) the upper end of C (one row
lane per workgroup; in f32 two trips over the 512 chunks of a row); (3, 6, 40) cut out of rows of 44 elements, a leading dimension above C.
Three more for the paths those leave out: (3, 5, 21) element accesses in every pair; (2, 3, 301) element accesses with more channels than
threads (two trips, the second partial); (2, 3, 760) 190 chunks in f32 - one row lane and idle threads - and 95 in the 16-bit pairs.
Masks: mixed, all kept, all dropped.

float32: ``out`` and ``grad_y`` are torch.equal to ``drop_path_residual_torch`` on the device (the object is built without contraction, so
every product and sum rounds where torch's separate kernels round); ``grad_x`` is the cotangent itself; ``grad_gamma`` against float64 within
(R + 2) 2^-24 sum_r |g t y| per channel, R rows: two roundings per term and an f32 accumulation of R terms in some fixed order.
The other four dtype pairs against float64 of the same (rounded) inputs: |out - ref| <= u |ref| + 4 * 2^-24 (|x| + |gamma y t|), u the unit
round-off of the output type (2^-11 f16, 2^-8 bf16, 2^-24 f32): three f32 roundings on the way and one to the output; grad_y the same form with
u of y's type. The inputs have magnitudes in [0.25, 2] (gamma [0.5, 1.5]), so an f16 result is either in the normal range or, where x and the
branch cancel, its 2^-25 of subnormal rounding is inside the second term.
"""
import pytest
import torch

from lwdetr_amd import _native as N
from lwdetr_amd.ops import (DropPathResidualFunction, drop_path_residual, drop_path_residual_torch, drop_path_supports)

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 0.25
SHAPES = {"odd_20": (3, 5, 20, 0), "wide_192": (4, 16, 192, 0), "partials_384": (33, 100, 384, 0), "top_2048": (2, 7, 2048, 0),
          "strided_40": (3, 6, 40, 4), "odd_21": (3, 5, 21, 0), "odd_301": (2, 3, 301, 0), "lanes_760": (2, 3, 760, 0)}
PAIRS = {"f32_f32": (torch.float32, torch.float32), "f16_f16": (torch.float16, torch.float16), "bf16_bf16": (torch.bfloat16, torch.bfloat16),
         "f32_f16": (torch.float32, torch.float16), "f32_bf16": (torch.float32, torch.bfloat16)}
UNIT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
_CASES = {}


def _signed(gen, shape, lo, hi):
    mag = torch.rand(shape, generator=gen) * (hi - lo) + lo
    return mag * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)


def _keep(kind, groups, gen):
    if kind == "mixed":
        k = torch.rand(groups, generator=gen) < 0.6
        k[0], k[-1] = True, False
        return k
    return torch.full((groups,), kind == "all_kept")


def case(shape, mask, pair):
    """One set of inputs per (shape, mask, dtype pair), made once: float32 values rounded to the pair's types, on the device. x, y and the
    cotangent g are views with the shape's leading dimension."""
    key = (shape, mask, pair)
    if key not in _CASES:
        groups, rpg, c, pad = SHAPES[shape]
        dx, dy = PAIRS[pair]
        gen = torch.Generator().manual_seed(list(SHAPES).index(shape) + 7)
        wide = lambda dt: _signed(gen, (groups, rpg, c + pad), 0.25, 2.0).to(dt).to(DEV)[..., :c]
        _CASES[key] = dict(x=wide(dx), y=wide(dy), g=wide(dx), gamma=_signed(gen, (c,), 0.5, 1.5).to(DEV), keep=_keep(mask, groups, gen).to(DEV))
    return _CASES[key]


def _run(fn, cs, gamma=True, **need):
    x, y = cs["x"].detach().requires_grad_(need.get("x", True)), cs["y"].detach().requires_grad_(need.get("y", True))
    gm = cs["gamma"].detach().requires_grad_(need.get("gamma", True)) if gamma else None
    out = fn(x, y, gm, cs["keep"], P)
    out.backward(cs["g"])
    return out.detach(), x.grad, y.grad, None if gm is None else gm.grad


def _f64(cs, gamma=True):
    x, y, g = cs["x"].double(), cs["y"].double(), cs["g"].double()
    gm = cs["gamma"].double() if gamma else torch.ones(x.shape[2], dtype=torch.float64, device=DEV)
    # the scale the kernel is handed: keep / (1 - p) formed in the branch's dtype as timm forms it (f32 beside the f32 gamma, y's without one)
    t = cs["keep"].to(torch.float32 if gamma else cs["y"].dtype).div_(1 - P).double().view(-1, 1, 1)
    return x, gm * y * t, g * t * gm, (g * t * y).abs().sum((0, 1)), (g * t * y).sum((0, 1))


@pytest.mark.parametrize("mask", ["mixed", "all_kept", "all_dropped"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_float32_equals_the_torch_formulation_bit_for_bit(shape, mask):
    cs = case(shape, mask, "f32_f32")
    assert drop_path_supports(cs["x"], cs["y"], cs["gamma"])
    if SHAPES[shape][3]:
        assert not cs["x"].is_contiguous() and cs["x"].stride(1) > cs["x"].shape[2]
    want, wx, wy, _ = _run(drop_path_residual_torch, cs)
    got, gx, gy, gg = _run(drop_path_residual, cs)
    assert got.is_contiguous() and torch.equal(got, want)
    assert torch.equal(gy, wy) and torch.equal(gx, cs["g"]) and torch.equal(gx, wx)
    _, _, _, mag, ref = _f64(cs)
    rows = SHAPES[shape][0] * SHAPES[shape][1]
    err, bound = (gg.double() - ref).abs(), (rows + 2) * 2.0 ** -24 * mag
    print(f"{shape} {mask}: grad_gamma worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    if mask == "all_dropped":
        assert torch.equal(got, cs["x"]) and not gy.any() and not gg.any()


@pytest.mark.parametrize("pair", [p for p in PAIRS if p != "f32_f32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_other_dtype_pairs_against_float64(shape, pair):
    cs = case(shape, "mixed", pair)
    dx, dy = PAIRS[pair]
    got, gx, gy, gg = _run(drop_path_residual, cs)
    assert got.dtype == dx and gy.dtype == dy and gg.dtype == torch.float32 and torch.equal(gx, cs["g"])
    x, branch, ref_gy, mag, ref_gg = _f64(cs)
    ref = x + branch
    slack = 4 * 2.0 ** -24
    err, bound = (got.double() - ref).abs(), UNIT[dx] * ref.abs() + slack * (x.abs() + branch.abs())
    assert bool((err <= bound).all()), float((err / bound).max())
    err_y, bound_y = (gy.double() - ref_gy).abs(), (UNIT[dy] + slack) * ref_gy.abs()
    assert bool((err_y <= bound_y).all()), float((err_y / bound_y.clamp_min(1e-300)).max())
    rows = SHAPES[shape][0] * SHAPES[shape][1]
    assert bool(((gg.double() - ref_gg).abs() <= (rows + 2) * 2.0 ** -24 * mag).all())
    print(f"{shape} {pair}: out worst error / bound {float((err / bound).max()):.3f}, grad_y {float((err_y / bound_y.clamp_min(1e-300)).max()):.3f}")


@pytest.mark.parametrize("pair", ["f32_f32", "f32_bf16"])
def test_a_second_backward_gives_the_first_ones_bits(pair):
    cs = case("partials_384", "mixed", pair)
    x, y, gm = cs["x"].detach().requires_grad_(), cs["y"].detach().requires_grad_(), cs["gamma"].detach().requires_grad_()
    out = drop_path_residual(x, y, gm, cs["keep"], P)
    first = torch.autograd.grad(out, (y, gm), cs["g"], retain_graph=True)
    second = torch.autograd.grad(out, (y, gm), cs["g"])
    again = drop_path_residual(x, y, gm, cs["keep"], P)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]) and torch.equal(out, again)


@pytest.mark.parametrize("shape", ["odd_20", "wide_192", "strided_40"])
def test_without_gamma(shape):
    cs = case(shape, "mixed", "f32_f32")
    want, _, wy, _ = _run(drop_path_residual_torch, cs, gamma=False)
    got, gx, gy, gg = _run(drop_path_residual, cs, gamma=False)
    assert gg is None and torch.equal(got, want) and torch.equal(gy, wy) and torch.equal(gx, cs["g"])
    cs16 = case(shape, "mixed", "f32_f16")
    got, _, gy, _ = _run(drop_path_residual, cs16, gamma=False)
    x, branch, ref_gy, _, _ = _f64(cs16, gamma=False)
    assert bool(((got.double() - (x + branch)).abs() <= 2.0 ** -24 * (x + branch).abs() + 4 * 2.0 ** -24 * (x.abs() + branch.abs())).all())
    assert bool(((gy.double() - ref_gy).abs() <= (2.0 ** -11 + 4 * 2.0 ** -24) * ref_gy.abs()).all())


def _moved(before):
    after = N.drop_path_path_counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


@pytest.mark.parametrize("pair", list(PAIRS))
def test_launch_record_moves_by_one_per_forward_and_one_per_backward(pair):
    cs = case("wide_192", "mixed", pair)
    x, y, gm = cs["x"].detach().requires_grad_(), cs["y"].detach().requires_grad_(), cs["gamma"].detach().requires_grad_()
    before = N.drop_path_path_counts()
    out = drop_path_residual(x, y, gm, cs["keep"], P)
    assert _moved(before) == {f"dp_fwd_{pair}": 1}
    before = N.drop_path_path_counts()
    out.backward(cs["g"])
    assert _moved(before) == {f"dp_bwd_{pair}": 1}
    # needs_input_grad is honoured: with x alone wanting a gradient the backward launches nothing and hands the cotangent through
    x2 = cs["x"].detach().requires_grad_()
    out = drop_path_residual(x2, cs["y"], cs["gamma"], cs["keep"], P)
    before = N.drop_path_path_counts()
    out.backward(cs["g"])
    assert _moved(before) == {} and torch.equal(x2.grad, cs["g"])
    # y alone: one launch, no grad_gamma
    _, _, gy, gg = _run(drop_path_residual, cs, x=False, gamma=False)
    assert gy is not None and gg is None


def test_the_function_refuses_what_the_kernel_does_not_take():
    cs = case("odd_20", "mixed", "f32_f32")
    with pytest.raises(RuntimeError, match="not supported"):
        DropPathResidualFunction.apply(cs["x"].double(), cs["y"].double(), cs["gamma"], cs["keep"], P)
    with pytest.raises(RuntimeError, match="not supported"):
        DropPathResidualFunction.apply(cs["x"].half(), cs["y"], cs["gamma"], cs["keep"], P)
    with pytest.raises(RuntimeError, match="ROCm device"):
        DropPathResidualFunction.apply(cs["x"].cpu(), cs["y"].cpu(), cs["gamma"].cpu(), cs["keep"].cpu(), P)
    wide = torch.zeros(2, 3, 2049, device=DEV)
    assert not drop_path_supports(wide, wide)
    with pytest.raises(RuntimeError, match="range"):
        DropPathResidualFunction.apply(wide, wide, None, torch.ones(2, dtype=torch.bool, device=DEV), P)
    # a 16-bit x beside an f32 gamma promotes to f32 in torch: the dispatch leaves that call to torch
    assert not drop_path_supports(cs["x"].half(), cs["y"].half(), cs["gamma"]) and drop_path_supports(cs["x"].half(), cs["y"].half())
