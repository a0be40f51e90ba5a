"""GPU: csrc/msda_train.hip (lwdetr_msda_train_forward / _backward) and lwdetr_amd.ops.deform_train on the cases of msda_train_ref.py, in
f32 / f16 / bf16. Every element of out, grad_value, grad_offsets, grad_logits and grad_ref is checked against the float64 restatement under
    |got - ref64| <= 4 C[tensor] 2^-24 M_e + half_ulp_T(|ref64_e|)
(msda_train_ref.py: the magnitudes M_e, and C[tensor] = the measured worst ratio of the restatement in float32 on these cases; T of grad_ref
is float32; the near-edge case adds its coordinate term 4 E_e). Forward and backward of every case are pinned to their launch forms through lwdetr_msda_train_path_counts; every output sits
between sentinel guards that must come back bit-identical; a second forward and a second backward must give the same bits - grad_value of
the collision case (257 queries x 3 heads x 2 points aimed at one cell) included.

C[tensor] as measured on the CPU (msda_train_ref.C_MEASURED, units of 2^-24; profiles/r14a_msda_train_worst_ratios.txt lists the kernels' worst
|diff| / bound per dtype and tensor):   out 317.4   grad_value 260.7   grad_offsets 129.8   grad_logits 130.5   grad_ref 38.80

The autograd tests (the Function behind nn.Linears, MSDeformAttnTrain, patch_deformable_attention) use the rule of tests/test_gpu_train_tail.py
per tensor: max |native - fp64| <= max(4 x max |torch_T - fp64|, 2 ulp_T of the tensor's largest magnitude), torch_T being the same restatement
run by torch in dtype T on the device.
"""
import pytest
import torch
import torch.nn as nn

import msda_train_ref as R
from msda_train_helpers import msda_train_served_by

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD_ELEMS = 64
WORST = {}                      # dtype name -> {tensor: largest |diff| / bound seen}


@pytest.fixture(scope="module")
def T():
    from lwdetr_amd import _native
    from lwdetr_amd.ops import deform_train
    _native.lib()
    return deform_train


def guarded(shape, dtype, fill=R.SENT):
    """A sentinel-filled flat buffer and the contiguous view of `shape` in its middle."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD_ELEMS,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD_ELEMS:GUARD_ELEMS + n].view(shape)


def guards_intact(buf, fill=R.SENT):
    f = torch.full((), fill, dtype=buf.dtype, device=DEV)
    return bool((buf[:GUARD_ELEMS] == f).all()) and bool((buf[-GUARD_ELEMS:] == f).all())


def device_operands(T, inp):
    """The case on the device: value / offsets / logits as column views of wider buffers (strided cases) or as separate packed tensors."""
    case, dtype = inp["case"], inp["dtype"]
    B, Q, M, D, P = case["B"], case["Q"], case["M"], case["D"], case["P"]
    S, L = inp["S"], inp["shapes"].shape[0]
    W = M * L * P
    if case["strided"]:
        vbuf = torch.full((B, S, M * D + 16), R.SENT, dtype=dtype, device=DEV)
        value = vbuf[:, :, :M * D].unflatten(2, (M, D))
        obuf = torch.full((B, Q, 2 * W + 8), R.SENT, dtype=dtype, device=DEV)
        lbuf = torch.full((B, Q, W + 24), R.SENT, dtype=dtype, device=DEV)
        off, lg = obuf[:, :, :2 * W], lbuf[:, :, 8:8 + W]
    else:
        value = torch.empty(B, S, M, D, dtype=dtype, device=DEV)
        off, lg = torch.empty(B, Q, 2 * W, dtype=dtype, device=DEV), torch.empty(B, Q, W, dtype=dtype, device=DEV)
    value.copy_(inp["value"]); off.copy_(inp["off"].reshape(B, Q, 2 * W)); lg.copy_(inp["lg"].reshape(B, Q, W))
    mask = None if inp["mask"] is None else inp["mask"].to(DEV)
    ops = T._Operands(value, inp["shapes"].to(DEV), inp["lsi"].to(DEV), off, lg, inp["ref"].to(DEV), mask)
    # the operands are taken as they are: no copy was made
    assert ops.value.data_ptr() == value.data_ptr() and ops.off.data_ptr() == off.data_ptr() and ops.lg.data_ptr() == lg.data_ptr()
    if case["strided"]:
        assert (ops.ld_v, ops.ld_off, ops.ld_lg) == (M * D + 16, 2 * W + 8, W + 24)
    return ops


def forms(case, dtype):
    dt, f = R.NAME[dtype], R.form(case)
    e = 1 if case["D"] <= 16 else 2 if case["D"] <= 32 else 4
    return {f"msda_train_fwd_{dt}_{f}": 1}, {f"msda_train_bwd_q_{dt}_{f}": 1, f"msda_train_bwd_v_{dt}_e{e}": 1}


CASE_PARAMS = [pytest.param(c, dt, id=f"{c['name']}-{R.NAME[dt]}") for dt in R.DTYPES for c in R.ALL_CASES]


@pytest.mark.parametrize("case,dtype", CASE_PARAMS)
def test_every_element_against_fp64(T, case, dtype):
    inp = R.make_case(case, dtype)
    r64 = R.ref64(inp)
    ops = device_operands(T, inp)
    B, Q, M, D, P = case["B"], case["Q"], case["M"], case["D"], case["P"]
    S, L = inp["S"], inp["shapes"].shape[0]
    shapes = dict(out=(B, Q, M * D), grad_value=(B, S, M, D), grad_offsets=(B * Q, M * L * P * 2), grad_logits=(B * Q, M * L * P), grad_ref=(B, Q, L, 4))
    bufs = {t: guarded(shapes[t], R.OUT_DTYPE.get(t, dtype)) for t in R.TENSORS}
    go = inp["go"].to(DEV)
    want_f, want_b = forms(case, dtype)

    def run():
        T.msda_train_forward(ops, out=bufs["out"][1])
        T.msda_train_backward(ops, go, *(bufs[t][1] for t in R.TENSORS[1:]))

    with msda_train_served_by({**want_f, **want_b}):
        run()
    first = {t: bufs[t][1].clone() for t in R.TENSORS}
    label = f"{case['name']} {R.NAME[dtype]}"
    fails = R.check(first, r64, dtype, label, WORST.setdefault(R.NAME[dtype], {}))
    assert not fails, fails
    for t in R.TENSORS:
        assert guards_intact(bufs[t][0]), f"{t}: wrote outside its tensor"
    # a second call on the same inputs, into buffers with another fill: every output element is written, and to the same bits
    for t in R.TENSORS:
        bufs[t][0].fill_(-7.0)
    run()
    torch.cuda.synchronize()
    for t in R.TENSORS:
        assert torch.equal(first[t], bufs[t][1]), f"{label}: {t} differs between two calls" + (" (the collision case)" if case["collide"] else "")
        assert guards_intact(bufs[t][0], -7.0), t


def test_refusals_on_the_device(T):
    from lwdetr_amd.ops import FusedMSDeformAttnFunction as F
    shapes, lsi = torch.tensor([[3, 5]], device=DEV), torch.tensor([0], device=DEV)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    with pytest.raises(RuntimeError, match="outside the kernel's range"):
        F.apply(z(1, 15, 2, 8, dt=torch.float64), shapes, lsi, z(1, 4, 8, dt=torch.float64), z(1, 4, 4, dt=torch.float64), z(1, 4, 1, 4))
    with pytest.raises(RuntimeError, match="outside the kernel's range"):
        F.apply(z(1, 15, 2, 12), shapes, lsi, z(1, 4, 8), z(1, 4, 4), z(1, 4, 1, 4))
    with pytest.raises(RuntimeError, match="share a dtype"):
        F.apply(z(1, 15, 2, 8), shapes, lsi, z(1, 4, 8, dt=torch.bfloat16), z(1, 4, 4), z(1, 4, 1, 4))
    with pytest.raises(RuntimeError, match="inconsistent shapes"):
        F.apply(z(1, 15, 2, 8), shapes, lsi, z(1, 4, 6), z(1, 4, 4), z(1, 4, 1, 4))


# ---------------------------------------------------------------------------------------------------------------------- through autograd
def ulp(x, dtype):
    return 2.0 * float(R.half_ulp(torch.tensor(float(x), dtype=torch.float64), dtype))


def tail_rule(native, torch_T, ref64, dtype, label):
    """max |native - fp64| <= max(4 x max |torch_T - fp64|, 2 ulp_T of the tensor's largest magnitude); prints before it asserts."""
    dn = float((native.double() - ref64).abs().max())
    dt = float((torch_T.double() - ref64).abs().max())
    bnd = max(4.0 * dt, 2.0 * ulp(ref64.abs().max(), dtype))
    print(f"{label}: |native - fp64| {dn:.3e}, |torch - fp64| {dt:.3e}, bound {bnd:.3e}")
    assert dn <= bnd, label


LEVELS = [(5, 5)]
B_, Q_, C_, M_, D_, P_ = 2, 65, 64, 4, 16, 2


def linear_problem():
    """Three Linears whose outputs are wider than the operands, so that value, offsets and logits are non-contiguous column views."""
    g = torch.Generator().manual_seed(21)
    S, W = sum(h * w for h, w in LEVELS), M_ * len(LEVELS) * P_
    x = torch.randn(B_, Q_, C_, generator=g)
    mem = torch.randn(B_, S, C_, generator=g)
    ws = [torch.randn(n, C_, generator=g) * C_ ** -0.5 for n in (M_ * D_ + 16, 2 * W + 8, W + 8)]
    bs = [torch.randn(n, generator=g) * 0.1 for n in (M_ * D_ + 16, 2 * W + 8, W + 8)]
    ref = torch.cat((torch.rand(B_, Q_, 1, 2, generator=g), torch.rand(B_, Q_, 1, 2, generator=g) * 0.6 + 0.1), -1)
    t = torch.randn(B_, Q_, M_ * D_, generator=g)
    mask = torch.zeros(B_, S, dtype=torch.bool)
    mask[1, ::6] = True
    return x, mem, ws, bs, ref, t, mask


def run_linears(prob, dtype, core):
    x, mem, ws, bs, ref, t, mask = prob
    S, W = mem.shape[1], M_ * len(LEVELS) * P_
    x, mem = x.to(DEV, dtype).requires_grad_(True), mem.to(DEV, dtype).requires_grad_(True)
    ref = ref.to(DEV, dtype).requires_grad_(True)
    lins = [nn.Linear(C_, w.shape[0]).to(DEV, dtype) for w in ws]
    with torch.no_grad():
        for lin, w, b in zip(lins, ws, bs):
            lin.weight.copy_(w); lin.bias.copy_(b)
    value = lins[0](mem)[..., :M_ * D_].unflatten(2, (M_, D_))
    off, lg = lins[1](x)[..., :2 * W], lins[2](x)[..., :W]
    assert not value.is_contiguous() and not off.is_contiguous() and not lg.is_contiguous()
    shapes = torch.tensor(LEVELS, dtype=torch.int64, device=DEV)
    lsi = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = core(value, shapes, lsi, off, lg, ref, mask.to(DEV))
    (out * t.to(DEV, dtype)).sum().backward()
    return [out.detach(), x.grad, mem.grad, ref.grad] + [p.grad for lin in lins for p in (lin.weight, lin.bias)]


def restatement_core(value, shapes, lsi, off, lg, ref, mask):
    B, Q = off.shape[:2]
    return R.core(value, off.reshape(B, Q, M_, len(LEVELS), P_, 2), lg.reshape(B, Q, M_, len(LEVELS) * P_), ref, mask, shapes.cpu(), lsi.cpu(), P_)


NAMES = ("out", "grad x", "grad memory", "grad reference boxes", "grad value weight", "grad value bias", "grad offsets weight", "grad offsets bias",
         "grad logits weight", "grad logits bias")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
def test_function_behind_linears_with_non_contiguous_outputs(T, dtype):
    x, mem, ws, bs, ref, t, mask = linear_problem()
    rd = lambda a: a.to(dtype).float()                                         # the same stored numbers in every evaluation
    prob = (rd(x), rd(mem), [rd(w) for w in ws], [rd(b) for b in bs], rd(ref), rd(t), mask)
    dt = R.NAME[dtype]
    with msda_train_served_by({f"msda_train_fwd_{dt}_l1p2": 1, f"msda_train_bwd_q_{dt}_l1p2": 1, f"msda_train_bwd_v_{dt}_e1": 1}):
        native = run_linears(prob, dtype, T.FusedMSDeformAttnFunction.apply)
    same = run_linears(prob, dtype, restatement_core)
    r64 = run_linears(prob, torch.float64, restatement_core)
    assert native[3].dtype == dtype                                            # the boxes' gradient comes back in the boxes' dtype
    for name, n, s, r in zip(NAMES, native, same, r64):
        tail_rule(n, s, r, dtype, f"{dt} {name}")


class StandIn(nn.Module):
    """What patch_deformable_attention looks for: the four Linears and n_heads / n_levels / n_points. Its own forward is the reference's:
    locations and softmax in torch, then MSDeformAttnFunction (ms_deform_attn.py:113-143)."""

    def __init__(self, d_model, n_levels, n_heads, n_points):
        super().__init__()
        self.n_heads, self.n_levels, self.n_points = n_heads, n_levels, n_points
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj, self.output_proj = nn.Linear(d_model, d_model), nn.Linear(d_model, d_model)

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index, input_padding_mask=None):
        from lwdetr_amd.ops import MSDeformAttnFunction
        N, Lq, _ = query.shape
        _, S, C = input_flatten.shape
        M, L, P = self.n_heads, self.n_levels, self.n_points
        value = self.value_proj(input_flatten)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None], float(0))
        off = self.sampling_offsets(query).view(N, Lq, M, L, P, 2)
        aw = self.attention_weights(query).view(N, Lq, M, L * P)
        loc = reference_points[:, :, None, :, None, :2] + off / P * reference_points[:, :, None, :, None, 2:] * 0.5
        aw = aw.softmax(-1).view(N, Lq, M, L, P)
        out = MSDeformAttnFunction.apply(value.view(N, S, M, C // M), input_spatial_shapes, input_level_start_index, loc, aw, 64)
        return self.output_proj(out)


def module_inputs(d_model, levels, B=2, Q=33, seed=4):
    g = torch.Generator().manual_seed(seed)
    S, L = sum(h * w for h, w in levels), len(levels)
    query, mem = torch.randn(B, Q, d_model, generator=g), torch.randn(B, S, d_model, generator=g)
    ref = torch.cat((torch.rand(B, Q, 1, 2, generator=g), torch.rand(B, Q, 1, 2, generator=g) * 0.5 + 0.05), -1).expand(B, Q, L, 4).contiguous()
    shapes = torch.tensor(levels, dtype=torch.int64)
    lsi = torch.cat((shapes.new_zeros(1), (shapes[:, 0] * shapes[:, 1]).cumsum(0)[:-1]))
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[1, -7:] = True
    return [a.to(DEV) for a in (query, ref, mem, shapes, lsi, mask)]


def randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name != "sampling_offsets.bias":                            # the directional grid of the reference's initialisation stays
                p.copy_(torch.randn(p.shape, generator=g) * (0.3 if "sampling_offsets" in name or "attention_weights" in name else 0.06))


def test_train_module_loads_the_inference_modules_state(T):
    from lwdetr_amd.ops import MSDeformAttn, MSDeformAttnTrain
    inference = MSDeformAttn(256, 1, 16, 2)
    randomise(inference, 8)
    inference = inference.to(DEV)
    train = MSDeformAttnTrain(256, 1, 16, 2).to(DEV)
    assert sorted(train.state_dict()) == sorted(inference.state_dict())
    train.load_state_dict(inference.state_dict(), strict=True)
    args = module_inputs(256, [(5, 5)])
    with torch.no_grad():
        have_inf = inference(*args)
    with msda_train_served_by({"msda_train_fwd_f32_l1p2": 1}):
        have = train(*args)
    assert have.requires_grad
    d64 = MSDeformAttnTrain(256, 1, 16, 2).to(DEV).double()
    d64.load_state_dict({k: v.double() for k, v in inference.state_dict().items()}, strict=True)
    r64 = d64(*[a.double() if a.is_floating_point() else a for a in args]).detach()       # float64: the torch formulation + MSDeformAttnFunction
    # "equal within the bound": the per-element bound of msda_train_ref.py needs M_e, which is not available through the two Linears in front of
    # the core and the one behind it, so this is the tensor-wide rule of the autograd tests - looser per element than the cases' bound - with the
    # inference module (fused GEMMs + the inference kernel) as the float32 yardstick
    tail_rule(have.detach(), have_inf, r64, torch.float32, "MSDeformAttnTrain vs the inference module")
    with pytest.raises(ValueError, match="4-coordinate"):
        train(args[0], args[1][..., :2].contiguous(), *args[2:])


def grads_of(model, args, dtype=None, autocast=None):
    args = list(args)
    args[1] = args[1].detach().clone().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    if autocast is not None:
        with torch.autocast("cuda", dtype=autocast):
            out = model(*args)
    else:
        out = model(*args)
    out.float().square().sum().backward()
    return out.detach(), [args[1].grad] + [p.grad for _, p in sorted(model.named_parameters())]


def test_patch_on_a_stand_in_and_bf16_autocast_training_step(T):
    from lwdetr_amd.ops import patch_deformable_attention
    model = nn.Sequential()
    model.add_module("attn", StandIn(256, 1, 16, 2))
    model.add_module("other", nn.Linear(4, 4))
    randomise(model.attn, 9)
    model = model.to(DEV)
    args = module_inputs(256, [(5, 5)], seed=6)
    keys = sorted(model.state_dict())
    before, gb = grads_of(model.attn, args)                                                  # the reference's formulation, f32
    m64 = StandIn(256, 1, 16, 2).to(DEV).double()
    m64.load_state_dict({k: v.double() for k, v in model.attn.state_dict().items()})
    r64, g64 = grads_of(m64, [a.double() if a.is_floating_point() else a for a in args])
    assert patch_deformable_attention(model) == 1 and sorted(model.state_dict()) == keys
    with msda_train_served_by({"msda_train_fwd_f32_l1p2": 1, "msda_train_bwd_q_f32_l1p2": 1, "msda_train_bwd_v_f32_e1": 1}):
        after, ga = grads_of(model.attn, args)
    tail_rule(after, before, r64, torch.float32, "patched stand-in, out")
    names = ["reference boxes"] + [n for n, _ in sorted(model.attn.named_parameters())]
    for n, a, b, r in zip(names, ga, gb, g64):
        tail_rule(a, b, r, torch.float32, f"patched stand-in, grad {n}")
    # mixed precision: on the operator alone this raised in ms_deform_attn_backward (float32 / float64 only)
    with msda_train_served_by({"msda_train_fwd_bf16_l1p2": 1, "msda_train_bwd_q_bf16_l1p2": 1, "msda_train_bwd_v_bf16_e1": 1}):
        out, grads = grads_of(model.attn, args, autocast=torch.bfloat16)
    assert out.dtype == torch.bfloat16
    assert len(grads) == 9
    for n, gr in zip(names, grads):
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, n
    # and they are the gradients. Those of the value / output / attention-weight Linears are continuous in the sampling locations: bf16 rounds
    # each Linear's output, the core's output and the gradients between them to 2^-9 relative, half a dozen roundings in a chain - a few per
    # cent of the tensor's largest element, where a wrong gradient is off by all of it. The gradients of the boxes and of sampling_offsets
    # are NOT continuous: bf16 offsets move a sample by ~0.003 pixel, a handful of the 2112 samples change their cell, and each of those changes
    # d out / d loc by its whole size (0.30 of the largest box gradient was seen); they are printed, not bounded.
    for n, gr, r in zip(names, grads, g64):
        rel = float((gr.double() - r).abs().max() / r.abs().max())
        print(f"bf16 autocast grad {n}: max |diff| / max |fp64| {rel:.3e}")
        if n != "reference boxes" and not n.startswith("sampling_offsets"):
            assert rel < 0.1, n


@pytest.mark.parametrize("cfg", [(128, 4, 8, 4, True), (96, 2, 8, 2, False)], ids=["L4_P4_d16", "head_width_12_falls_back"])
def test_configurations_at_and_outside_the_kernels_range(T, cfg):
    """n_levels = n_points = 4 (the reference module's defaults) has L P = 16 and runs on the fused kernel's run-time form; a head width of 12
    is outside its range, takes the torch formulation + MSDeformAttnFunction and still matches."""
    from lwdetr_amd.ops import MSDeformAttnTrain
    from lwdetr_amd import _native
    d_model, L, M, P, fused = cfg
    levels = [(6, 6), (4, 4), (3, 3), (2, 2)][:L]
    train = MSDeformAttnTrain(d_model, L, M, P)
    randomise(train, 12)
    train = train.to(DEV)
    args = module_inputs(d_model, levels, seed=13)
    stand = StandIn(d_model, L, M, P).to(DEV)
    stand.load_state_dict(train.state_dict(), strict=True)
    m64 = StandIn(d_model, L, M, P).to(DEV).double()
    m64.load_state_dict({k: v.double() for k, v in train.state_dict().items()})
    r64, g64 = grads_of(m64, [a.double() if a.is_floating_point() else a for a in args])
    want, gw = grads_of(stand, args)
    if fused:
        with msda_train_served_by({"msda_train_fwd_f32_gen": 1, "msda_train_bwd_q_f32_gen": 1, "msda_train_bwd_v_f32_e1": 1}):
            have, gh = grads_of(train, args)
    else:
        before = _native.msda_path_counts()
        with msda_train_served_by({}):
            have, gh = grads_of(train, args)
        assert _native.msda_path_counts()["msda_backward_f32"] == before["msda_backward_f32"] + 1
    tail_rule(have, want, r64, torch.float32, "out")
    names = ["reference boxes"] + [n for n, _ in sorted(train.named_parameters())]
    for n, a, b, r in zip(names, gh, gw, g64):
        tail_rule(a, b, r, torch.float32, f"grad {n}")


def test_expanded_and_overlapping_operands_and_an_unaligned_grad_out(T):
    """Offsets and logits that are legal tensors but do not hold B Q rows - one row expanded over the queries (row stride 0), rows that overlap
    (row stride below the width) - get a packed copy and give the bits of the materialised tensors; their gradients come back through autograd's
    own reduction. A contiguous grad_out that starts 4 bytes into a buffer is copied, not refused."""
    from lwdetr_amd.ops import FusedMSDeformAttnFunction as F
    B, Q, M, D, L, P = 2, 5, 2, 8, 1, 2
    W = M * L * P
    g = torch.Generator().manual_seed(3)
    value = torch.randn(B, 15, M, D, generator=g).to(DEV).requires_grad_(True)
    shapes, lsi = torch.tensor([[3, 5]], device=DEV), torch.tensor([0], device=DEV)
    ref = torch.cat((torch.rand(B, Q, L, 2, generator=g), torch.rand(B, Q, L, 2, generator=g) * 0.5 + 0.1), -1).to(DEV)
    off_row = torch.randn(1, 1, 2 * W, generator=g).to(DEV).requires_grad_(True)
    lg_store = torch.randn(B * Q * 2 + W, generator=g).to(DEV).requires_grad_(True)
    gbuf = torch.randn(B * Q * M * D + 1, generator=g).to(DEV)
    gout = gbuf[1:].view(B, Q, M * D)
    assert gout.is_contiguous() and gout.data_ptr() % 16 == 4

    def views():
        return off_row.expand(B, Q, 2 * W), torch.as_strided(lg_store, (B, Q, W), (Q * 2, 2, 1))       # row strides 0 and 2 < W

    off, lg = views()
    ops = T._Operands(value.detach(), shapes, lsi, off.detach(), lg.detach(), ref)
    for t, src, width in ((ops.off, off, 2 * W), (ops.lg, lg, W)):
        assert t.data_ptr() != src.data_ptr() and t.is_contiguous() and t.untyped_storage().nbytes() >= B * Q * width * 4
    assert (ops.ld_off, ops.ld_lg) == (2 * W, W)

    def run(materialise):
        for x in (value, off_row, lg_store):
            x.grad = None
        off, lg = views()
        if materialise:
            off, lg = off.contiguous(), lg.contiguous()
        out = F.apply(value, shapes, lsi, off, lg, ref)
        out.backward(gout)
        return out.detach(), value.grad, off_row.grad, lg_store.grad

    for name, a, b in zip(("out", "grad value", "grad offsets row", "grad logits store"), run(False), run(True)):
        assert torch.equal(a, b), name
    inp = dict(value=value.detach().cpu(), off=views()[0].detach().cpu().reshape(B, Q, M, L, P, 2), lg=views()[1].detach().cpu().reshape(B, Q, M, L * P),
               ref=ref.cpu(), go=gout.cpu(), mask=None, shapes=shapes.cpu(), lsi=lsi.cpu(), S=15, dtype=R.F32,
               case=dict(name="expanded_operands", B=B, Q=Q, M=M, D=D, levels=[(3, 5)], P=P))
    r64 = R.ref64(inp)
    out = run(False)[0]
    d = (out.double().cpu() - r64["out"]).abs()
    print("expanded operands, out: worst |diff| / M_e in units of 2^-24", float((d / (r64["M_out"] * R.U32).clamp_min(1e-300)).max()))
    assert bool((d <= 1e-4 * r64["M_out"] + 1e-6).all())        # the right rows were read (a wrong row is off by all of M_e); accuracy is the cases' business


def test_every_launch_form_is_served_by_a_case_and_was_launched(T):
    """The last test of the file. Every instantiation name is served by a case, and every one was launched in this process: by the tests above
    in a whole run, and by the serving case right here for any name that is still at zero (this test selected alone, or run first)."""
    from lwdetr_amd import _native
    assert len(_native.msda_train_path_counts()) == 27
    served = set()
    for dt in R.DTYPES:
        for c in R.CASES:
            f, b = forms(c, dt)
            served |= set(f) | set(b)
            if any(_native.msda_train_path_counts()[n] == 0 for n in list(f) + list(b)):
                inp = R.make_case(c, dt)
                ops = device_operands(T, inp)
                with msda_train_served_by({**f, **b}):
                    T.msda_train_forward(ops)
                    T.msda_train_backward(ops, inp["go"].to(DEV))
    counts = _native.msda_train_path_counts()
    assert served == set(counts), sorted(set(counts) ^ served)
    assert all(n > 0 for n in counts.values()), {k: n for k, n in counts.items() if n == 0}
    for dt in sorted(WORST):
        print("WORST", dt, " ".join(f"{t} {w:.4f}" for t, w in WORST[dt].items()))
