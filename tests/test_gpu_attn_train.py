"""GPU: csrc/attention_train.hip (lwdetr_attn_train_forward / _backward) and lwdetr_amd.ops.attention on the cases of attn_train_ref.py, in
f32 / f16 / bf16. Every element of o, dq, dk, dv is checked against the float64 evaluation under
    |got - ref64| <= 4 C[T][tensor] u_T M_e + half_ulp_T(|ref64_e|)
(attn_train_ref.py: the magnitudes M_e, and C[T][tensor] = the measured worst ratio of the reference formulation in dtype T on these cases), lse
under its own bound. Forward and backward of every case are pinned to one launch form through lwdetr_attn_train_path_counts; outputs sit in
sentinel-filled buffers (guard rows before and after, row stride > heads hd, unused slots and heads of the packed gradient buffer) and everything
outside the op's elements must come back bit-identical; a second call must give the same bits.

C[T][tensor] as measured on the CPU (attn_train_ref.C_MEASURED, in units of u_T = 2^-24 / 2^-11 / 2^-8; profiles/r13a_attn_train_worst_ratios.txt
also lists the kernel's worst |diff| / bound per launch form):
              o        dq       dk       dv
    f32     37.41    3.642    1.770    16.56
    f16     2.018    0.4162   0.3005   1.589
    bf16    2.496    0.4439   0.4858   3.649

The autograd tests (FusedAttentionFunction behind an nn.Linear, the Attention module, patch_vit_attention, fused_attention) use the rule of
tests/test_gpu_train_tail.py per tensor: max |native - fp64| <= max(4 x max |torch_T - fp64|, 2 ulp_T of the tensor's largest magnitude).
"""
import pytest
import torch
import torch.nn as nn

import attn_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}                      # launch form -> {tensor: largest |diff| / bound seen}


@pytest.fixture(scope="module")
def A():
    from lwdetr_amd import _native
    from lwdetr_amd.ops import attention
    _native.lib()
    return attention


def launches(fn):
    from lwdetr_amd import _native
    before = _native.attn_train_path_counts()
    out = fn()
    after = _native.attn_train_path_counts()
    return out, {k: after[k] - before[k] for k in after if after[k] != before[k]}


def expected_forms(N, hd, dtype):
    dt = R.NAME[dtype]
    fwd = {f"attn_train_fwd_{dt}_hd{hd}": 1}
    if N <= R.ONE_LAUNCH_MAX_N:
        return fwd, {f"attn_train_bwd_one_{dt}_hd{hd}": 1}
    return fwd, {f"attn_train_bwd_dot_{dt}": 1, f"attn_train_bwd_dkdv_{dt}_hd{hd}": 1, f"attn_train_bwd_dq_{dt}_hd{hd}": 1}


def packed(B, N, heads, hd, dtype, slots, eh=0, ed=0):
    """A sentinel-filled (B, guard + N + guard, slots, heads + eh, hd + ed) buffer."""
    return torch.full((B, N + 2 * R.GUARD, slots, heads + eh, hd + ed), R.SENT, dtype=dtype, device=DEV)


def heads_view(buf, slot, N, heads, hd):
    return buf[:, R.GUARD:R.GUARD + N, slot, :heads, :hd].permute(0, 2, 1, 3)          # (B, heads, N, hd)


def rows(B, N, C, pad, dtype):
    """A sentinel-filled (guard + B N + guard, C + pad) matrix and its (B, N, C) view."""
    buf = torch.full((B * N + 2 * R.GUARD, C + pad), R.SENT, dtype=dtype, device=DEV)
    return buf, buf[R.GUARD:R.GUARD + B * N, :C].unflatten(0, (B, N))


def untouched(buf, *views):
    """Everything of buf outside `views` (views of buf) is still the sentinel, bit for bit."""
    c = buf.clone()
    for v in views:
        v_in_c = torch.as_strided(c, v.shape, v.stride(), v.storage_offset() - buf.storage_offset())
        v_in_c.fill_(R.SENT)
    return bool((c == torch.full((), R.SENT, dtype=buf.dtype, device=buf.device)).all())


def layout(inp):
    """Device operands of one case: inputs as views of packed buffers, outputs as views of sentinel buffers."""
    case, dtype = inp["case"], inp["dtype"]
    B, heads, N, hd = case["B"], case["heads"], case["N"], case["hd"]
    C = heads * hd
    if case["distinct"]:                        # every operand with strides of its own
        ins = [packed(B, N, heads, hd, dtype, 3), packed(B, N, heads, hd, dtype, 2, eh=1), packed(B, N, heads, hd, dtype, 4, ed=16)]
        q, k, v = heads_view(ins[0], 0, N, heads, hd), heads_view(ins[1], 1, N, heads, hd), heads_view(ins[2], 2, N, heads, hd)
        gb = [packed(B, N, heads, hd, dtype, 1), packed(B, N, heads, hd, dtype, 2, eh=1), packed(B, N, heads, hd, dtype, 3, ed=16)]
        dq, dk, dv = heads_view(gb[0], 0, N, heads, hd), heads_view(gb[1], 1, N, heads, hd), heads_view(gb[2], 2, N, heads, hd)
        gviews = [[dq], [dk], [dv]]
    else:                                       # q, k, v = qkv[:, :, i]; the gradients in one buffer with an unused slot and an unused head
        ins = [packed(B, N, heads, hd, dtype, 3)]
        q, k, v = (heads_view(ins[0], i, N, heads, hd) for i in range(3))
        gb = [packed(B, N, heads, hd, dtype, 4, eh=1)]
        dq, dk, dv = heads_view(gb[0], 0, N, heads, hd), heads_view(gb[0], 1, N, heads, hd), heads_view(gb[0], 3, N, heads, hd)
        gviews = [[dq, dk, dv]]
    q.copy_(inp["q"]); k.copy_(inp["k"]); v.copy_(inp["v"])
    obuf, o = rows(B, N, C, 16, dtype)
    dobuf, do = rows(B, N, C, 32, dtype)
    do.copy_(inp["do"])
    return dict(q=q, k=k, v=v, o=o, obuf=obuf, do=do, dq=dq, dk=dk, dv=dv, gb=gb, gviews=gviews)


CASE_PARAMS = [pytest.param(c, dt, id=f"{c['name']}-{R.NAME[dt]}") for dt in R.DTYPES for c in R.cases_for(dt)]


@pytest.mark.parametrize("case,dtype", CASE_PARAMS)
def test_every_element_against_fp64(A, case, dtype):
    inp = R.make_case(case, dtype)
    r64 = R.ref64(inp)
    L = layout(inp)
    N, hd, scale = case["N"], case["hd"], inp["scale"]
    want_f, want_b = expected_forms(N, hd, dtype)
    (o, lse), forms = launches(lambda: A.attn_train_forward(L["q"], L["k"], L["v"], scale, out=L["o"]))
    assert forms == want_f and o is L["o"]
    _, forms = launches(lambda: A.attn_train_backward(L["q"], L["k"], L["v"], o, lse, scale, L["do"], L["dq"], L["dk"], L["dv"]))
    assert forms == want_b
    torch.cuda.synchronize()
    got = dict(o=L["o"], lse=lse, dq=L["dq"], dk=L["dk"], dv=L["dv"])
    first = {t: g.clone() for t, g in got.items()}
    label = f"{case['name']} {R.NAME[dtype]}"
    wf, wb = WORST.setdefault(next(iter(want_f)), {}), WORST.setdefault(" + ".join(sorted(want_b)), {})
    fails = R.check(dict(o=got["o"], lse=lse), r64, dtype, label, wf) + R.check({t: got[t] for t in ("dq", "dk", "dv")}, r64, dtype, label, wb)
    assert not fails, fails
    assert untouched(L["obuf"], L["o"]), "forward wrote outside o"
    for buf, views in zip(L["gb"], L["gviews"]):
        assert untouched(buf, *views), "backward wrote outside dq / dk / dv"
    # a second call on the same inputs, into buffers with another fill: every output element is written, and to the same bits
    L["obuf"].fill_(-7.0)
    for buf in L["gb"]:
        buf.fill_(-7.0)
    o2, lse2 = A.attn_train_forward(L["q"], L["k"], L["v"], scale, out=L["o"])
    A.attn_train_backward(L["q"], L["k"], L["v"], o2, lse2, scale, L["do"], L["dq"], L["dk"], L["dv"])
    again = dict(o=L["o"], lse=lse2, dq=L["dq"], dk=L["dk"], dv=L["dv"])
    for t in first:
        assert torch.equal(first[t], again[t]), f"{t} differs between two calls"


def test_every_launch_form_is_served_by_a_case_and_print_worst(A):
    from lwdetr_amd import _native
    names = set(_native.attn_train_path_counts())
    assert len(names) == 39
    served = set()
    for dt in R.DTYPES:
        for c in R.cases_for(dt):
            f, b = expected_forms(c["N"], c["hd"], dt)
            served |= set(f) | set(b)
    assert served == names, sorted(names ^ served)
    for form in sorted(WORST):
        print(form, {t: round(w, 4) for t, w in WORST[form].items()})


def test_refusals_on_the_device(A):
    q = torch.zeros(1, 2, 8, 16, device=DEV)
    with pytest.raises(RuntimeError, match="dtype"):
        A.fused_attention(q.double(), q.double(), q.double(), 0.25)
    with pytest.raises(RuntimeError, match="head size"):
        A.fused_attention(q[..., :8], q[..., :8], q[..., :8], 0.25)
    with pytest.raises(RuntimeError, match="scale"):
        A.fused_attention(q, q, q, float("nan"))
    with pytest.raises(RuntimeError, match="head size"):
        A.FusedAttentionFunction.apply(torch.zeros(1, 8, 3, 2, 24, device=DEV), 0.2)


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


def window_problem(dtype, seed=0):
    """16 windows, N = 49, C = 192, 12 heads: a Linear whose output is wider than 3 C, so that qkv is a non-contiguous view of it."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(16, 49, 192, generator=g)
    w = torch.randn(3 * 192 + 64, 192, generator=g) * 192 ** -0.5
    b = torch.randn(3 * 192 + 64, generator=g) * 0.1
    t = torch.randn(16, 49, 192, generator=g)
    return x, w, b, t


def run_linear(x, w, b, t, dtype, core):
    x = x.to(DEV, dtype).requires_grad_(True)
    lin = nn.Linear(192, 3 * 192 + 64).to(DEV, dtype)
    with torch.no_grad():
        lin.weight.copy_(w); lin.bias.copy_(b)
    y = lin(x)[..., :3 * 192]
    assert not y.is_contiguous()
    qkv = y.reshape(16, 49, 3, 12, 16)
    out = core(qkv)
    (out * t.to(DEV, dtype)).sum().backward()
    return out.detach(), x.grad, lin.weight.grad, lin.bias.grad


def formulation_core(qkv):
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    return R.formulation(q, k, v, 0.25)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
def test_function_behind_a_linear(A, dtype):
    x, w, b, t = window_problem(dtype)
    x, w, b, t = (a.to(dtype).float() for a in (x, w, b, t))           # the same stored numbers in every evaluation
    (native, forms) = launches(lambda: run_linear(x, w, b, t, dtype, lambda qkv: A.FusedAttentionFunction.apply(qkv, 0.25)))
    dt = R.NAME[dtype]
    assert forms == {f"attn_train_fwd_{dt}_hd16": 1, f"attn_train_bwd_one_{dt}_hd16": 1}
    same = run_linear(x, w, b, t, dtype, formulation_core)
    r64 = run_linear(x, w, b, t, torch.float64, formulation_core)
    for name, n, s, r in zip(("out", "grad x", "grad weight", "grad bias"), native, same, r64):
        tail_rule(n, s, r, dtype, f"{dt} {name}")


class StandIn(nn.Module):
    """What patch_vit_attention looks for: qkv, proj, num_heads, scale; its own forward is the materialised formulation."""

    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads, self.scale = num_heads, (dim // num_heads) ** -0.5
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)

    def forward(self, x, mask=None):
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4).unbind(0)
        w = (q * self.scale) @ k.transpose(-2, -1)
        if mask is not None:
            w = w.masked_fill(mask.reshape(B, 1, 1, N).expand_as(w), float("-inf"))
        return self.proj((w.softmax(dim=-1) @ v).transpose(1, 2).reshape(B, N, C))


def test_attention_module_and_patch(A):
    from lwdetr_amd.ops import Attention, patch_vit_attention
    torch.manual_seed(3)
    keys = {False: ["qkv.weight", "qkv.bias", "proj.weight", "proj.bias"], True: ["qkv.weight", "q_bias", "v_bias", "proj.weight", "proj.bias"]}
    x = torch.randn(4, 49, 192, device=DEV)
    for cae in (False, True):
        m = Attention(192, 12, qkv_bias=True, use_cae=cae).to(DEV)
        assert sorted(m.state_dict()) == sorted(keys[cae])
        sd = {k: torch.randn_like(v) * 0.05 for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        bias = torch.cat((sd["q_bias"], torch.zeros_like(sd["v_bias"]), sd["v_bias"])) if cae else sd["qkv.bias"]
        ref = StandIn(192, 12).to(DEV)
        ref.load_state_dict({"qkv.weight": sd["qkv.weight"], "qkv.bias": bias, "proj.weight": sd["proj.weight"], "proj.bias": sd["proj.bias"]})
        with torch.no_grad():
            tail_rule(m(x), ref(x), ref.double()(x.double()), torch.float32, f"Attention use_cae={cae}")
    model = nn.Sequential(StandIn(192, 12), nn.Identity(), StandIn(192, 12)).to(DEV)
    with torch.no_grad():
        before = model(x)
        r64 = model.double()(x.double())
        model.float()
        assert patch_vit_attention(model) == 2
        (after, forms) = launches(lambda: model(x))
        assert forms == {"attn_train_fwd_f32_hd16": 2}
        tail_rule(after, before, r64, torch.float32, "patched stand-in")
        mask = torch.zeros(4, 49, dtype=torch.bool, device=DEV)
        mask[:, 40:] = True
        assert torch.equal(model[0](x, mask), StandIn.forward(model[0], x, mask))


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=lambda d: R.NAME[d])
def test_fused_attention_separate_operands(A, dtype):
    """The decoder's self-attention shape: 300 queries per group, hd 32, three separate tensors; q is a strided view."""
    g = torch.Generator().manual_seed(11)
    q, k, v, t = (torch.randn(2, 8, 300, 32, generator=g).to(dtype) for _ in range(4))
    t = t.permute(0, 2, 1, 3).reshape(2, 300, 256)

    def run(dt, core):
        ops = [a.to(DEV, dt).requires_grad_(True) for a in (q.float(), k.float(), v.float())]
        wide = torch.zeros(2, 8, 300, 64, device=DEV, dtype=dt)
        wide[..., :32] = ops[0].detach()
        qv = wide[..., :32].requires_grad_(True) if core is A.fused_attention else ops[0]
        out = core(qv, ops[1], ops[2], 32 ** -0.5)
        (out * t.to(DEV, dt)).sum().backward()
        return out.detach(), qv.grad, ops[1].grad, ops[2].grad
    native, forms = launches(lambda: run(dtype, A.fused_attention))
    dt = R.NAME[dtype]
    assert forms == {f"attn_train_fwd_{dt}_hd32": 1, f"attn_train_bwd_dot_{dt}": 1, f"attn_train_bwd_dkdv_{dt}_hd32": 1, f"attn_train_bwd_dq_{dt}_hd32": 1}
    same, r64 = run(dtype, R.formulation), run(torch.float64, R.formulation)
    for name, n, s, r in zip(("out", "dq", "dk", "dv"), native, same, r64):
        tail_rule(n, s, r, dtype, f"fused_attention {dt} {name}")


def test_memory_stays_far_below_one_weight_tensor(A):
    """B = 1, 12 heads, N = 1600, hd 16, f32: one materialised weight tensor is 123 MB; the op's own tensors total under 12 MB."""
    torch.manual_seed(0)
    qkv = torch.randn(1, 1600, 3, 12, 16, device=DEV, requires_grad=True)
    t = torch.randn(1, 1600, 192, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = A.FusedAttentionFunction.apply(qkv, 0.25)
    out.backward(t)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak over forward + backward: {peak / 2 ** 20:.2f} MiB above the inputs")
    assert qkv.grad.shape == qkv.shape
    assert peak < 64e6
