"""GPU: the training-step tail (lwdetr_amd.train: NativeAdamW, ModelEma, clip_grad_norm_ over lwdetr_mt_sumsq / _norm_finish / _step) on the
edge set of train_tail_ref.py against the fp64 restatement of the reference's three steps, per tensor:
    max |native - fp64| <= max(4 x max |torch_f32 - fp64|, 2 ulp_f32 of the tensor's largest magnitude),
total norm to 1e-6 relative, int64 EMA entries and EMA_SET exact, a parameter without a gradient bit-identical. One test runs the tiny model's
real parameter set (12 M elements). Every test prints its worst error / bound ratio before it asserts."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import train_tail_ref as R
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def T():
    from lwdetr_amd import _native, train
    _native.lib()
    assert train.CHUNK == R.CHUNK
    return train


def launches(fn):
    from lwdetr_amd import _native
    before = _native.mt_launch_counts()
    fn()
    after = _native.mt_launch_counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


@pytest.mark.parametrize("max_norm,ema", [(R.MAX_NORM, True), (0.0, True), (R.MAX_NORM, False), (0.0, False)])
def test_fused_step_on_the_edge_set(T, max_norm, ema):
    case = R.make_case()
    r64, r32 = R.references(max_norm, ema)
    got, model, opt, _ = R.run_native(case, DEV, "fused", max_norm, ema)
    for s in range(R.STEPS):
        if max_norm > 0:
            rel = abs(got[s]["norm"] - r64[s]["norm"]) / r64[s]["norm"]
            print(f"step {s}: total_norm {got[s]['norm']:.9g} fp64 {r64[s]['norm']:.12g} rel {rel:.2e}")
            assert rel <= 1e-6
        for g, g0 in zip(got[s]["grads"], case["grads"][s]):                       # the fused form does not rewrite the gradients
            assert (g is None and g0 is None) or torch.equal(g, g0)
        assert torch.equal(got[s]["p"][R.NO_GRAD], case["params"][R.NO_GRAD]) and got[s]["m"][R.NO_GRAD] is None
    worst = R.check_snapshots(got, r64, r32, label=f"fused max_norm={max_norm} ema={ema}")
    print(f"fused max_norm={max_norm} ema={ema}: worst error / bound = {worst:.3f}")
    assert model.plist()[R.NO_GRAD] not in opt.state
    assert [float(opt.state[p]["step"]) for i, p in enumerate(model.plist()) if i != R.NO_GRAD] == [3.0] * (len(R.SIZES) - 1)
    assert opt.last_total_norm.dim() == 0 and opt.last_total_norm.is_cuda


def test_standalone_clip_stock_adamw_standalone_ema(T):
    case = R.make_case()
    r64, r32 = R.references(R.MAX_NORM, True)
    got, _, _, _ = R.run_native(case, DEV, "standalone", R.MAX_NORM, True)
    for s in range(R.STEPS):
        assert abs(got[s]["norm"] - r64[s]["norm"]) <= 1e-6 * r64[s]["norm"]
        for g, g64 in zip(got[s]["grads"], r64[s]["grads"]):
            if g64 is not None:
                assert float((g.double() - g64).abs().max()) <= R.ulp32(float(g64.abs().max()))
    worst = R.check_snapshots(got, r64, r32, label="standalone")
    print(f"standalone: worst error / bound = {worst:.3f}")


def test_ema_set_is_an_exact_copy(T):
    case = R.make_case()
    model = R.EdgeModel(case, DEV)
    ema = T.ModelEma(model, decay=R.DECAY)
    model.load_step(case, 1, grads=False)
    with torch.no_grad():
        for p in model.plist():
            p.mul_(1.5).add_(0.25)
    assert launches(lambda: ema.set(model)) == {"mt_step": 1}
    for a, b in zip(ema.module.state_dict().values(), model.state_dict().values()):
        assert a.dtype == b.dtype and torch.equal(a, b) and a.data_ptr() != b.data_ptr()
    assert launches(lambda: ema.update(model)) == {"mt_step": 1}


def test_two_runs_from_the_same_state_are_bit_identical(T):
    case = R.make_case()
    a, _, _, _ = R.run_native(case, DEV, "fused", R.MAX_NORM, True)
    b, _, _, _ = R.run_native(case, DEV, "fused", R.MAX_NORM, True)
    for x, y in zip(a, b):
        assert x["norm"] == y["norm"]
        for k in ("p", "m", "v", "ema"):
            for u, w in zip(x[k], y[k]):
                assert (u is None and w is None) or torch.equal(u, w), k


def test_host_form_and_device_compute_the_same_bits(T):
    """The host form is the kernels' per-element code with contraction off on both sides: what the CPU tests check is what runs here."""
    case = R.make_case()
    a, _, _, _ = R.run_native(case, DEV, "fused", R.MAX_NORM, True)
    b, _, _, _ = R.run_native(case, "cpu", "fused", R.MAX_NORM, True)
    for x, y in zip(a, b):
        assert x["norm"] == y["norm"]
        for k in ("p", "m", "v", "ema"):
            for u, w in zip(x[k], y[k]):
                assert (u is None and w is None) or torch.equal(u, w), k


def test_lr_changed_through_param_groups_takes_effect_in_the_next_step(T):
    case = R.make_case()
    base, _, _, _ = R.run_native(case, DEV, "fused", 0.0, False, steps=2)

    def zero_lr(s, model, opt):
        if s == 1:
            for g in opt.param_groups:
                g["lr"] = 0.0
    got, _, _, _ = R.run_native(case, DEV, "fused", 0.0, False, steps=2, hook=zero_lr)
    for i, (a, b, p1) in enumerate(zip(got[1]["p"], base[1]["p"], got[0]["p"])):
        if i != R.NO_GRAD:
            assert torch.equal(a, p1) and not torch.equal(a, b), i
    for a, b in zip(got[1]["m"], base[1]["m"]):
        assert (a is None and b is None) or torch.equal(a, b)


def test_all_zero_gradients(T):
    case = R.make_case()
    zero = dict(case, grads=[[None if g is None else torch.zeros_like(g) for g in gs] for gs in case["grads"]])
    got, _, opt, _ = R.run_native(zero, DEV, "fused", R.MAX_NORM, False, steps=1)
    assert got[0]["norm"] == 0.0 and float(opt._tables.norm_clip[1]) == 1.0
    for i, (p, p0) in enumerate(zip(got[0]["p"], case["params"])):
        want = p0 if i == R.NO_GRAD else p0 * np.float32(1 - R.lr_of(i) * R.wd_of(i))
        assert torch.equal(p, want), i                                             # the parameters move by weight decay only


def test_one_nan_gradient_reaches_the_norm_and_every_parameter(T):
    case = R.make_case()
    bad = dict(case, grads=[[None if g is None else g.clone() for g in gs] for gs in case["grads"]])
    bad["grads"][0][11][17] = float("nan")
    got, _, opt, _ = R.run_native(bad, DEV, "fused", R.MAX_NORM, False, steps=1)     # returns normally
    assert np.isnan(got[0]["norm"]) and bool(torch.isnan(opt.last_total_norm))
    assert all(bool(torch.isnan(p).all()) for i, p in enumerate(got[0]["p"]) if i != R.NO_GRAD)      # as torch: the NaN coefficient scales every gradient
    assert torch.equal(got[0]["p"][R.NO_GRAD], case["params"][R.NO_GRAD])


def test_launch_counts_of_a_fused_step(T):
    case = R.make_case()
    for max_norm, want in ((R.MAX_NORM, {"mt_sumsq": 1, "mt_norm_finish": 1, "mt_step": 1}), (0.0, {"mt_step": 1})):
        model = R.EdgeModel(case, DEV)
        ema = T.ModelEma(model, decay=R.DECAY)
        opt = T.NativeAdamW(R.groups_for(model.plist()), lr=1e-4, betas=R.BETAS, eps=R.EPS, max_norm=max_norm, ema=ema)
        for s in range(2):
            model.load_step(case, s)

            def one():
                opt.step()
                ema.update(model)                                                   # the optimizer's launch covered it
            assert launches(one) == want, (max_norm, s)
        torch.cuda.synchronize()


def _reference_step(model, shadow, order, groups, grads, max_norm, decay):
    """The reference sequence with torch's own classes on ``model`` (any float dtype): clip, AdamW over one group per parameter, the EMA loop."""
    named = dict(model.named_parameters())
    for n in order:
        named[n].grad = grads[n].to(named[n].dtype)
    torch.nn.utils.clip_grad_norm_([named[n] for n in order], max_norm)
    opt = torch.optim.AdamW([{"params": [named[n]], "lr": groups[n][0], "weight_decay": groups[n][1]} for n in order], lr=1e-4, betas=R.BETAS,
                            eps=R.EPS, foreach=False)
    opt.step()
    with torch.no_grad():
        for ev, mv in zip(shadow.state_dict().values(), model.state_dict().values()):
            ev.copy_(decay * ev + (1. - decay) * mv)
    return opt


def test_tiny_model_parameter_set_one_fused_step(T):
    import lwdetr_amd
    fx = json.load(open(os.path.join(GOLDEN, "train_tail_param_groups.json")))
    args = lwdetr_amd.get_args("tiny")
    for k, v in fx["args"].items():
        setattr(args, k, v)
    model, _, _ = lwdetr_amd.build_model(args)
    model = model.to(DEV)
    groups, order = fx["tiny"], list(fx["tiny"])
    gen = torch.Generator(device=DEV).manual_seed(11)
    named = dict(model.named_parameters())
    assert set(order) == {n for n, p in named.items() if p.requires_grad}
    with torch.no_grad():
        for b in model.buffers():                                                  # the step counters of the BatchNorms, as after some training
            if b.dtype == torch.int64:
                b.fill_(4000)
    grads = {n: torch.randn(named[n].shape, generator=gen, device=DEV) * 1e-3 for n in order}
    m32, m64 = copy.deepcopy(model), copy.deepcopy(model).double()
    s32, s64 = copy.deepcopy(m32).eval(), copy.deepcopy(m64).eval()
    for s in (s32, s64):
        with torch.no_grad():
            for b in s.buffers():
                if b.dtype == torch.int64:
                    b.fill_(3990)
    o32 = _reference_step(m32, s32, order, groups, grads, R.MAX_NORM, R.DECAY)
    o64 = _reference_step(m64, s64, order, groups, grads, R.MAX_NORM, R.DECAY)
    ema = T.ModelEma(model, decay=R.DECAY)
    with torch.no_grad():
        for b in ema.module.buffers():
            if b.dtype == torch.int64:
                b.fill_(3990)
    opt = T.NativeAdamW(T.get_param_dict(args, model), lr=args.lr, betas=R.BETAS, eps=R.EPS, weight_decay=args.weight_decay, max_norm=R.MAX_NORM,
                        ema=ema)
    assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [tuple(groups[n]) for n in order]
    for n in order:
        named[n].grad = grads[n].clone()
    assert launches(opt.step) == {"mt_sumsq": 1, "mt_norm_finish": 1, "mt_step": 1}
    ema.update(model)
    n64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    rel = abs(float(opt.last_total_norm) - n64) / n64
    print(f"tiny: {sum(p.numel() for p in named.values())} elements in {len(order)} parameters, total_norm rel error {rel:.2e}")
    assert rel <= 1e-6
    worst = 0.0
    p32, p64 = dict(m32.named_parameters()), dict(m64.named_parameters())

    def check(what, a, b64, c32):
        nonlocal worst
        if b64.dtype == torch.int64:
            assert torch.equal(a, b64) and torch.equal(c32, b64), what
            return
        err, bound = float((a.double() - b64).abs().max()), R.tensor_bound(b64, c32)
        worst = max(worst, err / bound)
        assert err <= bound, f"{what}: |native - fp64| = {err:.3e} > bound {bound:.3e}"
    for n in order:
        check(f"p {n}", named[n].detach(), p64[n].detach(), p32[n].detach())
        for k in ("exp_avg", "exp_avg_sq"):
            check(f"{k} {n}", opt.state[named[n]][k], o64.state[p64[n]][k], o32.state[p32[n]][k])
        assert float(opt.state[named[n]]["step"]) == 1.0
        assert torch.equal(named[n].grad, grads[n])
    for (n, a), b64, c32 in zip(ema.module.state_dict().items(), s64.state_dict().values(), s32.state_dict().values()):
        check(f"ema {n}", a, b64, c32)
    print(f"tiny: worst error / bound = {worst:.3f}")
