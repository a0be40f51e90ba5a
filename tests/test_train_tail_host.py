"""CPU: the training-step tail (lwdetr_amd.train over csrc/optim.hip) through the library's host form - lwdetr_mt_norm_host / lwdetr_mt_step_host,
the per-element functions of the kernels on host arrays - against the fp64 restatement of the reference's three steps, plus the parts that need
no kernel at all: the parameter groups against the reference's, the EMA arithmetic against the reference's ModelEma, torch's state-dict format,
the constructor's refusals and the argument rules of the C entries."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import train_tail_ref as R
from helpers import GOLDEN


@pytest.fixture(scope="module")
def T():
    import __graft_entry__ as ge
    ge.build()
    from lwdetr_amd import train
    assert train.CHUNK == R.CHUNK
    return train


# ---------------------------------------------------------------------------------------------- every flag combination on the edge set
@pytest.mark.parametrize("max_norm,ema", [(R.MAX_NORM, True), (0.0, True), (R.MAX_NORM, False), (0.0, False)])
def test_fused_host_form_on_the_edge_set(T, max_norm, ema):
    """ADAMW | EMA and ADAMW alone, with and without the clip coefficient: p, m, v, ema of every tensor after each of the three steps; the norm;
    the gradients untouched; the parameter without a gradient bit-identical, without state."""
    case = R.make_case()
    r64, r32 = R.references(max_norm, ema)
    got, model, opt, _ = R.run_native(case, "cpu", "fused", max_norm, ema)
    worst = R.check_snapshots(got, r64, r32, label=f"fused host max_norm={max_norm} ema={ema}")
    print(f"worst error / bound = {worst:.3f}")
    for s in range(R.STEPS):
        if max_norm > 0:
            assert abs(got[s]["norm"] - r64[s]["norm"]) <= 1e-6 * r64[s]["norm"]
        for g, g0 in zip(got[s]["grads"], case["grads"][s]):
            assert (g is None and g0 is None) or torch.equal(g, g0)
        assert torch.equal(got[s]["p"][R.NO_GRAD], case["params"][R.NO_GRAD]) and got[s]["m"][R.NO_GRAD] is None
    assert model.plist()[R.NO_GRAD] not in opt.state
    assert [float(opt.state[p]["step"]) for i, p in enumerate(model.plist()) if i != R.NO_GRAD] == [3.0] * (len(R.SIZES) - 1)
    if max_norm > 0:                       # steps 1 and 3 bind, step 2 clamps to 1
        assert r64[0]["norm"] > max_norm and r64[2]["norm"] > max_norm and r64[1]["norm"] < max_norm


def test_standalone_host_forms_on_the_edge_set(T):
    """SCALE_GRADS (clip_grad_norm_) and EMA (ModelEma.update) as calls of their own around a stock torch.optim.AdamW: what the host form writes
    - the norm, the gradients (g * clip_coef to 1 ulp) and the EMA entries under the rule; p, m, v are torch's own here, not the host form's."""
    case = R.make_case()
    r64, r32 = R.references(R.MAX_NORM, True)
    got, _, _, _ = R.run_native(case, "cpu", "standalone", R.MAX_NORM, True)
    worst = R.check_snapshots(got, r64, r32, keys=("ema",), label="standalone host")
    print(f"worst error / bound = {worst:.3f}")
    for s in range(R.STEPS):
        assert abs(got[s]["norm"] - r64[s]["norm"]) <= 1e-6 * r64[s]["norm"]
        for g, g64 in zip(got[s]["grads"], r64[s]["grads"]):
            if g64 is not None:
                assert float((g.double() - g64).abs().max()) <= R.ulp32(float(g64.abs().max()))


def test_ema_set_host_form_is_a_copy(T):
    case = R.make_case()
    model = R.EdgeModel(case, "cpu")
    ema = T.ModelEma(model, decay=R.DECAY)
    assert not ema.module.training and ema.decay == R.DECAY
    model.load_step(case, 1, grads=False)
    with torch.no_grad():
        for p in model.plist():
            p.mul_(1.5).add_(0.25)
    ema.set(model)
    for a, b in zip(ema.module.state_dict().values(), model.state_dict().values()):
        assert a.dtype == b.dtype and torch.equal(a, b) and a.data_ptr() != b.data_ptr()


def test_all_zero_gradients_and_a_nan_gradient_host(T):
    case = R.make_case()
    zero = dict(case, grads=[[None if g is None else torch.zeros_like(g) for g in gs] for gs in case["grads"]])
    got, _, opt, _ = R.run_native(zero, "cpu", "fused", R.MAX_NORM, False, steps=1)
    assert got[0]["norm"] == 0.0 and float(opt._tables.norm_clip[1]) == 1.0
    for i, (p, p0) in enumerate(zip(got[0]["p"], case["params"])):
        want = p0 if i == R.NO_GRAD else p0 * np.float32(1 - R.lr_of(i) * R.wd_of(i))
        assert torch.equal(p, want), i
    bad = dict(case, grads=[[None if g is None else g.clone() for g in gs] for gs in case["grads"]])
    bad["grads"][0][11][17] = float("nan")
    got, _, _, _ = R.run_native(bad, "cpu", "fused", R.MAX_NORM, False, steps=1)
    assert np.isnan(got[0]["norm"])
    assert all(bool(torch.isnan(p).all()) for i, p in enumerate(got[0]["p"]) if i != R.NO_GRAD)


# ---------------------------------------------------------------------------------------------- parameter groups
@pytest.mark.parametrize("size", ["tiny", "small"])
def test_get_param_dict_matches_the_reference(T, size):
    import lwdetr_amd
    fx = json.load(open(os.path.join(GOLDEN, "train_tail_param_groups.json")))
    args = lwdetr_amd.get_args(size)
    for k, v in fx["args"].items():
        setattr(args, k, v)
    model, _, _ = lwdetr_amd.build_model(args)
    names = {id(p): n for n, p in model.named_parameters()}
    groups = T.get_param_dict(args, model)
    got = {names[id(g["params"])]: (g["lr"], g.get("weight_decay", args.weight_decay)) for g in groups}
    assert len(got) == len(groups) and list(got) == list(fx[size])            # the same names in the same order
    for n, (lr, wd) in fx[size].items():
        assert abs(got[n][0] - lr) <= 1e-12 * abs(lr) and abs(got[n][1] - wd) <= 1e-12 * abs(wd), (n, got[n], lr, wd)
    assert len({lr for lr, _ in got.values()}) > 5 and {wd for _, wd in got.values()} == {0.0, args.weight_decay}
    opt = torch.optim.AdamW(groups, lr=args.lr, weight_decay=args.weight_decay)     # the groups are what torch expects
    assert len(opt.param_groups) == len(fx[size])


# ---------------------------------------------------------------------------------------------- EMA against the reference's ModelEma
def test_model_ema_host_form_matches_the_reference_fixture(T):
    fx = np.load(os.path.join(GOLDEN, "train_tail_ema.npz"), allow_pickle=False)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
    ema = T.ModelEma(model, decay=0.9997)
    names = list(model.state_dict())
    assert "1.num_batches_tracked" in names
    for k in range(4):
        with torch.no_grad():
            for n, t in model.state_dict().items():
                t.copy_(torch.from_numpy(fx[f"model.{k}.{n}"]))
        (ema.set if k == 0 else ema.update)(model)
        for n, t in ema.module.state_dict().items():
            want = torch.from_numpy(fx[f"ema.{k}.{n}"])
            assert t.dtype == want.dtype and torch.equal(t, want), (k, n, t, want)      # the same two roundings per element: the same bits
    assert [int(fx[f"ema.{k}.1.num_batches_tracked"]) for k in range(4)] == [5, 5, 6, 17]
    for e, x, want in ((5, 6, 5), (0, 4000, 1), (-7, -9, -7)):                          # truncation toward zero, as copy_ does it
        m2 = torch.nn.BatchNorm1d(2)
        ema2 = T.ModelEma(m2)
        ema2.module.num_batches_tracked.fill_(e)
        m2.num_batches_tracked.fill_(x)
        ema2.update(m2)
        assert int(ema2.module.num_batches_tracked) == want == int(R.ema_i64(torch.tensor(e), torch.tensor(x)))


# ---------------------------------------------------------------------------------------------- torch's state-dict format
def test_state_dict_round_trip_with_stock_adamw(T):
    case = R.make_case()
    _, model, opt, _ = R.run_native(case, "cpu", "fused", R.MAX_NORM, False, steps=2)
    sd = opt.state_dict()
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in model.plist()]
    stock = torch.optim.AdamW(R.groups_for(ps2), lr=1e-4, betas=R.BETAS, eps=R.EPS, weight_decay=1e-4)
    stock.load_state_dict(copy.deepcopy(sd))            # load_state_dict keeps tensors of the right dtype and device as they are: no aliasing here
    sd2 = stock.state_dict()
    assert sd2["param_groups"] == sd["param_groups"] and sd2["state"].keys() == sd["state"].keys() and R.NO_GRAD not in sd["state"]
    for k, st in sd["state"].items():
        assert set(st) == set(sd2["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and float(st["step"]) == float(sd2["state"][k]["step"]) == 2.0
        for n in ("exp_avg", "exp_avg_sq"):
            assert st[n].shape == sd2["state"][k][n].shape == model.plist()[k].shape and torch.equal(st[n], sd2["state"][k][n])
    # ... and back: a fresh NativeAdamW continues from the stock optimizer's state exactly where the first one would
    model3 = R.EdgeModel(case, "cpu")
    with torch.no_grad():
        for a, b in zip(model3.plist(), model.plist()):
            a.copy_(b)
    opt3 = T.NativeAdamW(R.groups_for(model3.plist()), lr=1e-4, betas=R.BETAS, eps=R.EPS, weight_decay=1e-4, max_norm=R.MAX_NORM, host=True)
    opt3.load_state_dict(copy.deepcopy(sd2))
    for m_, o_ in ((model, opt), (model3, opt3)):
        m_.load_step(case, 2)
        o_.step()
    for a, b in zip(model3.plist(), model.plist()):
        assert torch.equal(a, b)
    assert float(opt3.state[model3.plist()[0]]["step"]) == 3.0
    sched = torch.optim.lr_scheduler.StepLR(opt3, step_size=1, gamma=0.5)          # schedulers see an ordinary optimizer
    opt3.step()
    sched.step()
    assert float(opt3.state[model3.plist()[0]]["step"]) == 4.0 and opt3.param_groups[1]["lr"] == pytest.approx(R.lr_of(1) * 0.5)


def test_lr_change_through_param_groups_takes_effect_host(T):
    case = R.make_case()
    base, _, _, _ = R.run_native(case, "cpu", "fused", 0.0, False, steps=2)

    def halve(s, model, opt):
        if s == 1:
            for g in opt.param_groups:
                g["lr"] = 0.0
    got, _, _, _ = R.run_native(case, "cpu", "fused", 0.0, False, steps=2, hook=halve)
    for i, (a, b, p1) in enumerate(zip(got[1]["p"], base[1]["p"], got[0]["p"])):
        if i != R.NO_GRAD:
            assert torch.equal(a, p1) and not torch.equal(a, b), i                 # lr = 0: no weight decay, no update, in the very next step
    for a, b in zip(got[1]["m"], base[1]["m"]):
        assert (a is None and b is None) or torch.equal(a, b)                      # the moments do not depend on lr


# ---------------------------------------------------------------------------------------------- refusals
def test_constructor_refusals(T):
    p = torch.nn.Parameter(torch.zeros(8))
    ok = dict(lr=1e-4, host=True)
    T.NativeAdamW([p], **ok)
    for bad in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(max_norm=-1.0),
                dict(lr=torch.tensor(1e-4)), dict(ema=object())):
        with pytest.raises(ValueError):
            T.NativeAdamW([p], **dict(ok, **bad))
    with pytest.raises(ValueError, match="GPU"):
        T.NativeAdamW([p], lr=1e-4)                                                # host memory without host=True: there is no quiet CPU path
    for q in (torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float16), torch.zeros(4, 4).t(), torch.zeros(0)):
        with pytest.raises(ValueError):
            T.NativeAdamW([torch.nn.Parameter(q)], **ok)
    opt = T.NativeAdamW([p], **ok)
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (8,))
    with pytest.raises(ValueError, match="sparse"):
        opt.step()
    with pytest.raises(ValueError):
        T.ModelEma(torch.nn.Linear(2, 2), device="cpu")
    with pytest.raises(ValueError):
        T.clip_grad_norm_([p], 0.1, norm_type=1.0)


def test_c_entries_refuse_bad_tables_before_anything_runs(T):
    from lwdetr_amd import _native as N
    l = N.lib()
    x = np.arange(2500, dtype=np.float32)
    e = np.zeros_like(x)
    tb = T._Tables(np.array([2500], dtype=np.int64), N.MT_EMA_F32, "cpu")
    tb.rec["p"], tb.rec["ema"] = x.ctypes.data, e.ctypes.data
    h = N.MtHyper()
    args = lambda rec=tb.rec, n=1, ch=tb.chunks, nc=None: (rec.ctypes.data if rec is not None else None, n, ch.ctypes.data if ch is not None else None,
                                                           len(tb.chunks) if nc is None else nc)
    assert l.lwdetr_mt_step_host(*args(), C.byref(h), N.MT_EMA_SET, None) == 0 and np.array_equal(e, x)
    assert l.lwdetr_mt_step_host(*args(rec=None), C.byref(h), N.MT_EMA_SET, None) == N.ERR_BAD_ARG
    assert l.lwdetr_mt_step_host(*args(ch=None), C.byref(h), N.MT_EMA_SET, None) == N.ERR_BAD_ARG
    assert l.lwdetr_mt_step_host(*args(n=0), C.byref(h), N.MT_EMA_SET, None) == N.ERR_BAD_ARG
    assert l.lwdetr_mt_step_host(*args(nc=0), C.byref(h), N.MT_EMA_SET, None) == N.ERR_BAD_ARG
    assert l.lwdetr_mt_step_host(*args(nc=2), C.byref(h), N.MT_EMA_SET, None) == N.ERR_BAD_ARG          # a tensor left partly undone: never truncated
    for field, val in (("offset", 2048 + 1024), ("count", 1024), ("tensor", 1), ("offset", -1024)):          # a chunk outside its tensor
        ch = tb.chunks.copy()
        ch[field][2] = val
        assert l.lwdetr_mt_check(*args(ch=ch)) == N.ERR_BAD_ARG, field
        before = e.copy()
        assert l.lwdetr_mt_step_host(*args(ch=ch), C.byref(h), N.MT_EMA_SET, None) == N.ERR_BAD_ARG and np.array_equal(e, before)
    assert l.lwdetr_mt_step_host(*args(), C.byref(h), 0, None) == N.ERR_BAD_ARG
    assert l.lwdetr_mt_step_host(*args(), C.byref(h), N.MT_EMA | N.MT_EMA_SET, None) == N.ERR_BAD_ARG
    assert l.lwdetr_mt_step_host(*args(), None, N.MT_EMA, None) == N.ERR_BAD_ARG
    assert l.lwdetr_mt_step_host(*args(), C.byref(h), N.MT_SCALE_GRADS, None) == N.ERR_BAD_ARG             # no clip buffer to scale by
    nc = np.ones(4, dtype=np.float32)
    assert l.lwdetr_mt_step_host(*args(), C.byref(h), N.MT_SCALE_GRADS | N.MT_ADAMW, nc.ctypes.data) == N.ERR_UNSUPPORTED
    assert l.lwdetr_mt_norm_host(*args(), 0.0, nc.ctypes.data) == N.ERR_BAD_ARG
    assert l.lwdetr_mt_norm_host(*args(), float("nan"), nc.ctypes.data) == N.ERR_BAD_ARG
    # the device entries refuse the same before any launch (no GPU is touched: the counters do not move)
    before = N.mt_launch_counts()
    assert set(before) == {"mt_sumsq", "mt_norm_finish", "mt_step"}
    assert l.lwdetr_mt_step(None, 1, None, 1, C.byref(h), N.MT_EMA, None, None) == N.ERR_BAD_ARG
    assert l.lwdetr_mt_sumsq(None, 1, None, 1, None, None) == N.ERR_BAD_ARG
    assert l.lwdetr_mt_norm_finish(None, 1, 0.1, None, None) == N.ERR_BAD_ARG
    assert N.mt_launch_counts() == before
