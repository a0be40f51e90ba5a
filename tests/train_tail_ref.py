"""Shared inputs and references of the training-step-tail tests (test_train_tail_host.py on the CPU, test_gpu_train_tail.py on the GPU).

The *edge set*: f32 parameters of the element counts SIZES - around the quad (4), the wave (64), a round of a wave (256) and the chunk
(lwdetr_amd.train.CHUNK = 1024: one below, at, above, two chunks + 1) -, two of them views at element offset 1 of a larger storage (not
16-byte aligned: a short one and one with a full chunk), one without a gradient, per-tensor lr = 1e-4 * 0.8^(i % 5), weight decay 0 for every
third tensor, and three EMA-only buffers: an int64 scalar and two f32 tensors. Three steps at max_norm = 0.1: the clip binds in steps 1 and 3
and clamps to 1 in step 2.

References, computed once per process and never changed by a test:
  restate(case, float64, ...)  the three reference steps (clip_grad_norm_, AdamW, ModelEma.update) restated with torch ops in float64 on the
                               rounded f32 inputs;
  torch_sequence(case, ...)    the reference sequence itself in f32 on the CPU: torch.nn.utils.clip_grad_norm_, torch.optim.AdamW(foreach=False)
                               over one group per parameter, the ModelEma formula with copy_.
The bound, per tensor: max |native - fp64| <= max(4 x max |torch_f32 - fp64| over the same tensor, 2 ulp_f32 of the tensor's largest magnitude).
"""
import copy
import functools

import numpy as np
import torch

CHUNK = 1024
SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 257, 1023, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, CHUNK + 6]
VIEWS = (8, 14)                # views at element offset 1
NO_GRAD = 4
BUF_SIZES = (7, CHUNK + 6)     # the two f32 buffers; the int64 buffer is a scalar
MAX_NORM = 0.1
BETAS, EPS, DECAY = (0.9, 0.999), 1e-8, 0.9997
GRAD_SCALE = (1e-2, 1e-6, 3e-2)
STEPS = 3


def lr_of(i):
    return 1e-4 * 0.8 ** (i % 5)


def wd_of(i):
    return 0.0 if i % 3 == 0 else 0.05


@functools.lru_cache(maxsize=None)
def make_case(seed=1234, grad_scale=GRAD_SCALE):
    """Deterministic CPU f32 inputs: params, grads[step][i] (None at NO_GRAD), the buffers' initial values and their values at each step."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda n, s: torch.randn(n, generator=g, dtype=torch.float32) * s
    case = {"params": [rn(n, 0.5) for n in SIZES],
            "grads": [[None if i == NO_GRAD else rn(n, grad_scale[s]) for i, n in enumerate(SIZES)] for s in range(STEPS)],
            "buf0": [torch.tensor(5, dtype=torch.int64)] + [rn(n, 1.0) for n in BUF_SIZES],
            "bufs": [[torch.tensor(x, dtype=torch.int64)] + [rn(n, 1.0) for n in BUF_SIZES] for x in (6, 4000, 40000)]}
    return case


def groups_for(params):
    return [{"params": [p], "lr": lr_of(i), "weight_decay": wd_of(i)} for i, p in enumerate(params)]


class EdgeModel(torch.nn.Module):
    """The edge set as a module built ON its device (Module.to() would compact the views): parameters p0.., buffers b0 (int64), b1, b2."""

    def __init__(self, case, device):
        super().__init__()
        for i, p in enumerate(case["params"]):
            if i in VIEWS:
                store = torch.zeros(p.numel() + 3, dtype=torch.float32, device=device)
                t = store[1:1 + p.numel()]
                t.copy_(p)
                assert t.data_ptr() % 16 == 4
            else:
                t = p.clone().to(device)
            self.register_parameter(f"p{i}", torch.nn.Parameter(t))
        for j, b in enumerate(case["buf0"]):
            self.register_buffer(f"b{j}", b.clone().to(device))

    def plist(self):
        return [getattr(self, f"p{i}") for i in range(len(SIZES))]

    def blist(self):
        return [getattr(self, f"b{j}") for j in range(1 + len(BUF_SIZES))]

    def load_step(self, case, s, grads=True):
        for p, g in zip(self.plist(), case["grads"][s]):
            p.grad = None if (g is None or not grads) else g.clone().to(p.device)
        with torch.no_grad():
            for b, x in zip(self.blist(), case["bufs"][s]):
                b.copy_(x)


def _snap(p, m, v, ema, norm, grads):
    f = lambda ts: [None if t is None else t.detach().cpu().clone() for t in ts]
    return {"p": f(p), "m": f(m), "v": f(v), "ema": f(ema), "norm": None if norm is None else float(norm), "grads": f(grads)}


def ema_i64(e, x, decay=DECAY):
    """The reference's ModelEma formula on int64 tensors, as it runs: f32 arithmetic, truncated by copy_."""
    out = e.clone()
    out.copy_(decay * e + (1. - decay) * x)
    return out


def restate(case, dtype=torch.float64, max_norm=MAX_NORM, ema=True):
    """The reference's three steps with torch ops in ``dtype``: [snapshot per step] with p, m, v, ema (parameters, then buffers), norm, grads
    (the clipped gradients, as the reference leaves them in p.grad)."""
    p = [t.to(dtype) for t in case["params"]]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    e = [t.clone() for t in p] + [case["buf0"][0].clone()] + [b.to(dtype) for b in case["buf0"][1:]]
    t_of = [0] * len(p)
    b1, b2 = BETAS
    out = []
    for s in range(STEPS):
        gs = [None if g is None else g.to(dtype) for g in case["grads"][s]]
        norm = None
        if max_norm > 0:
            norm = torch.sqrt(sum((g * g).sum() for g in gs if g is not None))
            coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
            gs = [None if g is None else g * coef for g in gs]
        for i, g in enumerate(gs):
            if g is None:
                continue
            t_of[i] += 1
            lr, wd = lr_of(i), wd_of(i)
            p[i] = p[i] * (1 - lr * wd)
            m[i] = m[i] + (g - m[i]) * (1 - b1)
            v[i] = v[i] * b2 + (1 - b2) * g * g
            denom = v[i].sqrt() / (1 - b2 ** t_of[i]) ** 0.5 + EPS
            p[i] = p[i] - (lr / (1 - b1 ** t_of[i])) * (m[i] / denom)
        if ema:
            x = p + [case["bufs"][s][0]] + [b.to(dtype) for b in case["bufs"][s][1:]]
            e = [ema_i64(a, b) if a.dtype == torch.int64 else DECAY * a + (1. - DECAY) * b for a, b in zip(e, x)]
        seen = lambda ts: [t if t_of[i] else None for i, t in enumerate(ts)]      # torch creates a parameter's state with its first gradient
        out.append(_snap(p, seen(m), seen(v), e if ema else [], norm, gs))
    return out


def torch_sequence(case, max_norm=MAX_NORM, ema=True):
    """The reference sequence in f32 on the CPU with torch's own classes; snapshots as restate()."""
    model = EdgeModel(case, "cpu")
    ps = model.plist()
    opt = torch.optim.AdamW(groups_for(ps), lr=1e-4, betas=BETAS, eps=EPS, weight_decay=1e-4, foreach=False)
    shadow = copy.deepcopy(model).eval()
    out = []
    for s in range(STEPS):
        model.load_step(case, s)
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm) if max_norm > 0 else None
        opt.step()
        if ema:
            with torch.no_grad():
                for ev, mv in zip(shadow.state_dict().values(), model.state_dict().values()):
                    ev.copy_(DECAY * ev + (1. - DECAY) * mv)
        out.append(snapshot(model, opt, shadow if ema else None, norm))
    return out


def snapshot(model, opt, shadow, norm):
    ps = model.plist()
    st = [opt.state.get(p, {}) for p in ps]
    return _snap(ps, [s.get("exp_avg") for s in st], [s.get("exp_avg_sq") for s in st],
                 list(shadow.state_dict().values()) if shadow is not None else [], norm, [p.grad for p in ps])


@functools.lru_cache(maxsize=None)
def references(max_norm=MAX_NORM, ema=True):
    """(fp64 restatement, f32 torch sequence) for the edge set - computed once, shared by the tests."""
    case = make_case()
    return restate(case, torch.float64, max_norm, ema), torch_sequence(case, max_norm, ema)


def run_native(case, device, form, max_norm=MAX_NORM, ema=True, steps=STEPS, hook=None):
    """The edge set through lwdetr_amd.train on ``device`` ("cpu": the library's host form). form "fused": NativeAdamW(max_norm=, ema=) and the
    ema.update() the reference's loop keeps calling; form "standalone": train.clip_grad_norm_ + stock torch.optim.AdamW + a stand-alone
    ModelEma.update. Returns (snapshots, model, optimizer, ema); hook(step, model, opt) runs before each step."""
    from lwdetr_amd import train as T
    model = EdgeModel(case, device)
    ps = model.plist()
    ema_m = T.ModelEma(model, decay=DECAY) if ema else None
    if form == "fused":
        opt = T.NativeAdamW(groups_for(ps), lr=1e-4, betas=BETAS, eps=EPS, weight_decay=1e-4, max_norm=max_norm, ema=ema_m, host=device == "cpu")
    else:
        opt = torch.optim.AdamW(groups_for(ps), lr=1e-4, betas=BETAS, eps=EPS, weight_decay=1e-4)
    out = []
    for s in range(steps):
        model.load_step(case, s)
        if hook is not None:
            hook(s, model, opt)
        norm = None
        if form == "fused":
            opt.step()
            norm = opt.last_total_norm if max_norm > 0 else None
        else:
            if max_norm > 0:
                norm = T.clip_grad_norm_(ps, max_norm)
            opt.step()
        if ema:
            ema_m.update(model)
        out.append(snapshot(model, opt, ema_m.module if ema else None, norm))
    return out, model, opt, ema_m


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def tensor_bound(ref64, ref32):
    """The bound for one tensor: max(4 x torch's own f32 distance to fp64, 2 ulp_f32 of the largest magnitude)."""
    dist = float((ref32.double() - ref64).abs().max())
    return max(4.0 * dist, 2.0 * ulp32(float(ref64.abs().max())))


def check_snapshots(got, ref64, ref32, keys=("p", "m", "v", "ema"), label=""):
    """Every tensor of every step under the rule; int64 entries exact. Returns the worst error / bound ratio (printed by the callers)."""
    worst = 0.0
    for s, (g, r64, r32) in enumerate(zip(got, ref64, ref32)):
        for k in keys:
            assert len(g[k]) == len(r64[k]), (label, s, k)
            for i, (a, b, c) in enumerate(zip(g[k], r64[k], r32[k])):
                if b is None:
                    assert a is None, (label, s, k, i)
                    continue
                if b.dtype == torch.int64:
                    assert a.dtype == torch.int64 and torch.equal(a, b) and torch.equal(c, b), (label, s, k, i, a, b)
                    continue
                err, bound = float((a.double() - b).abs().max()), tensor_bound(b, c)
                worst = max(worst, err / bound)
                assert err <= bound, f"{label} step {s} {k}[{i}] ({a.numel()} elements): |native - fp64| = {err:.3e} > bound {bound:.3e}"
    return worst
