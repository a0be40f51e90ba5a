"""Cases, float64 references and the yardstick for csrc/train_glue.hip (lwdetr_amd.ops.train_glue).

Yardstick (the sibling training operators' rule): per case, dtype and tensor,
    figure(got, ref64) <= MARGIN * max(figure(torch formulation in the case's dtype, ref64), u_T)
with figure = max |a - b| / max |b| (two_stage_ref.figure), MARGIN = 4, the torch formulation the reference's own chain of torch operators
(projector.py:41-46, transformer.py:42-68) with autograd, run in float32 for float32 inputs and in the 16-bit dtype for 16-bit inputs, and
u_T the unit round-off of the output type (2^-24, 2^-11, 2^-8): one correct rounding of the output alone already has a figure of up to u_T,
so a formulation that happens to be exact at a shape (C = 1: y = b) sets no bound below it. float64 references take the inputs as stored in
T, widened exactly.
"""
import math

import torch

import two_stage_ref as R

DTYPES = R.DTYPES
NAME = R.NAME
MARGIN = R.MARGIN
UNIT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
EPS = 1e-6

# (B, C, H, W)
LN_CASES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 256, 1, 65), (2, 384, 9, 11), (1, 64, 8, 8), (1, 1024, 2, 3)]
# (B, Q, dim)
SINE_CASES = [(1, 1, 128), (2, 37, 128), (1, 300, 192), (1, 5, 6)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ln_inputs(shape, dtype, offset=0.0, seed=0):
    """x, weight, bias and the cotangents of both output layouts, stored in `dtype`. `offset` = 100 is the cancellation case: x = 100 + small."""
    B, C, H, W = shape
    g = _gen(seed + 7 * C + H * W)
    x = (offset + torch.randn(B, C, H, W, generator=g) * (0.05 if offset else 1.0)).to(dtype)
    w = (1 + 0.3 * torch.randn(C, generator=g)).to(dtype)
    b = (0.2 * torch.randn(C, generator=g)).to(dtype)
    go = torch.randn(B, C, H, W, generator=g).to(dtype)
    return dict(x=x, w=w, b=b, go=go)


def ln_formulation(x, w, b, eps):
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    y = (x - u) / torch.sqrt(s + eps)
    return w[:, None, None] * y + b[:, None, None]


def ln_run(inp, ct, device="cpu"):
    """The formulation with autograd in `ct` on `device`: {y, dx, dw, db} (NCHW; the token layout is a permutation of y and of the cotangent)."""
    x, w, b = (inp[k].to(device=device, dtype=ct).clone().requires_grad_(True) for k in ("x", "w", "b"))
    y = ln_formulation(x, w, b, EPS)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), inp["go"].to(device=device, dtype=ct))
    return dict(y=y.detach().cpu(), dx=dx.cpu(), dw=dw.cpu(), db=db.cpu())


def sine_boxes(case, dtype, seed=0):
    """(B, Q, 4) boxes in [-8, 8] with 0, a negative, 8, -8 and 1e-4 planted in the first row."""
    B, Q, dim = case
    g = _gen(seed + 31 * Q + dim)
    v = (torch.rand(B, Q, 4, generator=g) * 16 - 8)
    v[:, ::3] = torch.rand(B, (Q + 2) // 3, 4, generator=g)              # most boxes of a model are in [0, 1]
    v[0, 0] = torch.tensor([0.0, -0.37, 8.0, 1e-4])
    if Q > 1:
        v[0, 1] = torch.tensor([-8.0, 1e-4, -1e-4, 7.999])
    return v.to(dtype)


def sine_formulation(boxes, dim):
    dim_t = torch.arange(dim, dtype=torch.float32, device=boxes.device)
    dim_t = 10000 ** (2 * (dim_t // 2) / dim)
    out = []
    for c in (1, 0, 2, 3):
        e = (boxes[:, :, c] * (2 * math.pi))[:, :, None] / dim_t
        out.append(torch.stack((e[:, :, 0::2].sin(), e[:, :, 1::2].cos()), dim=3).flatten(2))
    return torch.cat(out, dim=2)


def sine_run(boxes, go, dim, ct, device="cpu"):
    b = boxes.to(device=device, dtype=ct).clone().requires_grad_(True)
    out = sine_formulation(b, dim)
    gb, = torch.autograd.grad(out, b, go.to(device=device, dtype=ct))
    return dict(out=out.detach().cpu(), gboxes=gb.cpu())


def check(got, ref64, yard, dtype, what):
    """Prints both figures of every tensor and returns the failures [(tensor, figure, bound)]."""
    fails = []
    for k in ref64:
        f_got, f_yard = R.figure(got[k].cpu(), ref64[k]), R.figure(yard[k], ref64[k])
        bound = MARGIN * max(f_yard, UNIT[dtype])
        print(f"{what} {k}: figure {f_got:.3e}, torch formulation {f_yard:.3e}, bound {bound:.3e}")
        if not f_got <= bound:
            fails.append((k, f_got, bound))
    return fails
