"""GPU: csrc/train_glue.hip through lwdetr_amd.ops.train_glue on the cases of train_glue_ref.py.
  - LayerNorm2d: y, dx, dw and db of every case, both output layouts, f32 / bf16 / f16, against the float64 formulation under the yardstick of
    train_glue_ref.py; x = 100 + small (cancellation in the variance); a channels-last x; a second backward bit-identical; the launch forms
    pinned through train_glue_path_counts;
  - sine embed: the output and d boxes of every case (values 0, negative, |v| up to 8, 1e-4) on a row-strided boxes view, the same yardstick,
    a second backward bit-identical, launch forms pinned;
  - CPU tensors and float64 raise.
"""
import contextlib

import pytest
import torch

import train_glue_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def TG():
    from lwdetr_amd import _native
    from lwdetr_amd.ops import train_glue
    _native.lib()
    return train_glue


@contextlib.contextmanager
def served_by(forms):
    """The train_glue launches inside the block are exactly `forms` ({name: launches})."""
    from lwdetr_amd import _native
    before = _native.train_glue_path_counts()
    assert set(forms) <= set(before), sorted(before)
    yield
    torch.cuda.synchronize()
    after = _native.train_glue_path_counts()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert delta == forms, f"expected {forms}, the launches went to {delta}"


def ln_gpu(TG, inp, tokens, x=None):
    x = (inp["x"].to(DEV) if x is None else x).requires_grad_(True)
    w, b = inp["w"].to(DEV).requires_grad_(True), inp["b"].to(DEV).requires_grad_(True)
    y = TG.layer_norm_2d(x, w, b, G.EPS, tokens=tokens)
    B, C, H, W = inp["x"].shape
    go = inp["go"].to(DEV)
    if tokens:
        assert y.shape == (B, H * W, C) and y.is_contiguous()
        go = go.flatten(2).transpose(1, 2).contiguous()
    else:
        assert y.shape == (B, C, H, W) and y.is_contiguous()
    dx, dw, db = torch.autograd.grad(y, (x, w, b), go, retain_graph=True)
    again = torch.autograd.grad(y, (x, w, b), go)
    assert all(torch.equal(a, b_) for a, b_ in zip((dx, dw, db), again)), "a second backward returned other bits"
    assert dx.shape == x.shape and dw.dtype == w.dtype and db.dtype == b.dtype
    y = y.detach()
    if tokens:
        y = y.transpose(1, 2).reshape(B, C, H, W)
    return dict(y=y, dx=dx, dw=dw, db=db)


LN_PARAMS = [pytest.param(c, dt, tok, id=f"{'x'.join(map(str, c))}-{G.NAME[dt]}-{'tok' if tok else 'nchw'}")
             for dt in G.DTYPES for c in G.LN_CASES for tok in (False, True)]


@pytest.mark.parametrize("shape,dtype,tokens", LN_PARAMS)
def test_layer_norm_2d_against_fp64(TG, shape, dtype, tokens):
    inp = G.ln_inputs(shape, dtype)
    ref64 = G.ln_run(inp, torch.float64)
    yard = G.ln_run(inp, dtype, DEV if dtype != torch.float32 else "cpu")
    lay = "tok" if tokens else "nchw"
    with served_by({f"ln2d_fwd_{lay}_{G.NAME[dtype]}": 1, f"ln2d_bwd_{lay}_{G.NAME[dtype]}": 2}):
        got = ln_gpu(TG, inp, tokens)
    assert not G.check(got, ref64, yard, dtype, f"ln2d {shape} {G.NAME[dtype]} {lay}")


@pytest.mark.parametrize("tokens", [False, True])
def test_layer_norm_2d_cancellation(TG, tokens):
    """x = 100 + small: E[x^2] - E[x]^2 would lose the variance; two passes do not."""
    inp = G.ln_inputs((2, 384, 9, 11), torch.float32, offset=100.0)
    ref64, yard = G.ln_run(inp, torch.float64), G.ln_run(inp, torch.float32)
    assert not G.check(ln_gpu(TG, inp, tokens), ref64, yard, torch.float32, f"ln2d cancellation tokens={tokens}")


def test_layer_norm_2d_channels_last_input(TG):
    inp = G.ln_inputs((2, 64, 5, 7), torch.float32)
    x = inp["x"].to(DEV).contiguous(memory_format=torch.channels_last)
    assert not x.is_contiguous()
    ref64, yard = G.ln_run(inp, torch.float64), G.ln_run(inp, torch.float32)
    assert not G.check(ln_gpu(TG, inp, True, x=x), ref64, yard, torch.float32, "ln2d channels-last")


def sine_gpu(TG, boxes, go, dim):
    B, Q, _ = boxes.shape
    wide = torch.full((B, Q, 3, 4), 12345.0, dtype=boxes.dtype, device=DEV)
    wide[:, :, 0] = boxes.to(DEV)
    wide.requires_grad_(True)
    view = wide[:, :, 0, :]
    assert view.stride(1) == 12
    out = TG.query_sine_embed(view, dim)
    assert out.shape == (B, Q, 4 * dim) and out.is_contiguous()
    g1, = torch.autograd.grad(out, wide, go.to(DEV), retain_graph=True)
    g2, = torch.autograd.grad(out, wide, go.to(DEV))
    assert torch.equal(g1, g2), "a second backward returned other bits"
    assert not g1[:, :, 1:].any()
    return dict(out=out.detach(), gboxes=g1[:, :, 0])


SINE_PARAMS = [pytest.param(c, dt, id=f"{'x'.join(map(str, c))}-{G.NAME[dt]}") for dt in G.DTYPES for c in G.SINE_CASES]


@pytest.mark.parametrize("case,dtype", SINE_PARAMS)
def test_sine_embed_against_fp64(TG, case, dtype):
    B, Q, dim = case
    boxes = G.sine_boxes(case, dtype)
    go = torch.randn(B, Q, 4 * dim, generator=torch.Generator().manual_seed(5)).to(dtype)
    ref64 = G.sine_run(boxes, go, dim, torch.float64)
    yard = G.sine_run(boxes, go, dim, dtype, DEV if dtype != torch.float32 else "cpu")
    with served_by({f"sine_fwd_{G.NAME[dtype]}": 1, f"sine_bwd_{G.NAME[dtype]}": 2}):
        got = sine_gpu(TG, boxes, go, dim)
    assert not G.check(got, ref64, yard, dtype, f"sine {case} {G.NAME[dtype]}")


def test_cpu_tensors_and_float64_raise(TG):
    x, w = torch.randn(1, 4, 2, 2), torch.ones(4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        TG.layer_norm_2d(x, w, w, 1e-6)
    with pytest.raises(RuntimeError, match="not supported"):
        TG.layer_norm_2d(x.double().to(DEV), w.double().to(DEV), w.double().to(DEV), 1e-6)
    with pytest.raises(RuntimeError, match="outside the kernel's range"):
        TG.layer_norm_2d(torch.randn(1, 1025, 1, 1, device=DEV), torch.ones(1025, device=DEV), torch.ones(1025, device=DEV), 1e-6)
    with pytest.raises(RuntimeError, match="ROCm device"):
        TG.query_sine_embed(torch.rand(1, 2, 4), 128)
    with pytest.raises(RuntimeError, match="not supported"):
        TG.query_sine_embed(torch.rand(1, 2, 4, device=DEV).double(), 128)
    with pytest.raises(RuntimeError, match="must be even"):
        TG.query_sine_embed(torch.rand(1, 2, 4, device=DEV), 7)
