"""GPU: the 16-bit C = 384 form of lwdetr_vit_block_few (vit_block_few384_kernel, vit_block_few384.hip) against float64 - residual stream, tap copy, row
statistics, chained q / k / v^T - under the 16-bit bounds of test_gpu_kernels.py::test_mlp_fused; element-wise against the error of lwdetr_mlp_fused
at C = 384 (mlp_kernel<T, 384>, row-major weights) on the same operands; determinism; the entry's refusals; and LW-DETR-medium / large in 16-bit with the
plan switch LWDETR_VIT_BLOCK_FEW_C384 on and unset against the reference goldens. One tile form is built (16 tokens per workgroup), so there is no
tile-form case. Every launch is pinned to its instantiation by the launch-form record (helpers.mlp_served_by); the per-element bounds are in
tests/test_gpu_mlp_fp64.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import case_batch, golden_state_dict, load_golden, mlp_served_by
from test_gpu_kernels import _dev, _rand, _relerr

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
C = 384
SENT = 7.0
# (M, Tp, heads): one lane group of one tile; a ragged second tile (clamped-address rows); an image boundary inside a tile, hd 64; hd 16, full tiles;
# 13 tiles with images that straddle tiles
SHAPES = [(4, 4, 12), (20, 20, 12), (40, 20, 6), (48, 16, 24), (208, 52, 12)]
TOL = {F16: 6e-3, BF16: 5e-2}                                        # test_mlp_fused's; q / k / v^T twice that
QSCALE = 0.37
_CACHE = {}


def _case(m, tp, heads, dtype):
    """Operands drawn as in test_gpu_vit_block_few_f32.py::_case with C = 384, their packing in `dtype`, and the float64 reference (x1 rounded to the
    storage type, as the kernels do and test_mlp_fused's reference does) - once per shape and dtype, never modified."""
    key = (m, tp, heads, dtype)
    if key in _CACHE:
        return _CACHE[key]
    from lwdetr_amd import kernels as K
    c, hd, nb = C, C // heads, m // tp
    o = dict(m=m, tp=tp, heads=heads, hd=hd, nb=nb, dtype=dtype)
    o["x"] = _rand(m, c, dtype=dtype, seed=1) * 2 + 0.3
    o["att"] = _rand(m, c, dtype=dtype, seed=9)
    w1, b1 = _rand(4 * c, c, scale=c ** -0.5, seed=2), _rand(4 * c, seed=3) * 0.1
    w2, o["b2"] = _rand(c, 4 * c, scale=(4 * c) ** -0.5, seed=4), _rand(c, seed=5) * 0.1
    lw, lb = _rand(c, seed=6) * 0.2 + 1, _rand(c, seed=7) * 0.1
    o["g2"], o["g1"] = _rand(c, seed=8) * 0.3, _rand(c, seed=12) * 0.3
    wp, o["bp"] = _rand(c, c, scale=c ** -0.5, seed=10), _rand(c, seed=11) * 0.1
    wqkv = _rand(3 * c, c, scale=c ** -0.5, seed=13)
    qb, vb = _rand(c, seed=14) * 0.1, _rand(c, seed=15) * 0.1
    lw1, lb1 = _rand(c, seed=16) * 0.2 + 1, _rand(c, seed=17) * 0.1
    o["w1p"], o["b1p"], o["w2p"] = K.pack_mlp_weights(w1, b1, w2, lw, lb, dtype, proj=True)
    o["wq"], o["bq"] = K.pack_qkv_weights(wqkv, qb, vb, lw1, lb1, dtype)
    o["wp"] = wp.to(dtype).contiguous()
    o["w1F"], o["wpF"], o["wqF"] = K.pack_frag16(o["w1p"]), K.pack_frag16(o["wp"]), K.pack_frag16(o["wq"])
    d = lambda t: t.double()
    x1 = (d(o["x"]) + d(o["g1"]) * (d(o["att"]) @ d(wp).t() + d(o["bp"]))).to(dtype).double()
    ref = x1 + d(o["g2"]) * (F.gelu(F.layer_norm(x1, (c,), d(lw), d(lb), 1e-6) @ d(w1).t() + d(b1)) @ d(w2).t() + d(o["b2"]))
    y = F.layer_norm(ref, (c,), d(lw1), d(lb1), 1e-6) @ d(wqkv).t() + torch.cat([d(qb), torch.zeros_like(d(qb)), d(vb)])
    sp = lambda t_: t_.reshape(nb, tp, heads, hd).permute(0, 2, 1, 3)
    o["ref"] = dict(x=ref, q=(sp(y[:, :c]) * QSCALE).contiguous(), k=sp(y[:, c:2 * c]).contiguous(), vt=sp(y[:, 2 * c:]).transpose(2, 3).contiguous())
    _CACHE[key] = o
    return o


def _buffers(o, pad=16):
    """Fresh outputs with sentinel guards: `pad` rows behind x / taps / stats, `pad` elements behind q / k / v^T, the left half of the tap buffer."""
    m, dev, n, dt = o["m"], _dev(), o["nb"] * o["heads"] * o["tp"] * o["hd"], o["dtype"]
    b = dict(x=torch.full((m + pad, C), SENT, dtype=dt, device=dev), taps=torch.full((m + pad, 2 * C), SENT, dtype=dt, device=dev),
             stats=torch.full((m + pad, 2), SENT, dtype=F32, device=dev))
    b["x"][:m] = o["x"]
    for nme in ("q", "k", "vt"):
        b[nme + "_flat"] = torch.full((n + pad,), SENT, dtype=dt, device=dev)
    b["q"] = b["q_flat"][:n].view(o["nb"], o["heads"], o["tp"], o["hd"])
    b["k"] = b["k_flat"][:n].view(o["nb"], o["heads"], o["tp"], o["hd"])
    b["vt"] = b["vt_flat"][:n].view(o["nb"], o["heads"], o["hd"], o["tp"])
    return b


def _run(o, b, *, few=True, qkv=True, extras=True):
    from lwdetr_amd import kernels as K
    cls = K.VitBlockFewOp if few else K.MlpFusedOp
    kw = dict(att=o["att"], wp=o["wpF"] if few else o["wp"], bp=o["bp"], gamma1=o["g1"])
    if extras:
        kw.update(out2=b["taps"][:, C:], ld2=2 * C, stats_out=b["stats"])
    if qkv:
        kw.update(wqkv=o["wqF"] if few else o["wq"], bqkv=o["bq"], q=b["q"], k=b["k"], vt=b["vt"], qscale=QSCALE, heads=o["heads"], hd=o["hd"], Tp=o["tp"])
    name = {F16: "f16", BF16: "bf16"}[o["dtype"]]
    with mlp_served_by(f"vit_few384_{name}_qkv{int(qkv)}" if few else f"mlp_{name}_c384_proj1_qkv{int(qkv)}"):
        cls(b["x"], o["w1F"] if few else o["w1p"], o["b1p"], o["w2p"], o["b2"], o["g2"], o["m"], C, 1e-6, **kw)()
    torch.cuda.synchronize()


def _sentinel(t):
    return bool((t == SENT).all())


@pytest.mark.parametrize("extras", [True, False], ids=["tap+stats", "bare"])
@pytest.mark.parametrize("qkv", [True, False], ids=["qkv", "noqkv"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%d-Tp%d-h%d" % s)
def test_vit_block_few_c384_vs_fp64(shape, dtype, qkv, extras):
    o = _case(*shape, dtype)
    m, tol = o["m"], TOL[dtype]
    b = _buffers(o)
    _run(o, b, qkv=qkv, extras=extras)
    r = o["ref"]
    ex = _relerr(b["x"][:m].double(), r["x"])
    print(f"{shape} {dtype} qkv={qkv} extras={extras}: relerr x {ex:.3e}", end="")
    assert ex < tol, ex
    assert _sentinel(b["x"][m:])                                     # rows at or beyond M
    if extras:
        assert torch.equal(b["taps"][:m, C:], b["x"][:m])            # the tap: bit for bit
        assert _sentinel(b["taps"][:, :C]) and _sentinel(b["taps"][m:])
        xx = b["x"][:m].double()
        mean, var = xx.mean(1), xx.var(1, unbiased=False)
        rstd = (var + 1e-6).rsqrt()
        dm = (b["stats"][:m, 0].double() - mean).abs().max().item()
        dr = ((b["stats"][:m, 1].double() - rstd).abs() / rstd).max().item()
        print(f"  mean {dm:.2e} rstd {dr:.2e}", end="")
        assert dm < 1e-4 and dr < 1e-4, (dm, dr)
        assert _sentinel(b["stats"][m:])
    else:
        assert _sentinel(b["taps"]) and _sentinel(b["stats"])
    if qkv:
        n = b["q"].numel()
        for nme in ("q", "k", "vt"):
            e = _relerr(b[nme].double(), r[nme])
            print(f"  {nme} {e:.3e}", end="")
            assert e < 2 * tol, (nme, e)
            assert _sentinel(b[nme + "_flat"][n:]), nme
    else:
        assert all(_sentinel(b[nme + "_flat"]) for nme in ("q", "k", "vt"))
    print()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_vit_block_few_c384_error_is_that_of_the_fused_kernel(dtype):
    """Element-wise yardstick that is not the code under test: lwdetr_mlp_fused at C = 384 (mlp_kernel<T, 384>, row-major weights) on the same operands.
    Both kernels round at the same places and sum the same products in f32, in another order, so their worst elements against float64 over >= 10^4
    outputs per tensor differ by far less than 2x; more is a wrong operand. Figures: profiles/r7c_vit_block_few_c384.txt."""
    shape = (208, 52, 12)
    o = _case(*shape, dtype)
    m, r = o["m"], o["ref"]
    new, old = _buffers(o), _buffers(o)
    _run(o, new, few=True)
    _run(o, old, few=False)
    for nme in ("x", "q", "k", "vt"):
        a, y = (new[nme][:m], old[nme][:m]) if nme == "x" else (new[nme], old[nme])
        assert a.numel() >= 10 ** 4
        e_new = (a.double() - r[nme]).abs().max().item()
        e_old = (y.double() - r[nme]).abs().max().item()
        print(f"{shape} {dtype} {nme}: max|err| vs fp64  vit_block_few C=384 {e_new:.3e}   mlp_fused C=384 {e_old:.3e}   ratio {e_new / e_old:.2f}")
        assert e_old > 0 and e_new <= 2 * e_old, (nme, e_new, e_old)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_vit_block_few_c384_is_deterministic(dtype):
    o = _case(208, 52, 12, dtype)
    a, b = _buffers(o), _buffers(o)
    _run(o, a)
    _run(o, b)
    for nme in ("x", "taps", "stats", "q_flat", "k_flat", "vt_flat"):
        assert torch.equal(a[nme], b[nme]), nme


def test_vit_block_few_c384_refusals():
    """lwdetr_vit_block_few at C = 384 answers before any launch - every output bit-identical to a snapshot - LWDETR_ERR_BAD_ARG for ldx = 388 and for
    heads = 6, hd = 32, LWDETR_ERR_UNSUPPORTED for C = 768 and M = 12 800; the same call without the defect returns 0 and changes the outputs.
    (All buffers hold 12 800 rows of 768 values, so that no argument set of this test describes memory that is not there.)"""
    from lwdetr_amd import _native, kernels as K
    UNS, BAD = _native.ERR_UNSUPPORTED, _native.ERR_BAD_ARG
    o = _case(208, 52, 12, F16)
    dev, m, big, wide = _dev(), o["m"], 12800, 768
    n = o["nb"] * o["heads"] * o["tp"] * o["hd"]
    xs = torch.full((big * wide,), SENT, dtype=F16, device=dev)
    atts = torch.zeros(big * wide, dtype=F16, device=dev)
    taps = torch.full((big * 2 * wide,), SENT, dtype=F16, device=dev)
    stats = torch.full((big, 2), SENT, dtype=F32, device=dev)
    qs, ks, vs = (torch.full((big * wide,), SENT, dtype=F16, device=dev) for _ in range(3))
    xs[:m * C] = o["x"].flatten()
    atts[:m * C] = o["att"].flatten()
    outs = (xs, taps, stats, qs, ks, vs)
    snap = [t.clone() for t in outs]

    def call(*, ldx=C, c=C, rows=m, tp=o["tp"], heads=12, hd=32):
        nq = rows * c
        op = K.MlpFusedOp(xs, o["w1F"], o["b1p"], o["w2p"], o["b2"], o["g2"], rows, c, 1e-6, ldx=ldx, out2=taps[C:], ld2=2 * C,
                          stats_out=stats, att=atts, ldatt=C, wp=o["wpF"], bp=o["bp"], gamma1=o["g1"], wqkv=o["wqF"], bqkv=o["bq"],
                          q=qs[:nq], k=ks[:nq], vt=vs[:nq], qscale=QSCALE, heads=heads, hd=hd, Tp=tp)
        rc = _native.lib().lwdetr_vit_block_few(*op.args, _native.stream_ptr())
        torch.cuda.synchronize()
        return rc, all(torch.equal(t, s) for t, s in zip(outs, snap))

    assert call(ldx=388) == (BAD, True)
    assert call(heads=6, hd=32) == (BAD, True)
    assert call(c=768, heads=24) == (UNS, True)
    assert call(rows=12800, tp=400) == (UNS, True)
    assert n == m * C
    with mlp_served_by("vit_few384_f16_qkv1"):
        rc, same = call()                                            # the control
    assert rc == 0 and not same
    assert _relerr(xs[:m * C].view(m, C).double(), o["ref"]["x"]) < TOL[F16]
    assert _sentinel(xs[m * C:]) and _sentinel(qs[n:]) and _sentinel(ks[n:]) and _sentinel(vs[n:])


# ---------------------------------------------------------------------------------------------------------------- model level
def _forward_vs_golden(name, dtype, monkeypatch, switch, nested=False):
    """One teacher-forced 16-bit forward of the golden case `name` on a freshly built plan: (op class names of the plan, depth of the ViT, max |difference|
    per output tensor against the reference golden, |difference| of the encoder class maximum)."""
    import lwdetr_amd
    from test_gpu_model import DEV, _diffs, _model
    if switch is None:
        monkeypatch.delenv("LWDETR_VIT_BLOCK_FEW_C384", raising=False)
    else:
        monkeypatch.setenv("LWDETR_VIT_BLOCK_FEW_C384", switch)
    for var in ("LWDETR_MLP_FUSED", "LWDETR_VIT_BLOCK_FEW", "LWDETR_VIT_BLOCK_FEW_F32", "LWDETR_GEMM_FEW", "LWDETR_GEMM_FEW_F32", "LWDETR_MLP_SMALL_TT",
                "LWDETR_VIT_BLOCK"):
        monkeypatch.delenv(var, raising=False)
    g = load_golden(name)
    size, images, mask = case_batch(name)
    model, _ = _model(size, golden_state_dict(g), dtype)             # the plan is built by the first forward, under the environment above
    forced = torch.from_numpy(g["topk_idx"]).to(DEV)
    col = {}
    inp = lwdetr_amd.models.NestedTensor(images.to(DEV).to(dtype), mask.to(DEV)) if nested else images.to(DEV)
    out = model(inp, _collect=col, _forced_topk=forced)
    torch.cuda.synchronize()
    plans = list(model._plans.values())
    ops = [type(op).__name__ for plan in plans for grp in (plan.ops_backbone, plan.ops_enc, plan.ops_sel, plan.ops_dec) for op in grp]
    d = _diffs(out, g)
    d["enc_class_max"] = float(np.abs(col["enc.class_max"].cpu().numpy() - g["enc_class_max"]).max())
    return ops, plans[0].depth * len(plans), d


@pytest.mark.parametrize("name,dtype,tol_mem,tol_logit,tol_box", [("medium_640", BF16, 0.3, 0.26, 0.02), ("large_640", F16, 0.05, 0.083, 0.0074)])
def test_16_bit_model_with_the_switch_on_runs_one_block_launch_per_vit_block_and_meets_the_golden(name, dtype, tol_mem, tol_logit, tol_box, monkeypatch):
    """Bounds: test_gpu_model.py::test_low_precision_teacher_forced."""
    ops, depth, d = _forward_vs_golden(name, dtype, monkeypatch, "1")
    assert ops.count("VitBlockFewOp") == depth and depth > 0, (ops.count("VitBlockFewOp"), depth)
    assert "MlpFusedOp" not in ops
    print(f"{name} {dtype}, LWDETR_VIT_BLOCK_FEW_C384=1:", d)
    assert d["enc_class_max"] < tol_mem, d
    assert max(d["pred_logits"], d["enc_logits"]) < tol_logit, d
    assert max(d["pred_boxes"], d["enc_boxes"]) < tol_box, d


def test_large_padded_fp16_with_the_switch_on(monkeypatch):
    """Bounds: test_gpu_model.py::test_low_precision_padded_batches_through_the_row_chains (large_padded, fp16)."""
    ops, depth, d = _forward_vs_golden("large_padded", F16, monkeypatch, "1", nested=True)
    assert ops.count("VitBlockFewOp") == depth and depth > 0, (ops.count("VitBlockFewOp"), depth)
    assert "MlpFusedOp" not in ops
    print("large_padded fp16, LWDETR_VIT_BLOCK_FEW_C384=1:", d)
    assert max(d["pred_logits"], d["enc_logits"]) < 0.09, d
    assert max(d["pred_boxes"], d["enc_boxes"]) < 0.008, d


def test_large_fp16_with_the_switch_unset_builds_no_block_launch(monkeypatch):
    """No behaviour change: the default large fp16 plan at the golden batch has neither VitBlockFewOp nor MlpFusedOp and meets the golden as before."""
    ops, _, d = _forward_vs_golden("large_640", F16, monkeypatch, None)
    assert "VitBlockFewOp" not in ops and "MlpFusedOp" not in ops
    assert d["enc_class_max"] < 0.05, d
    assert max(d["pred_logits"], d["enc_logits"]) < 0.083, d
    assert max(d["pred_boxes"], d["enc_boxes"]) < 0.0074, d


def test_large_fp16_capture_with_the_switch_on_replays_bit_identically(monkeypatch):
    """model.capture on one large fp16 image with the switch on: two replays equal each other and the eager call bit for bit."""
    from test_gpu_model import DEV, _model
    monkeypatch.setenv("LWDETR_VIT_BLOCK_FEW_C384", "1")
    for var in ("LWDETR_MLP_FUSED", "LWDETR_VIT_BLOCK_FEW", "LWDETR_VIT_BLOCK"):
        monkeypatch.delenv(var, raising=False)
    g = load_golden("large_640")
    size, images, _ = case_batch("large_640")
    model, _ = _model(size, golden_state_dict(g), F16)
    one = images[:1].to(DEV)
    graphed = model.capture(one)
    r1 = {k: v.clone() for k, v in graphed(one).items() if isinstance(v, torch.Tensor)}
    r2 = graphed(one)
    assert torch.equal(r1["pred_logits"], r2["pred_logits"]) and torch.equal(r1["pred_boxes"], r2["pred_boxes"])
    eager = model(one)
    assert torch.equal(eager["pred_logits"], r2["pred_logits"]) and torch.equal(eager["pred_boxes"], r2["pred_boxes"])
    ops = [type(op).__name__ for plan in model._plans.values() for op in plan.ops_backbone]
    assert "VitBlockFewOp" in ops and "MlpFusedOp" not in ops
