"""GPU: the float32 form of lwdetr_vit_block_few (mlp_small_kernel<float, QKV, 1, true>, mlp.hip) against float64 - residual stream, tap copy, row
statistics, chained q / k / v^T - under the float32 bounds of test_gpu_kernels.py::test_mlp_fused; element-wise against the error of today's f32
lwdetr_mlp_fused kernel on the same operands; determinism; the entry's refusals; and LW-DETR-small / tiny in fp32 with the plan switch
LWDETR_VIT_BLOCK_FEW_F32 on and unset against the reference goldens. TT = 2 is not built in f32 (LWDETR_MLP_SMALL_TT is ignored), so there is no TT case.
Every launch is pinned to its instantiation by the launch-form record (helpers.mlp_served_by); the per-element bounds are in tests/test_gpu_mlp_fp64.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import case_batch, golden_state_dict, load_golden, mlp_served_by
from test_gpu_kernels import _dev, _rand, _relerr

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
C = 192
SENT = 7.0
# (M, Tp, heads): one lane group of one tile; a ragged second tile (clamped-address rows); an image boundary inside a tile, hd 32; hd 64, full tiles;
# 13 tiles with images that straddle tiles; the first row count above MLP_SMALL_TT1_MAX_ROWS (the 16-bit kernel changes its tile there, f32 must not)
SHAPES = [(4, 4, 12), (20, 20, 12), (40, 20, 6), (48, 16, 3), (208, 52, 12), (3216, 1608, 12)]
QSCALE = 0.37
_CACHE = {}


def _case(m, tp, heads):
    """Operands drawn as in test_vit_block_few_fragment_major_weights, their float32 packing, and the float64 reference - once per shape, never modified."""
    key = (m, tp, heads)
    if key in _CACHE:
        return _CACHE[key]
    from lwdetr_amd import kernels as K
    c, hd, nb = C, C // heads, m // tp
    o = dict(m=m, tp=tp, heads=heads, hd=hd, nb=nb)
    o["x"] = _rand(m, c, seed=1) * 2 + 0.3
    o["att"] = _rand(m, c, seed=9)
    w1, b1 = _rand(4 * c, c, scale=c ** -0.5, seed=2), _rand(4 * c, seed=3) * 0.1
    w2, o["b2"] = _rand(c, 4 * c, scale=(4 * c) ** -0.5, seed=4), _rand(c, seed=5) * 0.1
    lw, lb = _rand(c, seed=6) * 0.2 + 1, _rand(c, seed=7) * 0.1
    o["g2"], o["g1"] = _rand(c, seed=8) * 0.3, _rand(c, seed=12) * 0.3
    wp, o["bp"] = _rand(c, c, scale=c ** -0.5, seed=10), _rand(c, seed=11) * 0.1
    wqkv = _rand(3 * c, c, scale=c ** -0.5, seed=13)
    qb, vb = _rand(c, seed=14) * 0.1, _rand(c, seed=15) * 0.1
    lw1, lb1 = _rand(c, seed=16) * 0.2 + 1, _rand(c, seed=17) * 0.1
    o["w1p"], o["b1p"], o["w2p"] = K.pack_mlp_weights(w1, b1, w2, lw, lb, F32, proj=True)
    o["wq"], o["bq"] = K.pack_qkv_weights(wqkv, qb, vb, lw1, lb1, F32)
    o["wp"] = wp.contiguous()
    o["w1F"], o["wpF"], o["wqF"] = K.pack_frag16(o["w1p"]), K.pack_frag16(o["wp"]), K.pack_frag16(o["wq"])
    d = lambda t: t.double()
    x1 = d(o["x"]) + d(o["g1"]) * (d(o["att"]) @ d(wp).t() + d(o["bp"]))                  # f32 is the storage type: x1 is not rounded
    ref = x1 + d(o["g2"]) * (F.gelu(F.layer_norm(x1, (c,), d(lw), d(lb), 1e-6) @ d(w1).t() + d(b1)) @ d(w2).t() + d(o["b2"]))
    y = F.layer_norm(ref, (c,), d(lw1), d(lb1), 1e-6) @ d(wqkv).t() + torch.cat([d(qb), torch.zeros_like(d(qb)), d(vb)])
    sp = lambda t_: t_.reshape(nb, tp, heads, hd).permute(0, 2, 1, 3)
    o["ref"] = dict(x=ref, q=(sp(y[:, :c]) * QSCALE).contiguous(), k=sp(y[:, c:2 * c]).contiguous(), vt=sp(y[:, 2 * c:]).transpose(2, 3).contiguous())
    _CACHE[key] = o
    return o


def _buffers(o, pad=16):
    """Fresh outputs with sentinel guards: `pad` rows behind x / taps / stats, `pad` elements behind q / k / v^T, the left half of the tap buffer."""
    m, dev, n = o["m"], _dev(), o["nb"] * o["heads"] * o["tp"] * o["hd"]
    b = dict(x=torch.full((m + pad, C), SENT, dtype=F32, device=dev), taps=torch.full((m + pad, 2 * C), SENT, dtype=F32, device=dev),
             stats=torch.full((m + pad, 2), SENT, dtype=F32, device=dev))
    b["x"][:m] = o["x"]
    for nme in ("q", "k", "vt"):
        b[nme + "_flat"] = torch.full((n + pad,), SENT, dtype=F32, device=dev)
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
    with mlp_served_by(f"mlp_small_f32_tt1_qkv{int(qkv)}_frag1" if few else f"mlp_f32_c192_proj1_qkv{int(qkv)}"):
        cls(b["x"], o["w1F"] if few else o["w1p"], o["b1p"], o["w2p"], o["b2"], o["g2"], o["m"], C, 1e-6, **kw)()
    torch.cuda.synchronize()


def _sentinel(t):
    return bool((t == SENT).all())


@pytest.mark.parametrize("extras", [True, False], ids=["tap+stats", "bare"])
@pytest.mark.parametrize("qkv", [True, False], ids=["qkv", "noqkv"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%d-Tp%d-h%d" % s)
def test_vit_block_few_f32_vs_fp64(shape, qkv, extras):
    o = _case(*shape)
    m = o["m"]
    b = _buffers(o)
    _run(o, b, qkv=qkv, extras=extras)
    r = o["ref"]
    ex = _relerr(b["x"][:m].double(), r["x"])
    print(f"{shape} qkv={qkv} extras={extras}: relerr x {ex:.3e}", end="")
    assert ex < 3e-5, ex
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
            assert e < 6e-5, (nme, e)
            assert _sentinel(b[nme + "_flat"][n:]), nme
    else:
        assert all(_sentinel(b[nme + "_flat"]) for nme in ("q", "k", "vt"))
    print()


@pytest.mark.parametrize("shape", [(208, 52, 12), (3216, 1608, 12)], ids=lambda s: "M%d-Tp%d-h%d" % s)
def test_vit_block_few_f32_error_is_that_of_the_fused_f32_kernel(shape):
    """Element-wise yardstick that is not the code under test: lwdetr_mlp_fused in float32 (mlp_kernel<float, 192>, row-major weights) on the same
    operands. Both kernels sum the same f32 products in different orders, so their worst elements against float64 over >= 10^4 outputs per tensor
    (the two shapes with M * C >= 39 936) differ by far less than 2x; more is a wrong operand. Figures: profiles/r7b_vit_block_few_f32.txt."""
    o = _case(*shape)
    m, r = o["m"], o["ref"]
    new, old = _buffers(o), _buffers(o)
    _run(o, new, few=True)
    _run(o, old, few=False)
    for nme in ("x", "q", "k", "vt"):
        a, y = (new[nme][:m], old[nme][:m]) if nme == "x" else (new[nme], old[nme])
        assert a.numel() >= 10 ** 4
        e_new = (a.double() - r[nme]).abs().max().item()
        e_old = (y.double() - r[nme]).abs().max().item()
        print(f"{shape} {nme}: max|err| vs fp64  vit_block_few f32 {e_new:.3e}   mlp_fused f32 {e_old:.3e}   ratio {e_new / e_old:.2f}")
        assert e_old > 0 and e_new <= 2 * e_old, (nme, e_new, e_old)


def test_vit_block_few_f32_is_deterministic():
    o = _case(208, 52, 12)
    a, b = _buffers(o), _buffers(o)
    _run(o, a)
    _run(o, b)
    for nme in ("x", "taps", "stats", "q_flat", "k_flat", "vt_flat"):
        assert torch.equal(a[nme], b[nme]), nme


def test_vit_block_few_f32_refusals():
    """lwdetr_vit_block_few with dtype 0 answers LWDETR_ERR_UNSUPPORTED before any launch - every output bit-identical to a snapshot - for x / att /
    out2 / q at an 8-byte offset, ldx = 194, a bias vector at an 8-byte offset, C = 384 and M = 12 800; the same call without the defect returns 0 and
    changes the output. (x / att hold 12 800 rows here, so that no argument set of this test describes memory that is not there.)"""
    from lwdetr_amd import _native, kernels as K
    UNS = _native.ERR_UNSUPPORTED
    o = _case(208, 52, 12)
    dev, m, big = _dev(), o["m"], 12800
    n = o["nb"] * o["heads"] * o["tp"] * o["hd"]
    xs = torch.full((big * C + 8,), SENT, dtype=F32, device=dev)
    atts = torch.zeros(big * C + 8, dtype=F32, device=dev)
    taps = torch.full((big * 2 * C + 8,), SENT, dtype=F32, device=dev)
    stats = torch.full((big, 2), SENT, dtype=F32, device=dev)
    qs, ks, vs = (torch.full((big * C + 8,), SENT, dtype=F32, device=dev) for _ in range(3))
    vec = torch.zeros(3 * C + 8, dtype=F32, device=dev)
    xs[:m * C] = o["x"].flatten()
    atts[:m * C] = o["att"].flatten()
    outs = (xs, taps, stats, qs, ks, vs)
    snap = [t.clone() for t in outs]

    def call(*, x_off=0, att_off=0, tap_off=0, q_off=0, ldx=C, bp=o["bp"], c=C, rows=m, tp=o["tp"]):
        nq = rows * C
        op = K.MlpFusedOp(xs[x_off:], o["w1F"], o["b1p"], o["w2p"], o["b2"], o["g2"], rows, c, 1e-6, ldx=ldx, out2=taps[C + tap_off:], ld2=2 * C,
                          stats_out=stats, att=atts[att_off:], ldatt=C, wp=o["wpF"], bp=bp, gamma1=o["g1"], wqkv=o["wqF"], bqkv=o["bq"],
                          q=qs[q_off:q_off + nq], k=ks[:nq], vt=vs[:nq], qscale=QSCALE, heads=c // 16, hd=16, Tp=tp)
        rc = _native.lib().lwdetr_vit_block_few(*op.args, _native.stream_ptr())
        torch.cuda.synchronize()
        return rc, all(torch.equal(t, s) for t, s in zip(outs, snap))

    assert call(x_off=2) == (UNS, True)                              # 8-byte offsets: 16-byte accesses of 4 floats
    assert call(att_off=2) == (UNS, True)
    assert call(tap_off=2) == (UNS, True)
    assert call(q_off=2) == (UNS, True)
    assert call(ldx=194) == (UNS, True)
    assert call(bp=vec[2:2 + C]) == (UNS, True)
    assert call(c=384) == (UNS, True)
    assert call(rows=12800, tp=400) == (UNS, True)
    assert n == m * C
    with mlp_served_by("mlp_small_f32_tt1_qkv1_frag1"):
        rc, same = call()                                            # the control
    assert rc == 0 and not same
    assert _relerr(xs[:m * C].view(m, C).double(), o["ref"]["x"]) < 3e-5
    assert _sentinel(xs[m * C:]) and _sentinel(qs[n:])


# ---------------------------------------------------------------------------------------------------------------- model level
def _forward_vs_golden(name, monkeypatch, switch, gemm_few=None):
    """One fp32 forward of the golden case `name` (batch as stored) on a freshly built plan: (op class names of the plan, depth of the ViT, max |difference|
    per output tensor against the reference golden - selection teacher-forced where a tie flipped)."""
    import lwdetr_amd
    from test_gpu_model import DEV, _diffs, _model
    for var, val in (("LWDETR_VIT_BLOCK_FEW_F32", switch), ("LWDETR_GEMM_FEW_F32", gemm_few)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    for var in ("LWDETR_MLP_FUSED", "LWDETR_VIT_BLOCK_FEW", "LWDETR_GEMM_FEW", "LWDETR_MLP_SMALL_TT"):
        monkeypatch.delenv(var, raising=False)
    g = load_golden(name)
    size, images, mask = case_batch(name)
    model, _ = _model(size, golden_state_dict(g))                    # the plan is built by the first forward, under the environment above
    nt = lwdetr_amd.models.NestedTensor(images.to(DEV), mask.to(DEV))
    col = {}
    out = model(nt, _collect=col)
    torch.cuda.synchronize()
    if not np.array_equal(col["topk_idx"].cpu().numpy(), g["topk_idx"]):
        out = model(nt, _forced_topk=torch.from_numpy(g["topk_idx"]).to(DEV))
    plans = list(model._plans.values())
    ops = [type(op).__name__ for plan in plans for grp in (plan.ops_backbone, plan.ops_enc, plan.ops_sel, plan.ops_dec) for op in grp]
    return ops, plans[0].depth * len(plans), _diffs(out, g)


@pytest.mark.parametrize("name,gemm_few", [("small_640", None), ("small_640", "1"), ("small_padded", None), ("tiny_192x256", None)])
def test_fp32_model_with_the_switch_on_runs_one_block_launch_per_vit_block_and_meets_the_golden(name, gemm_few, monkeypatch):
    from test_gpu_model import FP32_TOL
    ops, depth, d = _forward_vs_golden(name, monkeypatch, "1", gemm_few)
    assert ops.count("VitBlockFewOp") == depth and depth > 0, (ops.count("VitBlockFewOp"), depth)
    assert "MlpFusedOp" not in ops
    assert ("GemmFewOp" in ops) == (gemm_few == "1")
    print(f"{name} fp32, LWDETR_VIT_BLOCK_FEW_F32=1, LWDETR_GEMM_FEW_F32={gemm_few}:", d)
    assert max(d.values()) < FP32_TOL, d


def test_small_fp32_with_the_switch_unset_builds_no_block_launch(monkeypatch):
    """No behaviour change: the default fp32 plan has neither VitBlockFewOp nor MlpFusedOp (seven launches per block) and meets the golden as before."""
    from test_gpu_model import FP32_TOL
    ops, _, d = _forward_vs_golden("small_640", monkeypatch, None)
    assert "VitBlockFewOp" not in ops and "MlpFusedOp" not in ops
    assert max(d.values()) < FP32_TOL, d


def test_fp32_capture_with_the_switch_on_replays_bit_identically(monkeypatch):
    """model.capture on one fp32 image with the switch on: two replays equal each other and the eager call bit for bit."""
    from test_gpu_model import DEV, _model
    monkeypatch.setenv("LWDETR_VIT_BLOCK_FEW_F32", "1")
    for var in ("LWDETR_MLP_FUSED", "LWDETR_VIT_BLOCK_FEW", "LWDETR_GEMM_FEW_F32"):
        monkeypatch.delenv(var, raising=False)
    g = load_golden("small_640")
    size, images, _ = case_batch("small_640")
    model, _ = _model(size, golden_state_dict(g))
    one = images[:1].to(DEV)
    graphed = model.capture(one)
    r1 = {k: v.clone() for k, v in graphed(one).items() if isinstance(v, torch.Tensor)}
    r2 = graphed(one)
    assert torch.equal(r1["pred_logits"], r2["pred_logits"]) and torch.equal(r1["pred_boxes"], r2["pred_boxes"])
    eager = model(one)
    assert torch.equal(eager["pred_logits"], r2["pred_logits"]) and torch.equal(eager["pred_boxes"], r2["pred_boxes"])
    ops = [type(op).__name__ for plan in model._plans.values() for op in plan.ops_backbone]
    assert "VitBlockFewOp" in ops and "MlpFusedOp" not in ops
