"""GPU: the float32 form of lwdetr_gemm_few (few.hip) - PLAIN, CONV3x3 Cin = 128 and Cin = 192 - pinned with the launch-path record and checked
ELEMENT BY ELEMENT against float64 with the comparator and the bound of tests/test_gpu_gemm_paths.py, unchanged (p = 24: half an ulp of the
stored f32 result + 2 (K + 2) 2^-24 sum |a w| + the documented activation slack; guard rows / columns bit-identical); its refusals; GemmOp's
automatic route; and LW-DETR-small / large in fp32 with the plan switch LWDETR_GEMM_FEW_F32 on and unset against the reference goldens."""
import numpy as np
import pytest
import torch

from helpers import case_batch, golden_state_dict, load_golden, served_by
from test_gpu_gemm_paths import (F32, FULL, GELU, RELU, SENT, SILU, WORST, _clear_knobs, _dev, _knobs, _products, _rand,  # noqa: F401
                                 compare, epilogue64, expected, index_linear, run_case)

pytestmark = pytest.mark.gpu
FEW_FAMILIES = ("gemm_few_plain", "gemm_few_conv_kch4", "gemm_few_conv_kch6")

SILU_INPLACE = dict(bias=True, act=SILU, res="inplace")
CONV_A = dict(conv=(1, 12, 11, 128, 1, 32, 224))
CONV_B = dict(conv=(2, 11, 12, 128, 2, 0, 128))
CONV_C = dict(conv=(1, 9, 10, 192, 1, 64, 320))
# family, M, K, segments, extra run_case arguments. PLAIN: M 1 (a single row), 15 / 17 (ragged 16-row tiles, clamped-address rows), 257 (17 tiles);
# K 32 (one chunk: shorter than any batch) and 416 (13 chunks: no batch size divides it, the past-the-end reload runs); N 16 (one wave, the others
# of the workgroup leave early) and 144 (9 column tiles: more than one workgroup owns at any wave count). CONV: every image has border pixels
# on all four sides (the out-of-image taps read the zero source); stride 2, two images, a column offset, Cin 128 and 192.
CASES = [
    ("gemm_few_plain", 1, 32, [dict(n=16, bias=True, act=RELU)], {}),
    ("gemm_few_plain", 15, 416, [dict(n=144, **FULL)], {}),
    ("gemm_few_plain", 17, 416, [dict(n=16, **SILU_INPLACE)], {}),
    ("gemm_few_plain", 257, 416, [dict(n=144, **FULL)], {}),
    ("gemm_few_plain", 257, 32, [dict(n=144, **SILU_INPLACE)], {}),
    ("gemm_few_plain", 17, 32, [dict(n=144, bias=True, act=RELU)], {}),
    ("gemm_few_plain", 1, 416, [dict(n=16, **FULL)], {}),
    ("gemm_few_conv_kch4", 1 * 12 * 11, 9 * 128, [dict(n=96, **FULL)], CONV_A),
    ("gemm_few_conv_kch4", 2 * 6 * 6, 9 * 128, [dict(n=64, bias=True, act=GELU)], CONV_B),
    ("gemm_few_conv_kch6", 1 * 9 * 10, 9 * 192, [dict(n=192, bias=True, act=SILU, res="sep")], CONV_C),
    # waves per workgroup 1 and 8 (the default is 2)
    ("gemm_few_plain", 257, 416, [dict(n=144, **FULL)], dict(force=_knobs(GEMM_FEW_WAVES=1))),
    ("gemm_few_plain", 257, 416, [dict(n=144, **FULL)], dict(force=_knobs(GEMM_FEW_WAVES=8))),
    ("gemm_few_conv_kch4", 1 * 12 * 11, 9 * 128, [dict(n=96, **FULL)], dict(force=_knobs(GEMM_FEW_WAVES=1), **CONV_A)),
    ("gemm_few_conv_kch4", 1 * 12 * 11, 9 * 128, [dict(n=96, **FULL)], dict(force=_knobs(GEMM_FEW_WAVES=8), **CONV_A)),
]


def _id(i, c):
    fam, m, k, segs, extra = c
    return f"{i}-{fam}-M{m}-K{k}-N{segs[0]['n']}" + ("-forced" if extra.get("force") else "")


@pytest.mark.parametrize("case", [pytest.param(c, id=_id(i, c)) for i, c in enumerate(CASES)])
def test_gemm_few_f32_vs_fp64(case):
    family, M, K, segs, extra = case
    run_case(family, F32, M, K, segs, entry="few", **extra)


def test_gemm_few_f32_refusals():
    """lwdetr_gemm_few in f32 answers LWDETR_ERR_UNSUPPORTED before any launch - nothing counted, the output buffer bit-identical - for: a row
    mask, N % 16, columns past N, K = 48, a residual / second destination / output at an 8-byte offset (runs of 4 floats are 16-byte
    accesses), a bias / LayerScale vector at an 8-byte offset, lda % 4 != 0. The same descriptor without the defect is served."""
    from lwdetr_amd import _native, kernels as K
    UNS = _native.ERR_UNSUPPORTED
    run_case(None, F32, 64, 64, [dict(n=32, bias=True, rowmask=0)], entry="few", expect_rc=UNS)
    run_case(None, F32, 64, 64, [dict(n=24, bias=True)], entry="few", expect_rc=UNS)               # ldo = 32: only N % 16 is wrong
    dev = _dev()
    a = _rand((64, 72), F32, 1)
    w = K.pack_frag16(_rand((32, 64), F32, 2))
    flat = torch.full((64 * 48 + 16,), SENT, dtype=F32, device=dev)
    out = flat[:64 * 48].view(64, 48)
    snap = flat.clone()
    store = torch.zeros(64 * 48 + 16, dtype=F32, device=dev)
    store2 = torch.zeros(64 * 48, dtype=F32, device=dev)
    vec = torch.zeros(64, dtype=F32, device=dev)

    def rc_of(*, A=a, W=w, Kd=64, lda=72, o=out, n_end=32, patch=None, **kw):
        op = K.GemmFewOp(A, W, 64, 32, Kd, [K.seg(o, 0, n_end, ldo=48, **kw)], lda=lda, keep=(flat, store, store2, vec))
        if patch:
            setattr(op.desc.seg[0], patch, vec.data_ptr() + 8)
        before = _native.gemm_path_counts()
        rc = op._fn(op._ref, op.dtype, _native.stream_ptr())
        torch.cuda.synchronize()
        return rc, _native.gemm_path_counts() == before, torch.equal(flat, snap)

    def refused(**kw):
        return rc_of(**kw) == (UNS, True, True)

    assert refused(n_end=48)                                           # columns past N
    assert refused(Kd=48, W=torch.zeros(32 * 48, dtype=F32, device=dev))   # K % 32 (the weights are never read)
    assert refused(res=store[2:], ldres=48)                            # residual at an 8-byte offset
    assert refused(out2=store[2:], ld2=48)                             # second destination at an 8-byte offset
    assert refused(o=flat[2:])                                         # output at an 8-byte offset
    assert refused(patch="bias")                                       # 16-byte loads of the vectors
    assert refused(patch="gamma")
    assert refused(lda=70)                                             # A rows off 16-byte alignment
    assert refused(A=a.flatten()[2:])                                  # A at an 8-byte offset
    # the control: the base descriptor (lda = 72, residual / second destination / vectors aligned) is launched and counted
    with served_by("gemm_few_plain"):
        rc, same_counts, same_out = rc_of(res=store, ldres=48, out2=store2, ld2=48, bias=vec, gamma=vec)
    assert rc == 0 and not same_counts and not same_out


def test_gemm_op_routes_f32_to_the_few_row_kernel_only_behind_the_switch(monkeypatch):
    """GemmOp's automatic few-row route in f32: off without LWDETR_GEMM_FEW_F32 (the 64 x 64 kernel serves the launch as before); with it, the few-row
    kernel takes what its entry takes, and a residual with ldres = N + 2 (8-byte rows) stays on the 64 x 64 kernel. All three against float64."""
    from lwdetr_amd import kernels as K
    M, N, Kd = 300, 256, 256
    dev = _dev()
    a, w = _rand((M, Kd), F32, 1), _rand((N, Kd), F32, 2, Kd ** -0.5)
    bias = _rand((N,), F32, 3)
    acc, s = _products(a, w)
    for switch, ldres, family in ((None, N, "gemm_kernel_64x64"), ("1", N + 2, "gemm_kernel_64x64"), ("1", N, "gemm_few_plain")):
        if switch is None:
            monkeypatch.delenv("LWDETR_GEMM_FEW_F32", raising=False)
        else:
            monkeypatch.setenv("LWDETR_GEMM_FEW_F32", switch)
        res = _rand((M, ldres), F32, 4)
        out = torch.full((M + 2, N), SENT, dtype=F32, device=dev)
        snap = out.clone()
        op = K.GemmOp(a, w, M, N, Kd, [K.seg(out, 0, N, ldo=N, bias=bias, act=GELU, res=res, ldres=ldres)], keep=(out, res))
        with served_by(family):
            op()
        y, bnd = epilogue64(acc, s, dtype=F32, K=Kd, bias=bias, act=GELU, res=res[:, :N])
        exp, b = expected(snap, index_linear(M, N, N, dev), y, bnd)
        ok, worst, nbad = compare(out, exp, b)
        assert ok, (switch, family, nbad, worst)
        key = (family + " (GemmOp route)", "float32")
        WORST[key] = max(WORST.get(key, 0.0), worst)


# ---------------------------------------------------------------------------------------------------------------- model level
def _forward_vs_golden(name, monkeypatch, switch):
    """One fp32 forward of the golden case `name` (batch as stored) on a freshly built plan: ({family: launches} of the few-row families,
    op class names of the plan, max |difference| per output tensor against the reference golden - selection teacher-forced where a tie flipped)."""
    import lwdetr_amd
    from lwdetr_amd import _native
    from test_gpu_model import DEV, _diffs, _model
    if switch is None:
        monkeypatch.delenv("LWDETR_GEMM_FEW_F32", raising=False)
    else:
        monkeypatch.setenv("LWDETR_GEMM_FEW_F32", switch)
    monkeypatch.delenv("LWDETR_GEMM_FEW", raising=False)
    g = load_golden(name)
    size, images, mask = case_batch(name)
    model, _ = _model(size, golden_state_dict(g))                    # the plan is built by the first forward, under the environment above
    nt = lwdetr_amd.models.NestedTensor(images.to(DEV), mask.to(DEV))
    before = _native.gemm_path_counts()
    col = {}
    out = model(nt, _collect=col)
    torch.cuda.synchronize()
    after = _native.gemm_path_counts()
    few = {k: after[k] - before[k] for k in FEW_FAMILIES}
    if not np.array_equal(col["topk_idx"].cpu().numpy(), g["topk_idx"]):
        out = model(nt, _forced_topk=torch.from_numpy(g["topk_idx"]).to(DEV))
    ops = [type(op).__name__ for plan in model._plans.values() for grp in (plan.ops_backbone, plan.ops_enc, plan.ops_sel, plan.ops_dec) for op in grp]
    return few, ops, _diffs(out, g)


def test_small_fp32_with_the_switch_on_runs_the_few_row_convolutions_and_meets_the_golden(monkeypatch):
    from test_gpu_model import FP32_TOL
    few, ops, d = _forward_vs_golden("small_640", monkeypatch, "1")
    assert ops.count("GemmFewOp") >= 6, ops.count("GemmFewOp")
    assert few["gemm_few_conv_kch4"] >= 6 and few["gemm_few_conv_kch6"] == 0, few
    print("small_640 fp32, LWDETR_GEMM_FEW_F32=1:", few, d)
    assert max(d.values()) < FP32_TOL, d


def test_small_fp32_with_the_switch_unset_launches_no_few_row_kernel(monkeypatch):
    """No behaviour change: the default fp32 plan has no GemmFewOp and one forward records no launch in the three gemm_few_* families."""
    from test_gpu_model import FP32_TOL
    few, ops, d = _forward_vs_golden("small_640", monkeypatch, None)
    assert "GemmFewOp" not in ops
    assert few == {k: 0 for k in FEW_FAMILIES}, few
    assert max(d.values()) < FP32_TOL, d


def test_large_fp32_with_the_switch_on_runs_the_cin192_form_and_meets_the_golden(monkeypatch):
    from test_gpu_model import FP32_TOL
    few, ops, d = _forward_vs_golden("large_640", monkeypatch, "1")
    assert ops.count("GemmFewOp") >= 6, ops.count("GemmFewOp")
    assert few["gemm_few_conv_kch6"] >= 6 and few["gemm_few_conv_kch4"] == 0, few
    print("large_640 fp32, LWDETR_GEMM_FEW_F32=1:", few, d)
    assert max(d.values()) < FP32_TOL, d
