"""CPU: the ABI of the two-stage selection under training (csrc/two_stage_train.hip), its Python layer and the bounds of two_stage_ref.py.
  - the entry points are declared, exported and bound, the launch record has its twelve names, the ops are exported;
  - every refusal of the header returns its code from the _check entries AND from the entries themselves, with made-up pointers and no
    device, and the launch record does not move;
  - kernel_supports is the instantiated range; host tensors raise the documented error;
  - patch_two_stage counts, rebinds, leaves parameters / state-dict keys and a two_stage=False module alone;
  - the float64 restatement reproduces the recording of the unmodified reference Transformer (tests/golden/two_stage_train.npz,
    tools/gen_golden_two_stage.py): indices exactly, values within 4 x the float32 figure, the decoder's inputs;
  - the restatement in float32 is inside the score bound, and its worst ratio IS C_SCORES (measured again, within [0.4, 1.5] x: another build of
    torch's CPU kernels may sum in another order); the same for the whole-operator figures F32_FIGURE;
  - planted mistakes in the restatement leave the bounds: another group's weights, LayerNorm's eps dropped, a descending-g gradient sum.
"""
import ctypes
import os
import re

import pytest
import torch

import two_stage_helpers as H
import two_stage_ref as R
from helpers import GOLDEN, ROOT

SYMBOLS = {"lwdetr_two_stage_scores": 16, "lwdetr_two_stage_scores_check": 15, "lwdetr_two_stage_gather": 15, "lwdetr_two_stage_gather_check": 14,
           "lwdetr_two_stage_scatter_backward": 11, "lwdetr_two_stage_scatter_backward_check": 10, "lwdetr_two_stage_path_counts": 2,
           "lwdetr_two_stage_path_name": 1}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from lwdetr_amd import _native
    return _native


def test_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "lwdetr_hip.h")).read()
    declared = set(re.findall(r"\b(lwdetr_two_stage_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(SYMBOLS)
    raw = ctypes.CDLL(built.LIB_PATH)
    for sym, nargs in SYMBOLS.items():
        assert hasattr(raw, sym), f"{sym} declared in include/lwdetr_hip.h but not exported"
        fn = getattr(built.lib(), sym)
        assert len(fn.argtypes) == nargs and fn.restype is (ctypes.c_char_p if sym.endswith("path_name") else ctypes.c_int), sym
    names = list(built.two_stage_path_counts())
    assert len(names) == len(set(names)) == 12
    for dt in ("f32", "f16", "bf16"):
        assert {f"ts_scores_{dt}_d256", f"ts_scores_{dt}_d384", f"ts_gather_{dt}", f"ts_scatter_{dt}"} <= set(names)
    from lwdetr_amd import ops
    for name in ("two_stage_scores", "SelectRowsFunction", "two_stage_select", "patch_two_stage"):
        assert hasattr(ops, name)


def test_every_refusal_returns_its_code_without_a_device(built):
    """None of these reaches a launch: the pointers are made up."""
    l, BAD, UNS = built.lib(), built.ERR_BAD_ARG, built.ERR_UNSUPPORTED
    before = built.two_stage_path_counts()
    P = [0x10000 * (i + 1) for i in range(10)]           # memory, rowvalid, w_eo, b_eo, ln_w, ln_b, w_cls, b_cls, scores

    def scores(check, ld=256, rows=100, d=256, ncls=91, G=13, dtype=0, null=None, ptr=None):
        p = list(P[:9])
        if null is not None:
            p[null] = None
        if ptr is not None:
            p[ptr[0]] = ptr[1]
        args = (p[0], ld, p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], rows, d, ncls, G, dtype)
        return l.lwdetr_two_stage_scores_check(*args) if check else l.lwdetr_two_stage_scores(*args, None)

    assert scores(True) == 0 and scores(True, d=384, ld=400, ncls=384, G=16, dtype=2) == 0 and scores(True, rows=0) == 0
    for check in (True, False):
        for kw in (dict(d=128), dict(d=320), dict(d=0), dict(ncls=0), dict(ncls=385), dict(G=0), dict(G=17), dict(rows=-1), dict(ld=255),
                   dict(ld=258, dtype=1), dict(ptr=(0, 0x10004)), dict(ptr=(2, 0x30008)), dict(ptr=(8, 0x90002))):
            assert scores(check, **kw) == BAD, (check, kw)
        for i in range(9):
            assert scores(check, null=i) == BAD, (check, i)
        assert scores(check, dtype=3) == UNS and scores(check, dtype=-1) == UNS

    def gather(check, B=2, S=20, G=13, nq=17, d=40, ld=40, dtype=0, null=None, ptr=None):
        p = list(P[:8])                                   # memory, rowvalid, props, idx, x_sel, props_sel, inv
        if null is not None:
            p[null] = None
        if ptr is not None:
            p[ptr[0]] = ptr[1]
        args = (p[0], ld, p[1], p[2], p[3], p[4], p[5], p[6], B, S, G, nq, d, dtype)
        return l.lwdetr_two_stage_gather_check(*args) if check else l.lwdetr_two_stage_gather(*args, None)

    def scatter(check, B=2, S=20, G=13, nq=17, d=40, dtype=0, null=None, ptr=None):
        p = list(P[:4])                                   # grad_x_sel, inv, rowvalid, grad_memory
        if null is not None:
            p[null] = None
        if ptr is not None:
            p[ptr[0]] = ptr[1]
        args = (p[0], p[1], p[2], p[3], B, S, G, nq, d, dtype)
        return l.lwdetr_two_stage_scatter_backward_check(*args) if check else l.lwdetr_two_stage_scatter_backward(*args, None)

    assert gather(True) == 0 and gather(True, nq=20) == 0 and scatter(True) == 0 and scatter(True, nq=1, G=16, dtype=1) == 0
    for check in (True, False):
        for kw in (dict(nq=21), dict(nq=0), dict(B=0), dict(S=0), dict(G=0), dict(G=17), dict(d=0), dict(d=4097)):
            assert gather(check, **kw) == BAD, (check, kw)
            assert scatter(check, **kw) == BAD, (check, kw)
        assert gather(check, ld=39) == BAD and gather(check, ptr=(0, 0x10002)) == BAD and gather(check, ptr=(3, 0x40004)) == BAD
        assert scatter(check, ptr=(1, 0x20002)) == BAD and scatter(check, ptr=(3, 0x40001), dtype=2) == BAD
        for i in range(7):
            assert gather(check, null=i) == BAD, (check, i)
        for i in range(4):
            assert scatter(check, null=i) == BAD, (check, i)
        assert gather(check, dtype=3) == UNS and scatter(check, dtype=7) == UNS
    assert built.two_stage_path_counts() == before


def test_kernel_supports_is_the_instantiated_range(built):
    from lwdetr_amd.ops.two_stage import kernel_supports
    for dt in R.DTYPES:
        for d in (256, 384):
            assert kernel_supports(d, 1, 1, dt) and kernel_supports(d, 384, 16, dt) and kernel_supports(d, 91, 13, dt)
            assert not kernel_supports(d, 0, 1, dt) and not kernel_supports(d, 385, 1, dt)
            assert not kernel_supports(d, 91, 0, dt) and not kernel_supports(d, 91, 17, dt)
        assert not kernel_supports(128, 91, 13, dt) and not kernel_supports(512, 91, 13, dt)
    assert not kernel_supports(256, 91, 13, torch.float64)
    # what the ABI's check says for the same arguments
    l = built.lib()
    for d, ncls, G in ((256, 91, 13), (384, 384, 16), (128, 91, 13), (256, 385, 1), (256, 91, 17)):
        rc = l.lwdetr_two_stage_scores_check(0x10000, d, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000, 10, d, ncls, G, 0)
        assert (rc == 0) == kernel_supports(d, ncls, G, torch.float32)


def test_host_tensors_raise(built):
    from lwdetr_amd.ops import two_stage as T
    inp = R.make_case(R.SCORE_CASES[1], torch.float32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        T.two_stage_scores(inp["memory"], inp["rowvalid"], inp["W_eo"], inp["b_eo"], inp["ln_w"], inp["ln_b"], inp["W_cls"], inp["b_cls"])
    with pytest.raises(RuntimeError, match="ROCm device"):
        T.SelectRowsFunction.apply(inp["memory"], inp["rowvalid"], torch.zeros(2, 1, 3, dtype=torch.int64))
    m = H.StandInTransformer(256, 2, 4, 5)
    with pytest.raises(RuntimeError, match="ROCm device"):
        T.two_stage_select(torch.zeros(1, 6, 256), None, [(2, 3)], m.enc_output, m.enc_output_norm, m.enc_out_class_embed, m.enc_out_bbox_embed,
                           4, 2, True)


def test_patch_counts_and_leaves_the_rest_alone(built):
    from lwdetr_amd.ops import patch_two_stage
    m = H.StandInTransformer(256, 2, 4, 5)
    keys, ptrs = list(m.state_dict()), [p.data_ptr() for p in m.parameters()]
    assert m.forward() == "unpatched"
    assert patch_two_stage(m) == 1
    assert m.forward.__func__.__name__ == "_transformer_forward"
    assert list(m.state_dict()) == keys and [p.data_ptr() for p in m.parameters()] == ptrs
    assert "enc_output.0.weight" in keys and "enc_out_bbox_embed.1.layers.2.bias" in keys and "enc_output_norm.1.weight" in keys
    wrapper = torch.nn.Sequential(H.StandInTransformer(256, 1, 4, 5), torch.nn.Linear(2, 2), H.StandInTransformer(256, 3, 4, 5))
    assert patch_two_stage(wrapper) == 2
    off = H.StandInTransformer(256, 2, 4, 5, two_stage=False)
    assert patch_two_stage(off) == 0 and off.forward() == "unpatched"
    assert patch_two_stage(torch.nn.Linear(3, 3)) == 0
    # the patched forward refuses host tensors like the operator
    with pytest.raises(RuntimeError, match="ROCm device"):
        m([torch.zeros(1, 256, 2, 3)], None, [torch.zeros(1, 256, 2, 3)], torch.zeros(8, 4), torch.zeros(8, 256))


def test_restatement_reproduces_the_reference_recording(built):
    q, rec = R.load_golden(os.path.join(GOLDEN, "two_stage_train.npz"))
    f = R.golden_floats(q)
    inp = R.golden_inputs(f)
    case = R.GOLDEN_CASE
    s64, M, Rr = R.scores_ref(inp)
    idx = R.stable_topk(s64, case["nq"])
    assert torch.equal(idx, rec["idx"])
    # the selection is decided: consecutive gaps among the top nq + 1 above 64 x the bound (what the generator asserted)
    bound = R.score_bound(M, Rr)
    top, order = torch.sort(s64, dim=-1, descending=True, stable=True)
    b_here = torch.gather(bound, -1, order[..., :case["nq"] + 1])
    assert bool((top[..., :case["nq"]] - top[..., 1:case["nq"] + 1] > 64 * torch.maximum(b_here[..., :-1], b_here[..., 1:])).all())
    r64 = R.operator_ref(inp, idx)
    for t in ("memory_ts", "boxes_ts"):
        assert R.figure(rec[t], r64[t]) <= R.MARGIN * R.F32_FIGURE[t], (t, R.figure(rec[t], r64[t]))
    # what the decoder was handed
    B, G, nq = case["B"], case["G"], case["nq"]
    assert bool(rec["dec_memory_is_input"]) and bool(rec["dec_pos_is_input"])
    assert torch.equal(rec["dec_mask"], inp["mask"]) and rec["dec_spatial_shapes"].tolist() == [list(case["levels"][0])]
    assert rec["dec_level_start_index"].tolist() == [0]
    assert torch.equal(rec["dec_tgt"], f["query_feat"].unsqueeze(0).repeat(B, 1, 1))
    bx, rp = rec["boxes_ts"], f["refpoint"].unsqueeze(0).repeat(B, 1, 1)
    want = torch.cat([rp[..., :2] * bx[..., 2:] + bx[..., :2], rp[..., 2:].exp() * bx[..., 2:]], -1)
    assert torch.allclose(rec["dec_refpoints"], want, rtol=1e-6, atol=1e-7)
    assert rec["memory_ts"].shape == (B, G * nq, case["d"]) and rec["boxes_ts"].shape == (B, G * nq, 4)


def test_float32_restatement_is_inside_the_bound_and_is_the_constant(built):
    worst = 0.0
    for case in R.ALL_SCORE_CASES:
        for dt in R.DTYPES:
            inp = R.make_case(case, dt)
            s64, M, Rr = R.scores_ref(inp)
            s32, _, _ = R.scores_ref(inp, torch.float32)
            err = (s32.double() - s64).abs()
            assert bool((err <= R.score_bound(M, Rr)).all()), (case["name"], dt)
            worst = max(worst, float((err / (R.U24 * M.amax(-1))).max()))
    assert 0.4 * R.C_SCORES <= worst <= 1.5 * R.C_SCORES, (worst, R.C_SCORES)
    fig = R.measure_f32_figure()
    for t in R.OP_TENSORS:
        assert 0.4 * R.F32_FIGURE[t] <= fig[t] <= 1.5 * R.F32_FIGURE[t], (t, fig[t], R.F32_FIGURE[t])


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
def test_planted_score_mistakes_leave_the_bound(built, dtype):
    for case in R.ALL_SCORE_CASES:
        inp = R.make_case(case, dtype)
        s64, M, Rr = R.scores_ref(inp)
        bound = R.score_bound(M, Rr)
        if case["G"] > 1:
            bad, _, _ = R.scores_ref(inp, mutate="swap_groups")
            assert bool(((bad - s64).abs() > bound).any()), ("swap_groups", case["name"])
        # LayerNorm without eps: invalid rows (h = the bias alone, variance ~ 0.01) show it in float32; the 16-bit types' derived rounding term is wider
        if dtype == torch.float32 and not bool(inp["rowvalid"].all()):
            bad, _, _ = R.scores_ref(inp, mutate="no_eps")
            assert bool(((bad - s64).abs() > bound).any()), ("no_eps", case["name"])


def test_descending_group_sum_is_caught_by_the_exact_scatter_check(built):
    """In float32: the 16-bit types round the f32 sum once to T, which hides its last bits - there the order is pinned by the kernel's code
    being one template for all three types."""
    caught = 0
    for case in R.SELECT_CASES:
        sc = R.make_select_case(case, torch.float32)
        up, down = R.scatter_ref(sc), R.scatter_ref(sc, descending=True)
        assert torch.equal(up[~sc["rowvalid"]], torch.zeros_like(up[~sc["rowvalid"]]))
        caught += int(not torch.equal(up, down))
    assert caught >= 3                     # every case in which a token is selected by three or more groups
    for dt in R.DTYPES:
        assert R.scatter_ref(R.make_select_case(R.SELECT_CASES[0], dt)).dtype == dt
