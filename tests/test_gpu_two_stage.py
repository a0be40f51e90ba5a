"""GPU: csrc/two_stage_train.hip and lwdetr_amd.ops.two_stage on the cases of two_stage_ref.py.
  - scores: every element of every case in f32 / f16 / bf16 against the float64 restatement under
        |got - ref64| <= max_c [ 4 C 2^-24 M_c + R_c ]        (two_stage_ref.py: M_c, the measured C = C_SCORES, the derived R_c),
    the launch form pinned through lwdetr_two_stage_path_counts (none for the d = 128 fall-back), guard words around `scores`, invalid rows
    of a group bit-equal to each other, a second call bit-identical;
  - top-k: the indices equal a stable descending sort of the operator's own scores, ties among invalid rows by ascending index included;
  - gather / scatter: torch.equal against indexing and against the ascending-g f32 loop, two backward calls bit-identical;
  - whole operator (float32): memory_ts, boxes_ts and the gradients of memory and of every parameter against the float64 restatement on the
    operator's own indices, per tensor max |diff| / max |ref| <= 4 x F32_FIGURE; the class head and unselected rows get exactly zero;
  - patch_two_stage on a stand-in module reproduces the recording of the unmodified reference Transformer (tests/golden/two_stage_train.npz);
  - memory: at B = 1, S = 6800, d = 384, G = 13, nq = 300 the peak above the inputs over forward + backward is under half of the reference loop's.
"""
import os

import pytest
import torch

import two_stage_helpers as H
import two_stage_ref as R
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
WEIGHTS = ("W_eo", "b_eo", "ln_w", "ln_b", "W_cls", "b_cls")


@pytest.fixture(scope="module")
def T():
    from lwdetr_amd import _native
    from lwdetr_amd.ops import two_stage
    _native.lib()
    return two_stage


def device_memory(inp, strided):
    """memory on the device: packed, or the (B, S, d) column view of a wider sentinel-filled buffer (row stride d + 8)."""
    m = inp["memory"]
    if not strided:
        return m.to(DEV)
    B, S, d = m.shape
    buf = torch.full((B, S, d + 8), R.SENT, dtype=m.dtype, device=DEV)
    buf[:, :, :d] = m.to(DEV)
    return buf[:, :, :d]


def raw_scores(inp, mem, ws, out):
    """lwdetr_two_stage_scores through the C ABI into the caller's buffer (so that it can sit between guards)."""
    from lwdetr_amd import _native as N
    B, S, d = mem.shape
    rv = inp["rowvalid"].reshape(-1).to(torch.uint8).to(DEV)
    rc = N.lib().lwdetr_two_stage_scores(mem.data_ptr(), mem.stride(1) if S > 1 else d, rv.data_ptr(), *[w.data_ptr() for w in ws], out.data_ptr(),
                                         B * S, d, inp["case"]["ncls"], inp["case"]["G"], N.dtype_code(mem.dtype), N.stream_ptr(mem.device))
    torch.cuda.synchronize()
    assert rc == 0, rc


SCORE_PARAMS = [pytest.param(c, dt, id=f"{c['name']}-{R.NAME[dt]}") for dt in R.DTYPES for c in R.ALL_SCORE_CASES]


@pytest.mark.parametrize("case,dtype", SCORE_PARAMS)
def test_every_score_against_fp64(T, case, dtype):
    inp = R.make_case(case, dtype)
    s64, M, Rr = R.scores_ref(inp)
    bound = R.score_bound(M, Rr)
    native = T.kernel_supports(case["d"], case["ncls"], case["G"], dtype)
    assert native == (case["d"] != 128)
    mem = device_memory(inp, strided=len(case["levels"]) > 1 or case["d"] == 384)
    ws = [inp[k].to(DEV) for k in WEIGHTS]
    form = {f"ts_scores_{R.NAME[dtype]}_d{case['d']}": 1} if native else {}
    with H.two_stage_served_by(form):
        got = T.two_stage_scores(mem, inp["rowvalid"].to(DEV), *ws)
    G, B, S = case["G"], case["B"], inp["S"]
    assert got.shape == (G, B, S) and got.dtype == torch.float32
    err = (got.cpu().double() - s64).abs()
    worst = float((err / bound).max())
    print(f"{case['name']} {R.NAME[dtype]}: worst |diff| / bound = {worst:.3f}, worst |diff| = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (case["name"], R.NAME[dtype], worst)
    # equal rows get equal bits: every invalid row of a group is the zero row
    inv = ~inp["rowvalid"].reshape(-1)
    if int(inv.sum()) > 1:
        rows = got.cpu().reshape(G, B * S)[:, inv]
        assert torch.equal(rows, rows[:, :1].expand_as(rows))
    if not native:
        return
    # through the ABI into a guarded buffer, twice, with different fills: every element written, nothing outside, the same bits
    for fill in (R.SENT, -7.0):
        buf = torch.full((G * B * S + 2 * GUARD,), fill, dtype=torch.float32, device=DEV)
        with H.two_stage_served_by(form):
            raw_scores(inp, mem, ws, buf[GUARD:GUARD + G * B * S])
        f = torch.full((), fill, dtype=torch.float32, device=DEV)
        assert bool((buf[:GUARD] == f).all()) and bool((buf[-GUARD:] == f).all()), "wrote outside scores"
        assert torch.equal(buf[GUARD:GUARD + G * B * S].view(G, B, S), got)


TOPK_PARAMS = [("two_levels_198_pad", 95), ("all_padding_image", 20), ("r65_g13", 64), ("one_row", 1)]


@pytest.mark.parametrize("name,nq", TOPK_PARAMS)
def test_topk_is_the_stable_sort_of_the_operators_own_scores(T, name, nq):
    case = next(c for c in R.SCORE_CASES if c["name"] == name)
    inp = R.make_case(case, torch.float32)
    scores = T.two_stage_scores(inp["memory"].to(DEV), inp["rowvalid"].to(DEV), *[inp[k].to(DEV) for k in WEIGHTS])
    idx = T.topk_rows(scores, nq)
    assert idx.shape == (case["G"], case["B"], nq) and idx.dtype == torch.int64
    assert torch.equal(idx.cpu(), R.stable_topk(scores.cpu(), nq))
    if name == "all_padding_image":           # image 0: every row ties, so the order is the index order
        assert torch.equal(idx[:, 0].cpu(), torch.arange(nq).expand(case["G"], nq))


SELECT_PARAMS = [pytest.param(c, dt, id=f"{c['name']}-{R.NAME[dt]}") for dt in R.DTYPES for c in R.SELECT_CASES]


@pytest.mark.parametrize("case,dtype", SELECT_PARAMS)
def test_gather_and_scatter_are_exact(T, case, dtype):
    sc = R.make_select_case(case, dtype)
    dt = R.NAME[dtype]
    mem = sc["memory"].to(DEV).requires_grad_(True)
    with H.two_stage_served_by({f"ts_gather_{dt}": 1}):
        x_sel, p_sel = T.SelectRowsFunction.apply(mem, sc["rowvalid"].to(DEV), sc["idx"].to(DEV), sc["props"].to(DEV))
    want_x, want_p = R.gather_ref(sc)
    assert torch.equal(x_sel.cpu(), want_x) and torch.equal(p_sel.cpu(), want_p)
    assert x_sel.requires_grad and not p_sel.requires_grad
    with H.two_stage_served_by({f"ts_scatter_{dt}": 1}):
        x_sel.backward(sc["grad"].to(DEV))
    want_g = R.scatter_ref(sc)
    assert mem.grad.dtype == dtype and torch.equal(mem.grad.cpu(), want_g)
    # without props, and a second backward straight through the ABI wrapper into fresh memory: the same bits
    x2 = T.SelectRowsFunction.apply(mem.detach(), sc["rowvalid"].to(DEV), sc["idx"].to(DEV))
    assert torch.equal(x2, x_sel)
    rv = sc["rowvalid"].to(torch.uint8).to(DEV)
    _, _, inv = T.select_rows_gather(sc["memory"].to(DEV), rv, sc["idx"].to(DEV), sc["props"].to(DEV))
    want_inv = torch.full((case["B"], case["S"], case["G"]), -1, dtype=torch.int32)
    for g in range(case["G"]):
        for b in range(case["B"]):
            want_inv[b, sc["idx"][g, b], g] = torch.arange(case["nq"], dtype=torch.int32)
    assert torch.equal(inv.cpu(), want_inv)
    again = T.select_rows_scatter(sc["grad"].to(DEV), inv, rv)
    assert torch.equal(again, mem.grad)


def _module_on_device(inp, reparam=True):
    case = inp["case"]
    m = H.StandInTransformer(case["d"], case["G"], case["nq"], case["ncls"], bbox_reparam=reparam)
    return H.load_case(m, inp).to(DEV)


def _stacked_grads(m, G):
    z = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    out = dict(g_W_eo=torch.stack([z(m.enc_output[g].weight) for g in range(G)]), g_b_eo=torch.stack([z(m.enc_output[g].bias) for g in range(G)]),
               g_ln_w=torch.stack([z(m.enc_output_norm[g].weight) for g in range(G)]),
               g_ln_b=torch.stack([z(m.enc_output_norm[g].bias) for g in range(G)]))
    for i in range(3):
        out[f"g_W_box{i}"] = torch.stack([z(m.enc_out_bbox_embed[g].layers[i].weight) for g in range(G)])
        out[f"g_b_box{i}"] = torch.stack([z(m.enc_out_bbox_embed[g].layers[i].bias) for g in range(G)])
    return out


@pytest.mark.parametrize("case", R.OP_CASES, ids=lambda c: c["name"])
def test_whole_operator_against_fp64(T, case):
    inp = R.make_case(case, torch.float32)
    m = _module_on_device(inp, case["reparam"])
    mem = inp["memory"].to(DEV).requires_grad_(True)
    mask = None if inp["mask"] is None else inp["mask"].to(DEV)
    G, B, nq, d = case["G"], case["B"], case["nq"], case["d"]
    dt = "f32"
    with H.two_stage_served_by({f"ts_scores_{dt}_d{d}": 1, f"ts_gather_{dt}": 1, f"ts_scatter_{dt}": 1}):
        ref_ts, memory_ts, boxes_ts, idx = T.two_stage_select(mem, mask, case["levels"], m.enc_output, m.enc_output_norm, m.enc_out_class_embed,
                                                              m.enc_out_bbox_embed, nq, G, case["reparam"], return_idx=True)
        assert memory_ts.shape == (B, G * nq, d) and boxes_ts.shape == (B, G * nq, 4)
        assert not ref_ts.requires_grad and torch.equal(ref_ts, boxes_ts.detach())
        fin = torch.isfinite(boxes_ts)
        loss = (memory_ts * inp["go_mem"].to(DEV)).sum() + (torch.where(fin, boxes_ts, torch.zeros_like(boxes_ts)) * inp["go_box"].to(DEV)).sum()
        loss.backward()
    idx = idx.cpu()
    r64 = R.operator_ref(inp, idx)
    got = dict(memory_ts=memory_ts.detach(), boxes_ts=boxes_ts.detach(), g_memory=mem.grad, **_stacked_grads(m, G))
    fails = []
    for t in R.OP_TENSORS:
        fig = R.figure(got[t].cpu(), r64[t])
        print(f"{case['name']} {t}: figure {fig:.3e}, float32 restatement {R.F32_FIGURE[t]:.3e}, ratio {fig / R.F32_FIGURE[t]:.2f}")
        if not fig <= R.MARGIN * R.F32_FIGURE[t]:
            fails.append((t, fig))
    assert not fails, fails
    # the class head decides indices only; rows no group selected, and invalid rows, get exactly zero
    for g in range(G):
        assert m.enc_out_class_embed[g].weight.grad is None and m.enc_out_class_embed[g].bias.grad is None
    hit = torch.zeros(B, inp["S"], dtype=torch.bool)
    for g in range(G):
        hit.scatter_(1, idx[g], True)
    quiet = ~(hit & inp["rowvalid"])
    assert bool(quiet.any()) and torch.equal(mem.grad.cpu()[quiet], torch.zeros(int(quiet.sum()), d))
    # a second forward + backward: the same bits
    first = mem.grad.clone()
    mem.grad = None
    _, m2, b2 = T.two_stage_select(mem, mask, case["levels"], m.enc_output, m.enc_output_norm, m.enc_out_class_embed, m.enc_out_bbox_embed, nq, G,
                                   case["reparam"])
    ((m2 * inp["go_mem"].to(DEV)).sum() + (torch.where(fin, b2, torch.zeros_like(b2)) * inp["go_box"].to(DEV)).sum()).backward()
    assert torch.equal(m2, memory_ts) and torch.equal(mem.grad, first)


def test_patched_module_reproduces_the_reference_recording(T):
    from lwdetr_amd.ops import patch_two_stage
    q, rec = R.load_golden(os.path.join(GOLDEN, "two_stage_train.npz"))
    f = R.golden_floats(q)
    inp = R.golden_inputs(f)
    case = R.GOLDEN_CASE
    G, B, nq, d = case["G"], case["B"], case["nq"], case["d"]
    (h, w), = case["levels"]
    m = _module_on_device(inp)
    keys = list(m.state_dict())
    assert patch_two_stage(m) == 1 and list(m.state_dict()) == keys
    m.train()
    masks = [inp["mask"].view(B, h, w).to(DEV)]
    args = ([f["src"].to(DEV)], masks, [f["pos"].to(DEV)], f["refpoint"].to(DEV), f["query_feat"].to(DEV))
    hs, refs, memory_ts, boxes_ts = m(*args)
    *_, idx = T.two_stage_select(inp["memory"].to(DEV), inp["mask"].to(DEV), case["levels"], m.enc_output, m.enc_output_norm,
                                 m.enc_out_class_embed, m.enc_out_bbox_embed, nq, G, True, return_idx=True)
    assert torch.equal(idx.cpu(), rec["idx"])
    r64 = R.operator_ref(inp, rec["idx"])
    for t, v in (("memory_ts", memory_ts), ("boxes_ts", boxes_ts)):
        fig, fig_rec = R.figure(v.detach().cpu(), r64[t]), R.figure(v.detach().cpu(), rec[t])
        print(f"golden {t}: figure against float64 {fig:.3e}, against the recording {fig_rec:.3e}, float32 restatement {R.F32_FIGURE[t]:.3e}")
        assert fig <= R.MARGIN * R.F32_FIGURE[t] and fig_rec <= (R.MARGIN + 1) * R.F32_FIGURE[t], (t, fig, fig_rec)
    seen = m.decoder.seen
    assert torch.equal(seen["tgt"].cpu(), rec["dec_tgt"]) and torch.equal(seen["memory"].cpu(), inp["memory"])
    assert torch.equal(seen["memory_key_padding_mask"].cpu(), rec["dec_mask"])
    assert torch.equal(seen["pos"].cpu(), f["pos"].flatten(2).transpose(1, 2))
    assert torch.equal(seen["spatial_shapes"].cpu(), rec["dec_spatial_shapes"]) and torch.equal(seen["level_start_index"].cpu(), rec["dec_level_start_index"])
    assert torch.equal(seen["valid_ratios"].cpu(), rec["dec_valid_ratios"])
    assert R.figure(seen["refpoints_unsigmoid"].cpu(), rec["dec_refpoints"].double()) <= (R.MARGIN + 1) * R.F32_FIGURE["boxes_ts"]
    assert not seen["refpoints_unsigmoid"].requires_grad and memory_ts.requires_grad and boxes_ts.requires_grad
    # eval mode: one group, the first group's rows (the caller hands over the first num_queries query rows then, lwdetr.py:150-156)
    m.eval()
    with torch.no_grad():
        _, _, m1, b1 = m(*args[:3], f["refpoint"][:nq].to(DEV), f["query_feat"][:nq].to(DEV))
    assert m1.shape == (B, nq, d) and torch.equal(m1, memory_ts[:, :nq]) and torch.equal(b1, boxes_ts[:, :nq])


def test_peak_memory_is_under_half_of_the_reference_loops(T):
    """B = 1, S = 6800, d = 384, G = 13, nq = 300, f32. Measured on an MI355X: see profiles/r15a_two_stage_train.txt."""
    d, G, nq, ncls, levels = 384, 13, 300, 91, [(80, 85)]
    torch.manual_seed(0)
    m = H.StandInTransformer(d, G, nq, ncls).to(DEV)
    mem = torch.randn(1, 6800, d, device=DEV, requires_grad=True)
    props, valid = T.proposals(1, levels, None, DEV, unsigmoid=False)

    def peak(fn):
        for p in m.parameters():
            p.grad = None
        mem.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        _, mts, bts = fn()
        (mts.sum() + bts.sum()).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    ours = peak(lambda: T.two_stage_select(mem, None, levels, m.enc_output, m.enc_output_norm, m.enc_out_class_embed, m.enc_out_bbox_embed, nq, G,
                                           True))
    theirs = peak(lambda: H.reference_loop(mem, valid, props, m, nq, G, True))
    print(f"peak above the inputs, forward + backward: operator {ours / 2**20:.1f} MiB, reference loop {theirs / 2**20:.1f} MiB")
    assert ours < 0.5 * theirs, (ours, theirs)
