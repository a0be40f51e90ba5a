"""GPU: ForwardPlan's fused plan - the one bench.py times: stem launch, VitBlockOp, encoder chain, row chains, fused FFN (float32: lwdetr_mlp_fused) -
at the shapes of tests/plan_shapes_cases.py: windows with pad tokens (Twp != Tw), non-square maps, padding masks at B >= 8, odd batches, images whose
first token row falls inside a 128-row tile, LWDETR_ARENA=1. Every other model-level test reaches that plan at 640 x 640 dense even batches only, and the
per-kernel fp64 suites build their own descriptors: an `ld`, a row offset, a `sub_len`, a pad row read as a key, a halo read across an image boundary or
a buffer that is only right because it was zero-filled when the plan was built would pass all of them.

Per case (one model, shared by the case's tests; dense batches run as ONE launch chain here - models.lwdetr.set_streams(1) - so that B images make
B * Tp rows of one plan, as a forced or masked call does anyway):
  (a) the intended plan ran, and which kernel instantiations served it (plan_shapes_forms.json in the records directory, tracked: profiles/plan_shapes_forms.json);
  (b) arithmetic against oracle/lwdetr_torch.py in float32 on the case's two distinct images (selection forced to the oracle's), for EVERY batch slot:
      the tapped ViT blocks at real tokens, memory, the class maxima, every decoder layer, all logits and boxes. The bound is no fixed number: it is what
      the reference's own arithmetic costs in the case's 16-bit dtype on the same images (helpers.oracle_lowp), times 1.5 (the project's factor,
      tests/test_gpu_baseline_configs.py), for the max AND the mean of |error| (plan_shapes_ratios.json in the records directory, tracked:
      profiles/plan_shapes_ratios.txt). The bfloat16 yardstick is WIDE at the outputs (max |bf16 - fp32| of the logits of a small model is 0.8 at
      704 x 704): in the bfloat16 cases the mean columns and the front stages (ViT taps, memory), where the reference's own error is still small,
      carry the weight; tests/test_plan_shapes_host.py shows which planted wiring mistakes the comparator sees. float32 (s320f): the bounds of
      test_fp32_stages_match_oracle, and for the un-normalised ViT taps its memory bound relative to the taps' scale. Free-running: the selected set
      against the oracle's, all outputs finite;
  (c) images do not see each other: with every other slot replaced (other pixels, the other valid size), slot j's rows of every output and collected
      tensor are bit-identical - j = 0, a slot that starts inside a 128-row tile, B - 1;
  (d) nothing depends on what the buffers held: every floating-point buffer of the plan that a kernel writes filled with +30000 / -30000 (finite on
      purpose: the value tests/test_gpu_attention_fp64.py puts into unusable K rows and V^T columns), then the same bits again;
  (e) the padding state of a cached plan: padded A, dense, padded B, padded A, list of equal-sized tensors;
  (f) LWDETR_ARENA=1 gives the same bits as the default allocation;
  (g) replicas of an image in the forced run agree within a quarter of the case's 16-bit logit yardstick."""
import json
import os
import time
from collections import Counter

import numpy as np
import pytest
import torch

import lwdetr_amd
import plan_shapes_cases as P
from helpers import ROOT, oracle_run
from plan_shapes_cases import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the records directory: where a run leaves its measured figures (LWDETR_TEST_RECORDS; default build/test_records, which git ignores)
OUT = os.environ.get("LWDETR_TEST_RECORDS") or os.path.join(ROOT, "build", "test_records")


@pytest.fixture(scope="module", autouse=True)
def one_launch_chain():
    from lwdetr_amd.models import lwdetr as M
    before = M._STREAMS
    M.set_streams(1)
    yield
    M.set_streams(before)


def _record(fname, key, value):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, fname)
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data.setdefault(key, {}).update(value)
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def _counts():
    from lwdetr_amd import _native as N
    c = {}
    for fam in ("vit", "attn", "chain", "mlp", "msda", "gemm"):
        c.update({f"{fam}:{k}": v for k, v in getattr(N, fam + "_path_counts")().items()})
    return c


class Ctx:
    def __init__(self, case):
        from lwdetr_amd.configs import VIT_SIZES
        from lwdetr_amd.synth import synth_state_dict
        self.case, self.dtype = case, P.dtype_of(case)
        self.cfg = lwdetr_amd.get_args(case.size)
        self.geo = P.plan_geometry(case.size, case.H, case.W)
        self.C = VIT_SIZES[self.cfg.encoder][0]
        self.x2, self.mask2 = P.case_images(case)                                  # the two distinct images (CPU, f32)
        t0 = time.time()
        self.ref32, self.c32 = oracle_run(case.size, self.x2, self.mask2, torch.float32)
        self.oracle_s = time.time() - t0
        self.t32 = P.oracle_tensors(self.ref32, self.c32, self.geo)
        self._yard = None
        self.x = P.tile(self.x2, case.B).to(DEV).to(self.dtype)
        self.mask = None if self.mask2 is None else P.tile(self.mask2, case.B).to(DEV)
        self.forced = P.tile(torch.from_numpy(self.ref32["topk_idx"]), case.B).to(DEV)
        self.model = self.new_model()
        self._forced_run = self._free_run = None

    @property
    def yard(self):
        """The yardstick: the reference's own arithmetic in the case's 16-bit dtype on the same two images, same (forced) selection; None in float32.
        Computed where it is first needed, (b): the two CPU runs of a case then fall into two tests."""
        if self._yard is None and self.dtype != torch.float32:
            t0 = time.time()
            ref16, c16 = oracle_run(self.case.size, self.x2, self.mask2, self.dtype, forced_topk=self.ref32["topk_idx"])
            self.lowp_s = time.time() - t0
            self._yard = P.yardstick(self.t32, P.oracle_tensors(ref16, c16, self.geo))
        return self._yard

    def new_model(self):
        from lwdetr_amd.synth import synth_state_dict
        model, _, _ = lwdetr_amd.build_model(self.cfg)
        model.load_state_dict(synth_state_dict(model.state_dict(), seed=0))
        return model.to(DEV).to(self.dtype).eval()

    def call(self, x=None, mask="case", forced=None, model=None):
        """One model call -> (output dict, collected tensors): a padded batch goes in as NestedTensor, a dense one as a tensor."""
        x = self.x if x is None else x
        mask = self.mask if isinstance(mask, str) else mask
        col = {}
        samples = x if mask is None else lwdetr_amd.models.NestedTensor(x, mask)
        out = (model or self.model)(samples, _forced_topk=forced, _collect=col)
        torch.cuda.synchronize()
        assert col.pop("launch_chains") == 1
        return out, col

    def plan(self, model=None):
        plans = list((model or self.model)._plans.values())
        assert len(plans) == 1 and (plans[0].B, plans[0].H, plans[0].W) == (self.case.B, self.case.H, self.case.W)
        return plans[0]

    def forced_run(self):
        if self._forced_run is None:
            before = _counts()
            out, col = self.call(forced=self.forced)
            after = _counts()
            self.forms = {k: after[k] - before[k] for k in after if after[k] != before[k]}
            self._forced_run = (out, col)
        return self._forced_run

    def free_run(self):
        if self._free_run is None:
            self._free_run = self.call()
        return self._free_run


_CTXS = {}          # case id -> Ctx: one model (and one pair of oracle runs) per case, shared by the case's tests, dropped with the module


@pytest.fixture(scope="module", autouse=True)
def drop_contexts():
    yield
    for c in _CTXS.values():
        c.model.invalidate_cache()
    _CTXS.clear()
    torch.cuda.empty_cache()


@pytest.fixture
def ctx(request):
    case = request.param
    if case.id not in _CTXS:
        _CTXS[case.id] = Ctx(case)
    return _CTXS[case.id]


def cases(ids=None):
    sel = CASES if ids is None else [P.BY_ID[i] for i in ids]
    return pytest.mark.parametrize("ctx", sel, indirect=True, ids=[c.id for c in sel])


def _flat(ctx, out, col):
    """Every output and collected tensor of a call, batch first."""
    g, B = ctx.geo, ctx.case.B
    t = {"pred_logits": out["pred_logits"], "pred_boxes": out["pred_boxes"], "enc_logits": out["enc_outputs"]["pred_logits"],
         "enc_boxes": out["enc_outputs"]["pred_boxes"]}
    for j, a in enumerate(out["aux_outputs"]):
        t[f"aux{j}_logits"], t[f"aux{j}_boxes"] = a["pred_logits"], a["pred_boxes"]
    t.update({"topk_idx": col["topk_idx"], "enc.class_max": col["enc.class_max"], "memory": col["memory"], "om": col["om"],
              "hs": col["hs"].view(g["nl"], B, g["nq"], g["d"]).transpose(0, 1), "taps_cat": col["taps_cat"].view(B, g["Tp"], -1),
              "x": col["x"].view(B, g["Tp"], -1)})
    assert all(v.shape[0] == B for v in t.values())
    return t


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _differences(a, b, slot=None):
    """Names (with the share of differing elements) of the tensors of two _flat dicts that are not bit-identical (``slot``: on that image's rows)."""
    bad = []
    for k in a:
        u, v = (a[k], b[k]) if slot is None else (a[k][slot], b[k][slot])
        if not torch.equal(_bits(u), _bits(v)):
            ne = (u != v)
            rows = ne.reshape(ne.shape[0], -1).any(1).nonzero().flatten().tolist() if ne.dim() > 1 else []
            bad.append(f"{k}: {int(ne.sum())} of {ne.numel()} elements differ (first rows {rows[:6]})")
    return bad


# ----------------------------------------------------------------------------------------------------- (a)
@cases()
def test_the_intended_plan_ran(ctx):
    from lwdetr_amd import kernels as K
    ctx.forced_run()
    plan, case = ctx.plan(), ctx.case
    assert (plan.Tw, plan.Twp, plan.Tp, plan.rows) == (case.Tw, case.Twp, case.Tp, case.rows)
    assert (plan.Hp, plan.Wp, plan.S, plan.lsi, plan.level_hw) == (ctx.geo["Hp"], ctx.geo["Wp"], ctx.geo["S"], ctx.geo["lsi"], ctx.geo["level_hw"])
    back = [type(op).__name__ for op in plan.ops_backbone]
    if ctx.dtype == torch.float32:
        assert back.count("MlpFusedOp") == plan.depth, back
        assert not plan.use_chain and plan.stem_op is None and "VitBlockOp" not in back
        assert not any(isinstance(op, (K.EncChainOp, K.RowChainOp)) for op in plan.ops_enc + plan.ops_sel + plan.ops_dec)
    else:
        assert plan.stem_op is not None
        assert back.count("VitBlockOp") == plan.depth and "MlpFusedOp" not in back, back
        assert plan.use_chain and any(isinstance(op, K.EncChainOp) for op in plan.ops_enc)
        if plan.d == 256:
            assert any(isinstance(op, K.RowChainOp) for op in plan.ops_dec)
    assert (plan._pad_state == "pad") == (case.valid is not None)
    assert ctx.forms, "no launch was recorded"
    _record("plan_shapes_forms.json", case.id, ctx.forms)


# ----------------------------------------------------------------------------------------------------- (b)
@cases()
def test_arithmetic_against_the_reference_formulation(ctx):
    case, geo = ctx.case, ctx.geo
    out, col = ctx.forced_run()
    assert torch.equal(col["topk_idx"].cpu(), ctx.forced.cpu())
    ours = P.plan_tensors(out, col, geo, ctx.C)
    assert set(ours) == set(ctx.t32) and all(ours[k].shape[1:] == ctx.t32[k].shape[1:] and ours[k].shape[0] == case.B for k in ours)
    assert all(np.isfinite(v).all() for v in ours.values())
    if ctx.dtype == torch.float32:
        rec, bad = {}, []
        for k, ref in ctx.t32.items():
            err = float(np.abs(ours[k] - ref[np.arange(case.B) % 2]).max())
            if k.startswith("vit.block"):          # un-normalised residual stream: the memory bound (a unit-scale LayerNorm output) relative to its scale
                bound = P.F32_BOUNDS["front"] * max(1.0, float(np.abs(ref).max()))
            else:
                bound = P.F32_BOUNDS["front"] if k in ("memory", "enc.class_max") else P.F32_BOUNDS["back"]
            rec[k] = {"err_max": err, "bound": bound}
            if not err < bound:
                bad.append((k, err, bound))
        print(case.id, json.dumps(rec))
        _record("plan_shapes_ratios.json", case.id, {"float32_abs": rec, "oracle_seconds": round(ctx.oracle_s, 2)})
        assert not bad, bad
    else:
        r = P.ratios(ours, ctx.t32, ctx.yard)
        print(case.id, json.dumps(r))
        _record("plan_shapes_ratios.json", case.id, {"ratios": r, "worst": list(P.worst(r)), "oracle_seconds": round(ctx.oracle_s, 2),
                                                     "oracle_16bit_seconds": round(ctx.lowp_s, 2)})
        bad = [(k, c, v[c], v["slot_" + c]) for k, v in r.items() for c in ("max", "mean") if not v[c] <= P.RATIO]
        assert not bad, f"ours > {P.RATIO} x the reference's own {case.dtype} error: (tensor, column, ratio, slot) {bad}"


@cases()
def test_free_running_selection(ctx):
    out, col = ctx.free_run()
    ours, ref = col["topk_idx"].cpu().numpy(), ctx.ref32["topk_idx"]
    assert ours.shape == (ctx.case.B, ctx.geo["nq"]) and ours.min() >= 0 and ours.max() < ctx.geo["S"]
    # Rows of padded / invalid cells have bit-identical scores in the oracle (their enc_output input row is zeroed): where the cut of the top-k falls into
    # such a tie (m448p, image 1: 416 tied rows, 125 of them selected; the reference's own bfloat16 run picks a set that overlaps 0.61 there), WHICH of
    # the tied rows are taken is arbitrary, as in test_fp32_matches_reference_golden. Tied rows count as one class, each pick of it once (a multiset
    # overlap); without ties this is the plain set overlap.
    sc = ctx.c32["enc.class_max"]
    per = []
    for k, a in enumerate(ours):
        first = {}
        cls = np.array([first.setdefault(v, i) for i, v in enumerate(sc[k % 2].tolist())])      # row -> first row with the same fp32 score
        per.append(sum((Counter(cls[a].tolist()) & Counter(cls[ref[k % 2]].tolist())).values()) / ref.shape[1])
    overlap = np.mean(per)
    plain = np.mean([len(set(a) & set(ref[k % 2])) / ref.shape[1] for k, a in enumerate(ours)])
    _record("plan_shapes_ratios.json", ctx.case.id, {"topk_set_overlap": float(overlap), "topk_set_overlap_min_image": float(min(per)),
                                                     "topk_set_overlap_ignoring_ties": float(plain)})
    assert overlap > 0.9, overlap
    for k, v in _flat(ctx, out, col).items():
        assert k == "topk_idx" or torch.isfinite(v.float()).all(), k


# ----------------------------------------------------------------------------------------------------- (g)
@cases()
def test_replicas_agree(ctx):
    out, _ = ctx.forced_run()
    lg = out["pred_logits"].float()
    for i in range(2):
        if ctx.yard is None:
            bound = P.F32_BOUNDS["back"] / 4
        else:
            bound = max(ctx.yard["pred_logits"]["max"][i], ctx.yard["enc_logits"]["max"][i]) / 4
        spread = max((lg[k] - lg[i]).abs().max().item() for k in range(i + 2, ctx.case.B, 2))
        _record("plan_shapes_ratios.json", ctx.case.id, {f"replica_spread_image{i}": {"spread": spread, "bound": float(bound)}})
        assert spread <= bound, (i, spread, bound)


# ----------------------------------------------------------------------------------------------------- (c)
@cases()
def test_images_do_not_see_each_other(ctx):
    case = ctx.case
    base = _flat(ctx, *ctx.free_run())
    ox2, om2 = P.case_images(case, seed=case.seed + 1000, swap=True)               # other pixels; padded cases: the other valid size in every slot
    other_x = P.tile(ox2, case.B).to(DEV).to(ctx.dtype)
    other_m = None if om2 is None else P.tile(om2, case.B).to(DEV)
    inside = [j for j in range(1, case.B - 1) if (j * case.Tp) % 128 != 0]         # first token row in the middle of a 128-row tile
    slots = [0, inside[len(inside) // 2] if inside else case.B // 2, case.B - 1]
    assert (case.Tp % 128 == 0) == (not inside) and len(set(slots)) == 3
    bad = []
    for j in slots:
        x, m = other_x.clone(), None if other_m is None else other_m.clone()
        x[j] = ctx.x[j]
        if m is not None:
            m[j] = ctx.mask[j]
        assert not torch.equal(x[(j + 1) % case.B], ctx.x[(j + 1) % case.B])
        got = _flat(ctx, *ctx.call(x, m))
        bad += [f"slot {j}: {d}" for d in _differences(base, got, slot=j)]
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------- (d)
@cases(P.SENTINEL_CASES)
@pytest.mark.parametrize("fill", [30000.0, -30000.0], ids=["plus", "minus"])
def test_nothing_depends_on_what_the_buffers_held(ctx, fill):
    base = _flat(ctx, *ctx.call())                                                # the reference run: it leaves the case's own padding state behind
    plan = ctx.plan()
    # Exempt: buffers no kernel writes - inputs of the launches that ForwardPlan._set_padding_state prepares with torch copies. Of the plan's floating-point
    # buffers that is `vr` alone, the valid ratios (engine.py, _build_transformer: `self.vr = self._own(torch.ones(B, L, 2, ...))`; filled by
    # _set_padding_state: `self.vr.fill_(1.0)` / `self.vr.copy_(vr)`). The other prepared inputs are not floating-point buffers of plan.buffers: the
    # row flags `rowvalid` / `notpad` are uint8 (`self.rowvalid.copy_(...)`, `self.notpad.copy_(...)` / `.fill_(1)` there), the proposals `props`
    # (`self.props.copy_(...)`) and the position table (PackedWeights.custom "pos.HxW") are not in plan.buffers. A run must leave all of them as they are.
    exempt = {"vr": plan.vr, "rowvalid": plan.rowvalid, "notpad": plan.notpad, "props": plan.props,
              "pos": plan.pw._cache[("c", f"pos.{plan.Hp}x{plan.Wp}")]}
    n = 0
    for t in plan.buffers:
        if t.is_floating_point() and t.data_ptr() != plan.vr.data_ptr():
            t.fill_(fill)
            n += 1
    assert n > 40, n
    plan._pad_state = None                                                        # the padding state is written again (as on a new plan)
    kept = {k: v.clone() for k, v in exempt.items()}
    got = _flat(ctx, *ctx.call())
    for k, v in exempt.items():
        assert torch.equal(_bits(v), _bits(kept[k])), f"the run changed the prepared input {k}"
    bad = _differences(base, got)
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------- (e)
@cases(P.PADSTATE_CASES)
def test_padding_state_of_a_cached_plan(ctx):
    case = ctx.case
    mask_a = ctx.mask
    mask_b = P.tile(P.case_images(case, swap=True)[1], case.B).to(DEV)
    assert not torch.equal(mask_a, mask_b)
    model = ctx.new_model()
    runs = [ctx.call(mask=mask_a, model=model), ctx.call(mask=None, model=model), ctx.call(mask=mask_b, model=model), ctx.call(mask=mask_a, model=model)]
    col5 = {}
    out5 = model([img for img in ctx.x], _collect=col5)                           # a list of equal-sized tensors: no mask
    torch.cuda.synchronize()
    col5.pop("launch_chains")
    plan = ctx.plan(model)                                                       # one (B, H, W): one cached plan served all five
    assert plan._pad_state == "nopad"
    r = [_flat(ctx, *o) for o in runs] + [_flat(ctx, out5, col5)]
    assert not _differences(r[0], r[3]), _differences(r[0], r[3])
    assert not _differences(r[1], r[4]), _differences(r[1], r[4])
    assert _differences(r[0], r[2]) and _differences(r[0], r[1])                  # the masks do matter
    fresh = ctx.new_model()
    dense = _flat(ctx, *ctx.call(mask=None, model=fresh))
    assert not _differences(dense, r[1]), _differences(dense, r[1])
    allfalse = _flat(ctx, *ctx.call(mask=torch.zeros_like(mask_a), model=fresh))
    assert not _differences(dense, allfalse), _differences(dense, allfalse)
    # and the case's own model (its plan has seen forced and free padded runs) gives run 1 again
    again = _flat(ctx, *ctx.free_run())
    assert not _differences(again, r[0]), _differences(again, r[0])


# ----------------------------------------------------------------------------------------------------- (f)
@cases(P.ARENA_CASES)
def test_arena_allocation_gives_the_same_bits(ctx, monkeypatch):
    base = _flat(ctx, *ctx.free_run())
    assert ctx.plan()._arena is None
    monkeypatch.setenv("LWDETR_ARENA", "1")
    ctx.model.invalidate_cache()
    try:
        got = _flat(ctx, *ctx.call())
        assert ctx.plan()._arena is not None
    finally:
        monkeypatch.delenv("LWDETR_ARENA")
        ctx.model.invalidate_cache()
    bad = _differences(base, got)
    assert not bad, bad
