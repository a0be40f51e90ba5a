"""CPU: the evaluation criterion without a GPU - the fp64 restatement (tests/criterion_ref.py) against the reference's results in
tests/golden/criterion_*.npz, the assignment solver's host instantiation (lwdetr_match_assign_host) against the same fixtures and on
non-finite costs, the C ABI of the new entries, and the Python interface's refusals."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import lwdetr_amd
import lwdetr_amd.models
import criterion_ref as R
from helpers import GOLDEN, ROOT, sample_idx


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from lwdetr_amd import _native
    return _native


@pytest.fixture(scope="module")
def problems():
    return np.load(os.path.join(GOLDEN, "criterion_problems.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def batch():
    return np.load(os.path.join(GOLDEN, "criterion_batch.npz"), allow_pickle=False)


def problem_inputs(g, nq, t, c):
    seed = int(g[R.problem_name(nq, t, c) + ".seed"])
    return R.synth_outputs(1, 1, nq, c, seed), R.synth_targets((t,), c, seed)


def loss_tol(ref32, ref64):
    """The issue's bound per key: 4 x the reference's own f32-vs-f64 distance, floor 1e-5 relative (f32 terms carry a few ulp each,
    and every implementation under test accumulates in f64)."""
    return np.maximum(4.0 * np.abs(ref32 - ref64), 1e-5 * np.abs(ref32))


def assign_host(native, cost_qt):
    """lwdetr_match_assign_host on a (nq, T) cost (as the reference lays it out): (idx_q, idx_t, status, steps)."""
    cost_qt = np.asarray(cost_qt, dtype=np.float32)
    nq, t = cost_qt.shape
    tm = np.ascontiguousarray(cost_qt.T)                         # the solver's layout: target-major
    iq, it = np.full(max(t, 1), -7, np.int64), np.full(max(t, 1), -7, np.int64)
    status, steps = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = native.lib().lwdetr_match_assign_host(tm.ctypes.data, nq, t, iq.ctypes.data, it.ctypes.data, ctypes.byref(status), ctypes.byref(steps))
    assert rc == 0, rc
    return iq[:t], it[:t], status.value, steps.value


# ---------------------------------------------------------------------------------------------------- the fp64 restatement
@pytest.mark.parametrize("nq,t,c", R.PROBLEMS)
def test_restatement_reproduces_the_reference_cost_and_assignment(problems, nq, t, c):
    pytest.importorskip("scipy")
    p = R.problem_name(nq, t, c)
    layers, targets = problem_inputs(problems, nq, t, c)
    for dn in ("f32", "f16", "bf16"):
        (lg, bx), = R.to_dtype(layers, dn)
        cost = R.cost_matrix(lg[0], bx[0], targets[0]["labels"], targets[0]["boxes"], **R.COST_W).numpy()
        i, j = R.solve(cost)
        assert np.array_equal(i, problems[f"{p}.{dn}.idx_q"]) and np.array_equal(j, problems[f"{p}.{dn}.idx_t"]), dn
        assert len(i) == min(nq, t) and (np.diff(i) > 0).all()
        if dn == "f32":
            si = sample_idx(cost.size)
            assert np.array_equal(cost.reshape(-1)[si], problems[p + ".cost_sample64"])           # same inputs, same fp64 formula
            d = np.abs(problems[p + ".cost_sample32"].astype(np.float64) - cost.reshape(-1)[si]).max()
            assert d <= float(problems[f"{p}.f32.cost_dist"]) and d < 1e-4
    if (nq, t, c) == (8, 5, 7):                                 # and without scipy: every injective map of 5 targets into 8 queries
        bi, bj = R.solve_brute(R.cost_matrix(layers[0][0][0], layers[0][1][0], targets[0]["labels"], targets[0]["boxes"], **R.COST_W).numpy())
        assert np.array_equal(bi, problems[p + ".f32.idx_q"]) and np.array_equal(bj, problems[p + ".f32.idx_t"])


@pytest.mark.parametrize("form", ["focal", "iabce"])
@pytest.mark.parametrize("nq,t,c", R.PROBLEMS)
def test_restatement_reproduces_the_reference_losses(problems, nq, t, c, form):
    pytest.importorskip("scipy")
    p = R.problem_name(nq, t, c)
    layers, targets = problem_inputs(problems, nq, t, c)
    got, _ = R.criterion(R.as_outputs(layers), targets, ia_bce=form == "iabce")
    keys = R.loss_keys(0, enc=False)
    assert list(got) == keys
    ref32, ref64 = problems[f"{p}.{form}.ref32"], problems[f"{p}.{form}.ref64"]
    err = np.abs(np.array([got[k] for k in keys]) - ref32)
    assert (err <= loss_tol(ref32, ref64)).all(), dict(zip(keys, zip(err, loss_tol(ref32, ref64))))


@pytest.mark.parametrize("name,dn,form", [(n, d, f) for n in ("batch", "empty") for d in ("f32", "f16") for f in ("focal", "iabce")])
def test_restatement_reproduces_the_reference_on_the_batches(batch, name, dn, form):
    pytest.importorskip("scipy")
    spec = R.BATCH if name == "batch" else R.BATCH_EMPTY
    seed = int(batch[name + ".seed"])
    layers = R.to_dtype(R.synth_outputs(spec["layers"], len(spec["counts"]), spec["nq"], spec["C"], seed), dn)
    targets = R.synth_targets(spec["counts"], spec["C"], seed)
    got, idx = R.criterion(R.as_outputs(layers), targets, ia_bce=form == "iabce")
    keys = [str(k) for k in batch["keys"]]
    assert list(got) == keys == R.loss_keys(2)
    assert np.array_equal(np.concatenate([i for lay in idx for i, _ in lay]), batch[f"{name}.{dn}.idx_q"])
    assert np.array_equal(np.concatenate([j for lay in idx for _, j in lay]), batch[f"{name}.{dn}.idx_t"])
    ref32, ref64 = batch[f"{name}.{dn}.{form}.ref32"], batch[f"{name}.{dn}.{form}.ref64"]
    err = np.abs(np.array([got[k] for k in keys]) - ref32)
    assert (err <= loss_tol(ref32, ref64)).all(), dict(zip(keys, zip(err, loss_tol(ref32, ref64))))


# ---------------------------------------------------------------------------------------------------- the solver on the host
@pytest.mark.parametrize("nq,t,c", R.PROBLEMS)
def test_host_solver_reproduces_the_fixture_pairs(built, problems, nq, t, c):
    """T = 1, T = nq (65), nq = 37 / 65 / 300: the reference's pairs, ascending in the query index, from the f32 cost of the restatement
    (the fixtures only hold problems whose assignment survives 1e-4 perturbations of every entry)."""
    p = R.problem_name(nq, t, c)
    layers, targets = problem_inputs(problems, nq, t, c)
    cost = R.cost_matrix(layers[0][0][0], layers[0][1][0], targets[0]["labels"], targets[0]["boxes"], **R.COST_W).numpy().astype(np.float32)
    iq, it, status, steps = assign_host(built, cost)
    assert status == 0 and t <= steps <= t * (t + 1) // 2
    assert np.array_equal(iq, problems[p + ".f32.idx_q"]) and np.array_equal(it, problems[p + ".f32.idx_t"])


def test_host_solver_equals_scipy_on_random_rectangles(built):
    """Every lane count the dispatcher has (nq up to 64 / 128 / 320 / 512 / 1024) and ties: integer costs have many optima, so the TOTAL is compared."""
    sp = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(5)
    for nq, t in [(1, 1), (3, 3), (64, 17), (100, 100), (128, 5), (321, 64), (512, 33), (1024, 40)]:
        cost = rng.normal(size=(nq, t)).astype(np.float32)
        iq, it, status, _ = assign_host(built, cost)
        ri, rj = sp.linear_sum_assignment(cost.astype(np.float64))
        assert status == 0 and np.array_equal(iq, ri) and np.array_equal(it, rj), (nq, t)
    cost = rng.integers(0, 4, size=(40, 12)).astype(np.float32)
    iq, it, status, _ = assign_host(built, cost)
    ri, rj = sp.linear_sum_assignment(cost.astype(np.float64))
    assert status == 0 and len(set(iq)) == 12 and sorted(it) == list(range(12)) and cost[iq, it].sum() == cost[ri, rj].sum()


def test_host_solver_with_no_target_writes_nothing(built):
    iq, it, status, steps = assign_host(built, np.zeros((37, 0), np.float32))
    assert len(iq) == 0 and status == 0 and steps == 0


def test_host_solver_refuses_more_targets_than_queries(built):
    c = np.zeros((5, 3), np.float32)
    buf = np.zeros(5, np.int64)
    rc = built.lib().lwdetr_match_assign_host(c.ctypes.data, 3, 5, buf.ctypes.data, buf.ctypes.data, None, None)
    assert rc == built.ERR_UNSUPPORTED
    rc = built.lib().lwdetr_match_assign_host(c.ctypes.data, 2000, 1, buf.ctypes.data, buf.ctypes.data, None, None)
    assert rc == built.ERR_UNSUPPORTED


@pytest.mark.parametrize("kind", ["nan_row", "inf_entries", "all_nan", "neg_inf"])
@pytest.mark.parametrize("nq,t", [(8, 5), (65, 65), (300, 40)])
def test_host_solver_terminates_on_non_finite_costs(built, kind, nq, t):
    """The loops' trip counts are fixed by T and nq: a NaN row, +inf entries, an all-NaN matrix and -inf entries all return, set the status
    word, and still leave min(nq, T) distinct in-range pairs in ascending query order."""
    rng = np.random.default_rng(nq + t)
    cost = rng.normal(size=(nq, t)).astype(np.float32)
    if kind == "nan_row":
        cost[:, t // 2] = np.nan                                 # one target's whole solver row
    elif kind == "inf_entries":
        cost[rng.random(cost.shape) < 0.3] = np.inf
        cost[:, 0] = np.inf
    elif kind == "all_nan":
        cost[:] = np.nan
    else:
        cost[rng.random(cost.shape) < 0.2] = -np.inf
    iq, it, status, steps = assign_host(built, cost)
    assert status == 1 and steps <= t * (t + 1) // 2
    assert len(iq) == min(nq, t) and (np.diff(iq) > 0).all() and iq.min() >= 0 and iq.max() < nq
    assert sorted(it.tolist()) == list(range(t))


def test_host_solver_status_is_local_to_the_poisoned_problem(built, problems):
    """The same fixture problem beside a poisoned copy: the clean one is unchanged (one problem per call on the host; the GPU test runs both in one launch)."""
    nq, t, c = 300, 40, 91
    layers, targets = problem_inputs(problems, nq, t, c)
    lg = layers[0][0].clone()
    lg[0, 17, :] = float("nan")
    cost = R.cost_matrix(lg[0], layers[0][1][0], targets[0]["labels"], targets[0]["boxes"], **R.COST_W).numpy().astype(np.float32)
    assert np.isnan(cost[17]).all() and np.isfinite(np.delete(cost, 17, 0)).all()
    iq, it, status, _ = assign_host(built, cost)
    assert status == 1 and len(set(iq.tolist())) == t and sorted(it.tolist()) == list(range(t))


# ---------------------------------------------------------------------------------------------------- C ABI
def test_new_entries_are_declared(built):
    hdr = open(os.path.join(ROOT, "include", "lwdetr_hip.h")).read()
    lib = ctypes.CDLL(built.LIB_PATH)
    for sym in ("lwdetr_match_cost", "lwdetr_match_assign", "lwdetr_match_assign_host", "lwdetr_criterion_partials",
                "lwdetr_criterion_partials_floats", "lwdetr_criterion_finish"):
        assert sym + "(" in hdr and hasattr(lib, sym), sym
    assert built.lib().lwdetr_criterion_partials_floats(4, 32, 300) == 4 * 32 * 10 * 5


def test_criterion_ctypes_struct_matches_header_layout(built):
    """sizeof() / offsets of the ctypes mirror equal what a C compiler computes for lwdetr_crit_layer, and the limits agree."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lwdetr_hip.h"\nint main(){printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(lwdetr_crit_layer),'
           ' offsetof(lwdetr_crit_layer, boxes), offsetof(lwdetr_crit_layer, class_error), offsetof(lwdetr_crit_layer, reserved),'
           ' LWDETR_CRIT_MAX_LAYERS, LWDETR_MATCH_MAX_NQ, LWDETR_CRIT_QCHUNK);return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(td, "s")]).split()]
    cl = built.CritLayer
    assert got == [ctypes.sizeof(cl), cl.boxes.offset, cl.class_error.offset, cl.reserved.offset, built.CRIT_MAX_LAYERS,
                   built.MATCH_MAX_NQ, built.CRIT_QCHUNK]


# ---------------------------------------------------------------------------------------------------- Python interface
def test_build_model_returns_the_native_criterion_without_the_reference():
    """In a process where the reference is not importable build_model's second element is lwdetr_amd.models.SetCriterion
    (it was None before the native criterion existed)."""
    code = ("import sys, importlib.util\n"
            "assert importlib.util.find_spec('models') is None, 'the reference must not be importable here'\n"
            "import lwdetr_amd\n"
            "m, crit, post = lwdetr_amd.build_model(lwdetr_amd.get_args('tiny'))\n"
            "assert type(crit) is lwdetr_amd.models.SetCriterion and crit is not None, crit\n"
            "assert lwdetr_amd.SetCriterion is lwdetr_amd.models.SetCriterion and lwdetr_amd.HungarianMatcher is lwdetr_amd.models.HungarianMatcher\n"
            "assert isinstance(crit.matcher, lwdetr_amd.models.HungarianMatcher) and not crit.training\n"
            "assert crit.losses == ['labels', 'boxes', 'cardinality'] and crit.ia_bce_loss is False\n"
            "a = lwdetr_amd.get_args('tiny'); a.use_varifocal_loss = True\n"
            "assert lwdetr_amd.build_model(a)[1] is None\n"
            "a = lwdetr_amd.get_args('tiny'); a.ia_bce_loss = True; a.native_criterion = True\n"
            "assert lwdetr_amd.build_model(a)[1].ia_bce_loss is True\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_weight_dict_key_order_equals_the_reference(batch):
    args = lwdetr_amd.get_args("tiny")
    crit = lwdetr_amd.models.build_criterion(args)
    keys = [str(k) for k in batch["keys"]]                      # the reference's loss dict: 3 decoder layers + enc, as the tiny config has
    assert list(crit.weight_dict) == [k for k in keys if k.startswith("loss_")]
    assert crit.weight_dict["loss_ce"] == args.cls_loss_coef and crit.weight_dict["loss_bbox_enc"] == args.bbox_loss_coef
    assert crit.weight_dict["loss_giou_1"] == args.giou_loss_coef
    m = lwdetr_amd.models.build_matcher(args)
    assert (m.cost_class, m.cost_bbox, m.cost_giou, m.focal_alpha) == (args.set_cost_class, args.set_cost_bbox, args.set_cost_giou, args.focal_alpha)


def test_refusals():
    from lwdetr_amd._native import NativeError
    M = lwdetr_amd.models
    matcher = M.HungarianMatcher(2.0, 5.0, 2.0, 0.25)
    wd = {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou": 2.0}
    for flag in ("use_varifocal_loss", "use_position_supervised_loss"):
        with pytest.raises(NotImplementedError):
            M.SetCriterion(91, matcher, wd, 0.25, ["labels", "boxes", "cardinality"], **{flag: True})
    crit = M.SetCriterion(91, matcher, wd, 0.25, ["labels", "boxes", "cardinality"], group_detr=13)
    assert crit.eval() is crit and not crit.training and crit.weight_dict is wd
    with pytest.raises(NotImplementedError):
        crit.train()
    with pytest.raises(NotImplementedError):
        crit.train(True)
    out = {"pred_logits": torch.zeros(1, 8, 7), "pred_boxes": torch.full((1, 8, 4), 0.5)}
    tg = [{"labels": torch.zeros(5, dtype=torch.int64), "boxes": torch.full((5, 4), 0.5)}]
    with pytest.raises(NotImplementedError):
        matcher(out, tg, group_detr=13)
    with pytest.raises(NativeError, match="ROCm device"):        # CPU inputs: there is no CPU path
        matcher(out, tg)
    with pytest.raises(NativeError, match="ROCm device"):
        crit(out, tg)
    many = [{"labels": torch.zeros(9, dtype=torch.int64), "boxes": torch.full((9, 4), 0.5)}]
    with pytest.raises(NativeError, match="9 targets but the model has 8 queries"):      # T_b > nq, refused before anything is launched
        matcher(out, many)
    with pytest.raises(NativeError, match="9 targets but the model has 8 queries"):
        crit(out, many)


def test_assign_entry_refuses_more_targets_than_queries(built):
    """lwdetr_match_assign checks the host counts before it launches: LWDETR_ERR_UNSUPPORTED for T_b > nq, no GPU needed to be told so."""
    counts = (ctypes.c_int32 * 2)(3, 9)
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    assert built.lib().lwdetr_match_assign(p, p, counts, 1, 2, 8, p, p, p, None, None) == built.ERR_UNSUPPORTED
    assert built.lib().lwdetr_match_assign(p, p, counts, 1, 2, 2048, p, p, p, None, None) == built.ERR_UNSUPPORTED
