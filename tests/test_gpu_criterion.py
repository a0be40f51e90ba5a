"""GPU: the native evaluation criterion (csrc/match.hip through lwdetr_amd.models.criterion) against the reference's results in
tests/golden/criterion_*.npz and the fp64 restatement tests/criterion_ref.py: cost matrices element by element, assignments, every
loss key, determinism, graph capture (no host synchronisation), the engine.evaluate calling sequence, and a NaN in one image."""
import os

import numpy as np
import pytest
import torch

import lwdetr_amd
import lwdetr_amd.models
import criterion_ref as R
from helpers import GOLDEN, case_batch, golden_state_dict, load_golden
from lwdetr_amd.models import criterion as NC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSSES = ["labels", "boxes", "cardinality"]


@pytest.fixture(scope="module")
def problems():
    return np.load(os.path.join(GOLDEN, "criterion_problems.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def batch():
    return np.load(os.path.join(GOLDEN, "criterion_batch.npz"), allow_pickle=False)


def loss_tol(ref32, ref64):
    """tests/test_criterion_host.py's bound: 4 x the reference's own f32-vs-f64 distance, floor 1e-5 relative."""
    return np.maximum(4.0 * np.abs(ref32 - ref64), 1e-5 * np.abs(ref32))


def dev_layers(layers):
    return [(a.to(DEV), b.to(DEV)) for a, b in layers]


def dev_targets(targets):
    return [{k: v.to(DEV) for k, v in t.items()} for t in targets]


def new_matcher():
    return lwdetr_amd.models.HungarianMatcher(focal_alpha=R.FOCAL_ALPHA, **R.COST_W)


def new_criterion(ia_bce, num_classes=91):
    return lwdetr_amd.models.SetCriterion(num_classes, new_matcher(), {}, R.FOCAL_ALPHA, LOSSES, group_detr=13, ia_bce_loss=ia_bce)


def problem_inputs(g, nq, t, c, dn):
    seed = int(g[R.problem_name(nq, t, c) + ".seed"])
    return R.to_dtype(R.synth_outputs(1, 1, nq, c, seed), dn), R.synth_targets((t,), c, seed)


def batch_inputs(g, name, dn):
    spec = R.BATCH if name == "batch" else R.BATCH_EMPTY
    seed = int(g[name + ".seed"])
    return (R.to_dtype(R.synth_outputs(spec["layers"], len(spec["counts"]), spec["nq"], spec["C"], seed), dn),
            R.synth_targets(spec["counts"], spec["C"], seed), spec)


@pytest.mark.parametrize("dn", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("nq,t,c", R.PROBLEMS)
def test_cost_kernel_every_element_vs_fp64(problems, nq, t, c, dn):
    """lwdetr_match_cost on every fixture problem and input dtype, EVERY element against the fp64 cost of the same rounded inputs; the bound is
    2 x the reference's own f32-vs-fp64 distance on these inputs (stored in the fixture) + 1e-6. Measured maxima: profiles/r8a_criterion.txt."""
    layers, targets = problem_inputs(problems, nq, t, c, dn)
    m = new_matcher()
    arr, keep = NC._layer_array(dev_layers(layers), False)
    packed = NC._Packed(dev_targets(targets), torch.device(DEV), nq, m._offsets)
    ws = m._match(arr, 1, keep[0], packed)
    got = ws.cost[:t * nq].view(t, nq).t().double().cpu().numpy()            # target-major on the device -> (nq, T)
    ref = R.cost_matrix(layers[0][0][0], layers[0][1][0], targets[0]["labels"], targets[0]["boxes"], **R.COST_W).numpy()
    err = np.abs(got - ref).max()
    bound = 2.0 * float(problems[f"{R.problem_name(nq, t, c)}.{dn}.cost_dist"]) + 1e-6
    print(f"cost {R.problem_name(nq, t, c)} {dn}: max |hip - fp64| = {err:.3e}, bound {bound:.3e}, cost range [{ref.min():.2f}, {ref.max():.2f}]")
    assert np.isfinite(got).all() and err <= bound, (err, bound)


@pytest.mark.parametrize("dn", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("nq,t,c", R.PROBLEMS)
def test_matcher_pairs_equal_the_reference(problems, nq, t, c, dn):
    """HungarianMatcher end to end: for f32 inputs the reference's pairs; for f16 / bf16 inputs the pairs of the fp64 restatement on the same
    rounded inputs (the fixture stores them: the generator asserted their stability, tests/test_criterion_host.py that criterion_ref
    reproduces them). Ascending query index, status zero, device tensors, two calls bit-identical."""
    p = R.problem_name(nq, t, c)
    layers, targets = problem_inputs(problems, nq, t, c, dn)
    m = new_matcher()
    out = R.as_outputs(dev_layers(layers))
    (i, j), = m(out, dev_targets(targets))
    assert i.is_cuda and j.is_cuda and i.dtype == torch.int64 and j.dtype == torch.int64 and len(i) == len(j) == min(nq, t)
    assert np.array_equal(i.cpu().numpy(), problems[f"{p}.{dn}.idx_q"]) and np.array_equal(j.cpu().numpy(), problems[f"{p}.{dn}.idx_t"])
    assert (np.diff(i.cpu().numpy()) > 0).all()
    assert m.status().tolist() == [[0]]
    steps = int(m.steps()[0, 0])
    assert t <= steps <= t * (t + 1) // 2
    (i2, j2), = m(out, dev_targets(targets))
    assert torch.equal(i, i2) and torch.equal(j, j2)


def test_matcher_with_an_empty_image_between_two(batch):
    """Images reordered to target counts (7, 0, 40): the empty one sits between two with targets; per-image pairs are the fixture's."""
    layers, targets, spec = batch_inputs(batch, "batch", "f32")
    order = [1, 0, 2]
    lg, bx = layers[0][0][order].to(DEV), layers[0][1][order].to(DEV)
    m = new_matcher()
    res = m({"pred_logits": lg, "pred_boxes": bx}, dev_targets([targets[k] for k in order]))
    fq, ft = batch["batch.f32.idx_q"][:47], batch["batch.f32.idx_t"][:47]    # layer 0: image 0 (none), image 1 (7), image 2 (40)
    assert [len(i) for i, _ in res] == [7, 0, 40]
    assert np.array_equal(res[0][0].cpu().numpy(), fq[:7]) and np.array_equal(res[0][1].cpu().numpy(), ft[:7])
    assert np.array_equal(res[2][0].cpu().numpy(), fq[7:]) and np.array_equal(res[2][1].cpu().numpy(), ft[7:])
    assert m.status().tolist() == [[0, 0, 0]] and m.steps()[0, 1].item() == 0


@pytest.mark.parametrize("name,dn,form", [(n, d, f) for n in ("batch", "empty") for d in ("f32", "f16") for f in ("focal", "iabce")])
def test_criterion_every_key_vs_the_reference(batch, name, dn, form):
    """SetCriterion on the three-image batch (target counts 0, 7, 40; final + two aux + enc) and on the all-empty batch, both loss forms,
    f32 and f16 outputs: key order, every value within the host test's bound of the reference, class_error and cardinality_error exact,
    the assignment of every layer, and bit-identical values from a second call (deterministic reductions)."""
    layers, targets, spec = batch_inputs(batch, name, dn)
    crit = new_criterion(form == "iabce")
    out, tg = R.as_outputs(dev_layers(layers)), dev_targets(targets)
    got = crit(out, tg)
    keys = [str(k) for k in batch["keys"]]
    assert list(got) == keys
    assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in got.values())
    vals = np.array([got[k].item() for k in keys], dtype=np.float64)
    ref32, ref64 = batch[f"{name}.{dn}.{form}.ref32"], batch[f"{name}.{dn}.{form}.ref64"]
    err, tol = np.abs(vals - ref32), loss_tol(ref32, ref64)
    for k, v, r, e, t in zip(keys, vals, ref32, err, tol):
        print(f"{name} {dn} {form} {k}: hip {v:.8g} reference {r:.8g} |diff| {e:.2e} bound {t:.2e}")
    assert (err <= tol).all()
    for n, k in enumerate(keys):
        if k.startswith(("class_error", "cardinality_error")):
            assert vals[n] == ref32[n], k
    iq = torch.cat([i for lay in crit.last_indices for i, _ in lay]).cpu().numpy()
    it = torch.cat([j for lay in crit.last_indices for _, j in lay]).cpu().numpy()
    assert np.array_equal(iq, batch[f"{name}.{dn}.idx_q"]) and np.array_equal(it, batch[f"{name}.{dn}.idx_t"])
    assert not crit.matcher.status().any()
    again = crit(out, tg)
    assert all(torch.equal(got[k], again[k]) for k in keys)


@pytest.mark.parametrize("form", ["focal", "iabce"])
@pytest.mark.parametrize("nq,t,c", R.PROBLEMS)
def test_criterion_on_the_single_problems(problems, nq, t, c, form):
    """One image, one layer, every fixture shape (nq not a multiple of the 32-query chunk, T = nq, 366 classes): the reference's five values."""
    p = R.problem_name(nq, t, c)
    layers, targets = problem_inputs(problems, nq, t, c, "f32")
    got = new_criterion(form == "iabce", c)(R.as_outputs(dev_layers(layers)), dev_targets(targets))
    keys = R.loss_keys(0, enc=False)
    assert list(got) == keys
    vals = np.array([got[k].item() for k in keys], dtype=np.float64)
    ref32, ref64 = problems[f"{p}.{form}.ref32"], problems[f"{p}.{form}.ref64"]
    assert (np.abs(vals - ref32) <= loss_tol(ref32, ref64)).all(), (vals, ref32)
    assert vals[1] == ref32[1] and vals[4] == ref32[4]


def test_criterion_call_is_capturable_and_replays_bit_for_bit(batch):
    """No host synchronisation inside a call: at world size 1 the whole call (packing the targets included) is captured with
    torch.cuda.graph on one stream; replays on new outputs written into the captured tensors reproduce the eager values bit for bit."""
    layers, targets, spec = batch_inputs(batch, "batch", "f16")
    crit = new_criterion(False)
    tg = dev_targets(targets)
    static = dev_layers(layers)
    out = R.as_outputs(static)
    eager_a = {k: v.clone() for k, v in crit(out, tg).items()}
    other = dev_layers(R.to_dtype(R.synth_outputs(spec["layers"], 3, spec["nq"], spec["C"], 977), "f16"))
    eager_b = {k: v.clone() for k, v in crit(R.as_outputs(other), tg).items()}
    assert any(not torch.equal(eager_a[k], eager_b[k]) for k in eager_a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        crit(out, tg)                                            # warm-up on the capture stream: workspaces and offsets exist before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        captured = crit(out, tg)
    for (sa, sb), (oa, ob) in zip(static, other):
        sa.copy_(oa)
        sb.copy_(ob)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(captured[k], eager_b[k]) for k in eager_b)
    for (sa, sb), (oa, ob) in zip(static, dev_layers(layers)):
        sa.copy_(oa)
        sb.copy_(ob)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(captured[k], eager_a[k]) for k in eager_a)


def test_evaluate_loop_with_the_native_criterion():
    """The calling sequence of the reference's engine.evaluate (engine.py:93-164) as tests/test_gpu_model.py::test_evaluate_loop_contract
    walks it, with build_model's native criterion in place of the stub: tiny model, one 192x256 golden case, synthetic targets. The loop's
    loss_dict_reduced_scaled arithmetic runs, every value is finite and equals the fp64 restatement on the model's own outputs within
    the criterion bound's floor, 1e-5 relative (the reference cannot run beside the GPU, so its own f32-vs-f64 distance, the other
    term of the bound, is not available here: the tighter half is asserted). The synthetic targets were checked for a stable assignment
    on the golden outputs of this case (1e-4 perturbations of every cost entry), as the fixture generator checks its problems."""
    pytest.importorskip("scipy")
    g = load_golden("tiny_192x256")
    size, images, mask = case_batch("tiny_192x256")
    args = lwdetr_amd.get_args(size)
    args.native_criterion = True
    model, criterion, post = lwdetr_amd.build_model(args)
    assert type(criterion) is lwdetr_amd.models.SetCriterion
    model.load_state_dict(golden_state_dict(g), strict=True)
    model = model.to(DEV).eval()
    criterion.eval()
    synth = R.synth_targets((3, 5), 91, 31)
    loader = [(lwdetr_amd.models.NestedTensor(images, mask),
               [{"image_id": torch.tensor(7), "orig_size": torch.tensor([480, 640]), **synth[0]},
                {"image_id": torch.tensor(9), "orig_size": torch.tensor([480, 640]), **synth[1]}])]
    updates, logged = {}, {}
    for samples, targets in loader:
        samples = samples.to(DEV)
        targets = [{k: v.to(DEV) for k, v in t.items()} for t in targets]
        outputs = model(samples)
        loss_dict = criterion(outputs, targets)
        weight_dict = criterion.weight_dict
        loss_dict_reduced = loss_dict                             # utils.reduce_dict at world size 1
        loss_dict_reduced_scaled = {k: v * weight_dict[k] for k, v in loss_dict_reduced.items() if k in weight_dict}
        loss_dict_reduced_unscaled = {f"{k}_unscaled": v for k, v in loss_dict_reduced.items()}
        logged.update(loss=sum(loss_dict_reduced_scaled.values()).item(), class_error=loss_dict_reduced["class_error"].item(),
                      **{k: v.item() for k, v in loss_dict_reduced_scaled.items()}, **{k: v.item() for k, v in loss_dict_reduced_unscaled.items()})
        orig = torch.stack([t["orig_size"] for t in targets], dim=0)
        results = post["bbox"](outputs, orig)
        updates.update({t["image_id"].item(): o for t, o in zip(targets, results)})
    assert sorted(updates) == [7, 9] and all(np.isfinite(v) for v in logged.values())
    keys = R.loss_keys(args.dec_layers - 1)
    assert list(loss_dict) == keys and set(weight_dict) == {k for k in keys if k.startswith("loss_")}
    host = lambda d: {k: (host(v) if isinstance(v, dict) else [host(a) for a in v] if isinstance(v, list) else v.float().cpu())
                      for k, v in d.items() if k in ("pred_logits", "pred_boxes", "aux_outputs", "enc_outputs")}
    outs = host(outputs)
    ref, _ = R.criterion(outs, synth)
    for k in keys:
        tol = 1e-5 * abs(ref[k])
        print(f"evaluate {k}: hip {loss_dict[k].item():.8g} fp64 {ref[k]:.8g} bound {tol:.2e}")
        assert abs(loss_dict[k].item() - ref[k]) <= tol, k
    assert abs(logged["loss"] - sum(ref[k] * weight_dict[k] for k in weight_dict)) <= 1e-4 * abs(logged["loss"])


def test_nan_in_one_image_is_flagged_and_contained(batch):
    """Image 2's logits hold a NaN row in every layer: the launches return, images 0 and 1 keep their pairs and losses stay per-image
    contained in the assignment, matcher.status() flags exactly image 2 in each layer. (The same input terminates on the host
    instantiation: tests/test_criterion_host.py::test_host_solver_status_is_local_to_the_poisoned_problem; the trip counts are bounded.)"""
    layers, targets, spec = batch_inputs(batch, "batch", "f32")
    poisoned = [(lg.clone(), bx) for lg, bx in layers]
    for lg, _ in poisoned:
        lg[2, 17, :] = float("nan")
    crit = new_criterion(False)
    crit(R.as_outputs(dev_layers(poisoned)), dev_targets(targets))
    torch.cuda.synchronize()
    assert crit.matcher.status().tolist() == [[0, 0, 1]] * spec["layers"]
    fq, ft = batch["batch.f32.idx_q"], batch["batch.f32.idx_t"]
    for l, lay in enumerate(crit.last_indices):
        (i0, _), (i1, j1), (i2, j2) = lay
        assert len(i0) == 0
        assert np.array_equal(i1.cpu().numpy(), fq[47 * l:47 * l + 7]) and np.array_equal(j1.cpu().numpy(), ft[47 * l:47 * l + 7])
        q2, t2 = i2.cpu().numpy(), j2.cpu().numpy()
        assert len(q2) == 40 and (np.diff(q2) > 0).all() and q2.min() >= 0 and q2.max() < spec["nq"] and sorted(t2.tolist()) == list(range(40))
