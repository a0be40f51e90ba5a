"""GPU: the native training criterion (csrc/match_train.hip through lwdetr_amd.models.criterion_train) against the reference's train() mode
results in tests/golden/criterion_train.npz and the fp64 restatement tests/criterion_train_ref.py: the pairs of every (layer, image, group),
every loss key of the four forms, every element of every gradient, determinism, graph capture of forward + backward (no host
synchronisation), and a NaN in one image.

Shapes (criterion_train_ref.BATCHES): g3 = 3 groups of 37 queries (group edges cross the 32-query chunks and the 64-lane columns), target
counts 7 / 0 / 1 / 37 (an empty image between two others, T_b equal to the group width), 7 classes, four layers; g13 = the reference's
13 x 300 queries (above 1024 in total, not per group), 1 / 0 / 40 targets, 91 classes; c366 = 366 classes; empty = no target anywhere."""
import os

import numpy as np
import pytest
import torch

import lwdetr_amd
import lwdetr_amd.models
import criterion_ref as R
import criterion_train_ref as TR
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSSES = ["labels", "boxes", "cardinality"]
ROUND = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}      # one rounding of a gradient to the inputs' dtype, relative
# ... and absolute where the format has run out of exponent: most logit gradients (sigmoid tails over num_boxes) lie below f16's smallest
# normal number 2^-14, where the spacing is 2^-24 whatever the value, so one rounding is half of that. bf16 has f32's exponent range.
ROUND_ABS = {"f32": 0.0, "f16": 2.0 ** -25, "bf16": 0.0}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "criterion_train.npz"), allow_pickle=False)


def loss_tol(ref32, ref64):
    """tests/test_criterion_host.py's bound: 4 x the reference's own f32-vs-f64 distance, floor 1e-5 relative."""
    return np.maximum(4.0 * np.abs(ref32 - ref64), 1e-5 * np.abs(ref32))


def dev_layers(layers, grad=False):
    return [(a.to(DEV).requires_grad_(grad), b.to(DEV).requires_grad_(grad)) for a, b in layers]


def dev_targets(targets):
    return [{k: v.to(DEV) for k, v in t.items()} for t in targets]


def new_matcher():
    return lwdetr_amd.models.GroupHungarianMatcher(focal_alpha=R.FOCAL_ALPHA, **R.COST_W)


def new_criterion(form, groups, num_classes, **kw):
    return lwdetr_amd.models.TrainSetCriterion(num_classes, new_matcher(), {}, R.FOCAL_ALPHA, LOSSES, group_detr=groups,
                                               **TR.FORM_FLAGS[form], **kw)


def inputs(fx, name, dn):
    return TR.batch_inputs(name, int(fx[name + ".seed"]), dn)


def fixture_indices(fx, name, dn):
    s = TR.BATCHES[name]
    iq, it = fx[f"{name}.{dn}.idx_q"], fx[f"{name}.{dn}.idx_t"]
    out, pos = [], 0
    for _ in range(s["layers"]):
        lay = []
        for t in s["counts"]:
            n = t * s["G"]
            lay.append((iq[pos:pos + n], it[pos:pos + n]))
            pos += n
        out.append(lay)
    assert pos == len(iq)
    return out


def flat(indices, k):
    return torch.cat([pair[k] for lay in indices for pair in lay]).cpu().numpy()


def box_rows(gbox, idx):
    rows = [gbox[b][torch.as_tensor(i)] for b, (i, _) in enumerate(idx) if len(i)]
    return torch.cat(rows) if rows else torch.zeros(0, 4, dtype=gbox.dtype)


# ---------------------------------------------------------------------------------------------------- 1. pairs
@pytest.mark.parametrize("dn", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["g3", "g13", "c366"])
def test_group_matcher_pairs_equal_the_reference(fx, name, dn):
    """GroupHungarianMatcher layer by layer: the fixture's pairs of every (layer, image, group) (for f16 / bf16 the pairs on the rounded
    inputs), query indices offset by g * gw and ascending inside each group, status zero, steps within their fixed bound, two calls bit-identical."""
    s = TR.BATCHES[name]
    layers, targets = inputs(fx, name, dn)
    want = fixture_indices(fx, name, dn)
    m, tg, gw = new_matcher(), dev_targets(targets), s["nq"] // s["G"]
    for l, (lg, bx) in enumerate(dev_layers(layers)):
        out = {"pred_logits": lg, "pred_boxes": bx}
        res = m(out, tg, group_detr=s["G"])
        assert len(res) == len(targets)
        for b, ((i, j), (wi, wj)) in enumerate(zip(res, want[l])):
            assert i.is_cuda and j.is_cuda and i.dtype == torch.int64 and j.dtype == torch.int64
            t = s["counts"][b]
            assert len(i) == len(j) == s["G"] * t
            assert np.array_equal(i.cpu().numpy(), wi) and np.array_equal(j.cpu().numpy(), wj), (l, b)
            q = i.cpu().numpy().reshape(s["G"], t)
            assert all(((q[g] >= g * gw) & (q[g] < (g + 1) * gw)).all() and (np.diff(q[g]) > 0).all() for g in range(s["G"]))
        st, steps = m.status(), m.steps()
        assert tuple(st.shape) == tuple(steps.shape) == (1, len(targets), s["G"]) and not st.any()
        for b, t in enumerate(s["counts"]):
            assert ((steps[0, b] >= t) & (steps[0, b] <= t * (t + 1) // 2)).all()
        again = m(out, tg, group_detr=s["G"])
        assert all(torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) for a, c in zip(res, again))


@pytest.mark.parametrize("dn", ["f32", "bf16"])
def test_one_group_equals_the_evaluation_matcher_bit_for_bit(fx, dn):
    layers, targets = inputs(fx, "g3", dn)
    tg = dev_targets(targets)
    old = lwdetr_amd.models.HungarianMatcher(focal_alpha=R.FOCAL_ALPHA, **R.COST_W)
    for lg, bx in dev_layers(layers):
        out = {"pred_logits": lg, "pred_boxes": bx}
        a, c = new_matcher()(out, tg, group_detr=1), old(out, tg)
        assert [len(i) for i, _ in a] == [7, 0, 1, 37]
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, c))


# ---------------------------------------------------------------------------------------------------- 2. every loss key
LOSS_CASES = ([(n, d, f) for n in ("g3", "empty") for d in ("f32", "f16") for f in TR.FORMS] +
              [(n, "f32", f) for n in ("g13", "c366") for f in TR.FORMS])


@pytest.mark.parametrize("name,dn,form", LOSS_CASES)
def test_train_criterion_every_key_vs_the_reference(fx, name, dn, form):
    """TrainSetCriterion in train() mode: the reference's keys in its order, every value within the loss bound of the reference's f32 run,
    class_error and cardinality_error exact, the pairs of every layer, grad_fn on exactly the differentiable keys, a second call bit-identical."""
    s = TR.BATCHES[name]
    layers, targets = inputs(fx, name, dn)
    crit = new_criterion(form, s["G"], s["C"])
    assert crit.training
    out, tg = R.as_outputs(dev_layers(layers, grad=True)), dev_targets(targets)
    got = crit(out, tg)
    keys = [str(k) for k in fx[name + ".keys"]]
    assert list(got) == keys
    assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in got.values())
    for k, v in got.items():
        assert (v.grad_fn is not None) == k.startswith("loss_"), k
    vals = np.array([got[k].item() for k in keys], dtype=np.float64)
    ref32, ref64 = fx[f"{name}.{dn}.{form}.ref32"], fx[f"{name}.{dn}.{form}.ref64"]
    err, tol = np.abs(vals - ref32), loss_tol(ref32, ref64)
    for k, v, r, e, t in zip(keys, vals, ref32, err, tol):
        print(f"{name} {dn} {form} {k}: hip {v:.8g} reference {r:.8g} |diff| {e:.2e} bound {t:.2e}")
    assert (err <= tol).all()
    for n, k in enumerate(keys):
        if k.startswith(("class_error", "cardinality_error")):
            assert vals[n] == ref32[n], k
    assert np.array_equal(flat(crit.last_indices, 0), fx[f"{name}.{dn}.idx_q"]) and np.array_equal(flat(crit.last_indices, 1), fx[f"{name}.{dn}.idx_t"])
    assert not crit.matcher.status().any() and tuple(crit.matcher.status().shape) == (s["layers"], len(targets), s["G"])
    again = crit(out, tg)
    assert all(torch.equal(got[k], again[k]) for k in keys)
    with torch.no_grad():
        plain = crit(out, tg)
    assert all(v.grad_fn is None for v in plain.values()) and all(torch.equal(got[k], plain[k]) for k in keys)


def test_sum_group_losses(fx):
    """num_boxes is not multiplied by group_detr (lwdetr.py:418-419): the reference's values with sum_group_losses=True."""
    s = TR.BATCHES["g3"]
    layers, targets = inputs(fx, "g3", "f32")
    got = new_criterion("focal", s["G"], s["C"], sum_group_losses=True)(R.as_outputs(dev_layers(layers)), dev_targets(targets))
    keys = [str(k) for k in fx["g3.keys"]]
    ref32, ref64 = fx["g3.f32.focal.sgl.ref32"], fx["g3.f32.focal.sgl.ref64"]
    vals = np.array([got[k].item() for k in keys], dtype=np.float64)
    assert list(got) == keys and (np.abs(vals - ref32) <= loss_tol(ref32, ref64)).all(), (vals, ref32)
    assert vals[0] > 2.5 * fx["g3.f32.focal.ref32"][0]


@pytest.mark.parametrize("name,dn", [("g3", "f32"), ("g3", "f16"), ("c366", "f32"), ("empty", "f32")])
@pytest.mark.parametrize("form", ["focal", "iabce"])
def test_eval_mode_equals_the_evaluation_criterion_bit_for_bit(fx, name, dn, form):
    """eval(): one group (lwdetr.py:410) - every value and every pair equal lwdetr_amd.models.SetCriterion's, bit for bit."""
    s = TR.BATCHES[name]
    layers, targets = inputs(fx, name, dn)
    out, tg = R.as_outputs(dev_layers(layers)), dev_targets(targets)
    new = new_criterion(form, s["G"], s["C"]).eval()
    old = lwdetr_amd.models.SetCriterion(s["C"], lwdetr_amd.models.HungarianMatcher(focal_alpha=R.FOCAL_ALPHA, **R.COST_W), {}, R.FOCAL_ALPHA,
                                         LOSSES, group_detr=s["G"], ia_bce_loss=form == "iabce")
    a, c = new(out, tg), old(out, tg)
    assert list(a) == list(c)
    for k in a:
        assert torch.equal(a[k], c[k]), (k, a[k].item(), c[k].item())
    assert np.array_equal(flat(new.last_indices, 0), flat(old.last_indices, 0)) and np.array_equal(flat(new.last_indices, 1), flat(old.last_indices, 1))


# ---------------------------------------------------------------------------------------------------- 3. gradients
GRAD_CASES = ([("g3", d, f) for d in ("f32", "f16", "bf16") for f in TR.FORMS] + [("c366", "f32", f) for f in TR.FORMS] +
              [("g13", "f32", "focal"), ("g13", "f32", "possup"), ("g13", "f16", "iabce"), ("g13", "bf16", "varifocal"), ("empty", "f32", "focal")])


def run_backward(crit, layers, targets, weights):
    leaves = dev_layers(layers, grad=True)
    losses = crit(R.as_outputs(leaves), targets)
    total = sum(weights[k] * v for k, v in losses.items() if v.grad_fn is not None)
    total.backward()
    return leaves


@pytest.mark.parametrize("name,dn,form", GRAD_CASES)
def test_gradients_every_element_vs_fp64_autograd(fx, name, dn, form):
    """backward() of sum_k w_k loss_k, one distinct weight per key: EVERY element of every pred_logits.grad and pred_boxes.grad against the
    restatement's fp64 autograd on the same rounded inputs. Bound per tensor: 4 x the reference's own |f32 - f64| gradient distance
    (fixture) + 1e-6 x the tensor's gradient maximum, plus for 16-bit inputs one rounding of the result (2^-11 / 2^-8 relative; 2^-25
    absolute in f16's subnormal range). For f32
    the fixture's sampled points of the reference's own f32 gradients under the same bound. Unmatched box rows exactly zero; a second
    run bit-identical. Measured maxima: profiles/r10a_criterion_train.txt."""
    s = TR.BATCHES[name]
    layers, targets = inputs(fx, name, dn)
    keys = [str(k) for k in fx[name + ".keys"]]
    w = TR.loss_weights(keys)
    idx = fixture_indices(fx, name, dn)
    _, ref, _ = TR.gradients(layers, targets, form, s["G"], w, indices=idx)
    crit, tg = new_criterion(form, s["G"], s["C"]), dev_targets(targets)
    leaves = run_backward(crit, layers, tg, w)
    assert np.array_equal(flat(crit.last_indices, 0), fx[f"{name}.{dn}.idx_q"])
    p = f"{name}.{dn}.{form}"
    gdist, gmax = fx[p + ".gdist"], fx[p + ".gmax"]
    for l, ((lg, bx), (rl, rb)) in enumerate(zip(leaves, ref)):
        assert lg.grad.dtype == lg.dtype and bx.grad.dtype == bx.dtype and lg.grad.shape == lg.shape and bx.grad.shape == bx.shape
        for k, (g, r, tag) in enumerate(((lg.grad, rl, "logits"), (bx.grad, rb, "boxes"))):
            got = g.double().cpu()
            assert torch.isfinite(got).all()
            base = 4.0 * gdist[l, k] + 1e-6 * gmax[l, k]
            excess = ((got - r).abs() - (ROUND[dn] * r.abs()).clamp(min=ROUND_ABS[dn])).max().item()
            print(f"{name} {dn} {form} layer {l} d/d{tag}: max |hip - fp64| = {(got - r).abs().max().item():.3e}, beyond one rounding {excess:.3e}, "
                  f"bound {base:.3e} (reference |f32 - f64| {gdist[l, k]:.3e}, max |grad| {gmax[l, k]:.3e})")
            assert excess <= base, (l, tag, excess, base)
            if dn == "f32":
                pts = got.reshape(-1).numpy() if k == 0 else box_rows(got, idx[l]).reshape(-1).numpy()
                want = fx[f"{p}.{'glog' if k == 0 else 'gbox'}32.{l}"].astype(np.float64)
                e = np.abs(pts[TR.sample_points(pts.size)] - want).max() if len(want) else 0.0
                assert e <= base, (l, tag, "reference f32 sample", e, base)
        matched = torch.zeros(bx.shape[:2], dtype=torch.bool)
        for b, (i, _) in enumerate(idx[l]):
            matched[b, torch.as_tensor(i)] = True
        assert not bx.grad.cpu()[~matched].any()                 # exactly zero off the matched rows
        assert (bx.grad.cpu()[matched] != 0).any(-1).all()
    again = run_backward(crit, layers, tg, w)
    assert all(torch.equal(a.grad, c.grad) and torch.equal(ab.grad, cb.grad) for (a, ab), (c, cb) in zip(leaves, again))


def test_gradient_flows_only_where_it_is_asked(fx):
    """Boxes that do not require grad get none; the logits' gradient is unchanged by that."""
    s = TR.BATCHES["g3"]
    layers, targets = inputs(fx, "g3", "f32")
    keys = [str(k) for k in fx["g3.keys"]]
    w, tg = TR.loss_weights(keys), dev_targets(targets)
    crit = new_criterion("focal", s["G"], s["C"])
    full = run_backward(crit, layers, tg, w)
    leaves = [(a.to(DEV).requires_grad_(True), b.to(DEV)) for a, b in layers]
    losses = crit(R.as_outputs(leaves), tg)
    sum(w[k] * v for k, v in losses.items() if v.grad_fn is not None).backward()
    assert all(b.grad is None and torch.equal(a.grad, fa.grad) for (a, b), (fa, _) in zip(leaves, full))


# ---------------------------------------------------------------------------------------------------- 4. no host synchronisation
def test_forward_and_backward_are_capturable_and_replay_bit_for_bit(fx):
    """Forward plus torch.autograd.grad captured with torch.cuda.graph on one stream (after a warm-up on that side stream); replays on other
    inputs written into the captured tensors reproduce the eager losses and gradients bit for bit. Nothing in forward or backward reads the device."""
    s = TR.BATCHES["g3"]
    layers, targets = inputs(fx, "g3", "f16")
    keys = [str(k) for k in fx["g3.keys"]]
    w, tg = TR.loss_weights(keys), dev_targets(targets)
    crit = new_criterion("possup", s["G"], s["C"])
    other = TR.batch_inputs("g3", 977, "f16")[0]

    def step(leaves):
        losses = crit(R.as_outputs(leaves), tg)
        total = sum(w[k] * v for k, v in losses.items() if v.grad_fn is not None)
        grads = torch.autograd.grad(total, [t for pair in leaves for t in pair])
        return losses, grads

    def snapshot(res):
        return {k: v.detach().clone() for k, v in res[0].items()}, [g.clone() for g in res[1]]

    eager_a, eager_b = snapshot(step(dev_layers(layers, grad=True))), snapshot(step(dev_layers(other, grad=True)))
    assert any(not torch.equal(eager_a[0][k], eager_b[0][k]) for k in keys)
    static = dev_layers(layers, grad=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static)                                             # warm-up: workspaces and offsets exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = step(static)
    for src, eager in ((other, eager_b), (layers, eager_a)):
        with torch.no_grad():
            for (sa, sb), (oa, ob) in zip(static, src):
                sa.copy_(oa.to(DEV))
                sb.copy_(ob.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(captured[0][k].detach(), eager[0][k]) for k in keys)
        assert all(torch.equal(g, e) for g, e in zip(captured[1], eager[1]))


# ---------------------------------------------------------------------------------------------------- 5. NaN
def test_nan_in_one_image_is_flagged_and_contained(fx):
    """Image 3 (37 targets of 37 queries per group) holds a NaN logit row in every group of every layer: the launches return (the trip counts
    are fixed), its problems report status 1 and still return perfect matchings of its 37 targets, the other images keep their pairs.
    (The same kind of input terminates on the host instantiation: tests/test_criterion_host.py::test_host_solver_terminates_on_non_finite_costs.)"""
    s = TR.BATCHES["g3"]
    layers, targets = inputs(fx, "g3", "f32")
    gw = s["nq"] // s["G"]
    poisoned = [(lg.clone(), bx) for lg, bx in layers]
    for lg, _ in poisoned:
        for g in range(s["G"]):
            lg[3, g * gw + 17, :] = float("nan")
    crit = new_criterion("focal", s["G"], s["C"])
    crit(R.as_outputs(dev_layers(poisoned)), dev_targets(targets))
    torch.cuda.synchronize()
    status = crit.matcher.status()
    assert status[:, :3].eq(0).all() and status[:, 3].eq(1).all()
    want = fixture_indices(fx, "g3", "f32")
    for l, lay in enumerate(crit.last_indices):
        for b in range(3):
            assert np.array_equal(lay[b][0].cpu().numpy(), want[l][b][0]) and np.array_equal(lay[b][1].cpu().numpy(), want[l][b][1])
        q, t = lay[3][0].cpu().numpy().reshape(s["G"], 37), lay[3][1].cpu().numpy().reshape(s["G"], 37)
        for g in range(s["G"]):
            assert np.array_equal(q[g], np.arange(g * gw, (g + 1) * gw)) and sorted(t[g].tolist()) == list(range(37))
