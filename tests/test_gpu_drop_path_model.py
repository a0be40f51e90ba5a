"""GPU: drop-path in the differentiable model forward with the fused operators (``fused=None``).
  - the recording of tests/golden/drop_path_model.npz (the reference's ``large`` step with drop-path 0.3) in float32 with the recorded masks
    replayed: the two-stage indices equal the reference's; per group of quantities the figure against the float64 recording is at most
    MARGIN x the reference's own float32 figure (the rule of tests/test_gpu_train_model.py, both printed); the launch record shows six
    forward and six backward launches of the fused residual (two per block with a rate above 0); two further steps from the same state, with
    the convolution library asked for its deterministic kernels, give the same bits outside NONDETERMINISTIC;
  - under one torch.manual_seed, ``fused=None`` and ``fused=False`` collect identical masks;
  - bfloat16 autocast with the masks replayed: finite, the f32 + bf16 form served, figures within MARGIN x those of ``fused=False``;
  - eval(): the launch plan runs, equals a model built without drop-path bit for bit and draws nothing.
"""
import pytest
import torch

import drop_path_ref as DR
import lwdetr_amd
import train_model_ref as T
from lwdetr_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda"
# As in tests/test_gpu_train_model.py: the gradient of pos_embed passes through the bicubic F.interpolate, whose backward torch documents as
# non-deterministic on the GPU.
NONDETERMINISTIC = ("backbone.0.encoder.pos_embed",)


@pytest.fixture(scope="module")
def golden():
    return DR.load_golden()


def _moved(before):
    after = N.drop_path_path_counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _step(model, keep, fused=None, autocast=False):
    with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
        out, idx, used = DR.run_native(model, fused, device=DEV, keep=keep)
    assert torch.equal(torch.stack(used).cpu(), keep)
    q, _ = T.quantities(model, out, idx)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return q, grads


def test_float32_training_step_with_drop_path_against_the_reference_recording(golden):
    ref, ref_fig, names, seed, _, keep, _ = golden
    yard = T.group_figures(ref_fig)
    model = DR.build_native(seed, device=DEV)
    assert [n for n, _ in model.named_parameters()] == names
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    before = N.drop_path_path_counts()
    q, _ = _step(model, keep)
    torch.cuda.synchronize()
    moved = _moved(before)
    assert torch.equal(q["idx"], ref["idx"])
    got = T.group_figures(T.figures(q, ref))
    for g in T.GROUPS:
        print(f"drop-path {g}: figure {got[g]:.3e}, reference float32 figure {yard[g]:.3e}, bound {T.MARGIN * yard[g]:.3e}")
    assert moved == {"dp_fwd_f32_f32": DR.DRAWS, "dp_bwd_f32_f32": DR.DRAWS}, moved
    assert all(got[g] <= T.MARGIN * yard[g] for g in T.GROUPS), (got, yard)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        model.load_state_dict(state0)
        q1, grads1 = _step(model, keep)
        model.load_state_dict(state0)
        q2, grads2 = _step(model, keep)
    finally:
        torch.backends.cudnn.deterministic = was
    differing = [n for n in grads1 if not torch.equal(grads1[n], grads2[n])]
    print(f"drop-path: parameters whose gradient differs between two steps: {differing}")
    for k in q1:
        if k.startswith(("out.", "bn.")) or k == "idx":
            assert torch.equal(q1[k], q2[k]), k
    assert set(differing) <= set(NONDETERMINISTIC), differing


def test_fused_and_torch_draw_the_same_masks_under_one_seed(golden):
    seed, keep = golden[3], golden[5]
    model = DR.build_native(seed, device=DEV)
    with torch.no_grad():
        _, _, fused = DR.run_native(model, None, device=DEV, draw_seed=31)
        _, _, plain = DR.run_native(model, False, device=DEV, draw_seed=31)
        _, _, other = DR.run_native(model, None, device=DEV, draw_seed=32)
    assert len(fused) == len(plain) == DR.DRAWS
    assert all(m.is_cuda and m.dtype == torch.bool and tuple(m.shape) == (keep.shape[1],) for m in fused)
    assert all(torch.equal(a, b) for a, b in zip(fused, plain))
    assert not all(torch.equal(a, b) for a, b in zip(fused, other))          # the seed is what decides them


def test_bfloat16_autocast_step_with_drop_path(golden):
    ref, _, _, seed, _, keep, _ = golden
    model = DR.build_native(seed, device=DEV)
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    before = N.drop_path_path_counts()
    q_fused, _ = _step(model, keep, fused=None, autocast=True)
    assert _moved(before) == {"dp_fwd_f32_bf16": DR.DRAWS, "dp_bwd_f32_bf16": DR.DRAWS}
    model.load_state_dict(state0)
    before = N.drop_path_path_counts()
    q_torch, _ = _step(model, keep, fused=False, autocast=True)
    assert _moved(before) == {}
    assert T.is_finite(q_fused)
    for k in ref:
        assert q_fused[k].shape == ref[k].shape, k
    print("autocast: slots selected as in the recording - fused", float((q_fused["idx"] == ref["idx"]).float().mean()),
          "fused=False", float((q_torch["idx"] == ref["idx"]).float().mean()))
    got, yard = T.group_figures(T.figures(q_fused, ref)), T.group_figures(T.figures(q_torch, ref))
    for g in T.GROUPS:
        print(f"autocast drop-path {g}: fused figure {got[g]:.3e}, fused=False figure {yard[g]:.3e}, bound {T.MARGIN * yard[g]:.3e}")
    assert all(got[g] <= T.MARGIN * yard[g] for g in T.GROUPS), (got, yard)


def test_eval_mode_runs_the_launch_plan_and_draws_nothing():
    from lwdetr_amd.synth import synth_images, synth_state_dict
    # the shapes the launch plan takes (tests/test_gpu_train_model.py): the reduced tiny configuration with 100 queries at 192 x 256

    def build(drop_path):
        args = T.args_of("tiny")
        args.num_queries = args.num_select = 100
        args.drop_path = drop_path
        model, _, _ = lwdetr_amd.build_model(args)
        model.load_state_dict(synth_state_dict(model.state_dict(), seed=0), strict=True)
        return model.to(DEV)

    model, plain = build(DR.DROP_PATH), build(0.0)
    images = synth_images(2, 192, 256, seed=T.IMAGE_SEED).to(DEV)
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    model.train()
    col = {}
    model(images, _collect=col)                                     # the training forward draws: two masks for each of three blocks
    assert len(col["drop_path_keep"]) == 6
    model.load_state_dict(state0)                                   # the BatchNorm statistics the training forward moved
    model.eval()
    plain.eval()
    torch.manual_seed(5)
    state = torch.cuda.get_rng_state()
    before = N.drop_path_path_counts()
    with torch.no_grad():
        out = model(images)
        want = plain(images)
    torch.cuda.synchronize()
    assert torch.equal(torch.cuda.get_rng_state(), state) and _moved(before) == {}
    assert torch.equal(out["pred_logits"], want["pred_logits"]) and torch.equal(out["pred_boxes"], want["pred_boxes"])
