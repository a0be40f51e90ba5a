"""GPU: the differentiable model forward with the fused operators (``fused=None``).
  - both recordings of tests/golden/train_model.npz in float32: the two-stage indices equal the reference's; per group of quantities
    (outputs, full gradients, gradient norms and sums, BatchNorm statistics) the figure against the float64 recording is at most MARGIN x the
    reference's own float32 figure (both printed); two further forward + backward passes from the same state, with the convolution
    library asked for its deterministic kernels, give bit-identical outputs and bit-identical gradients of every parameter outside
    NONDETERMINISTIC; the launch records show that the fused attention, deformable attention, two-stage and
    train_glue kernels served;
  - eval mode against the inference golden tiny_192x256 within FP32_TOL;
  - bfloat16 autocast on the first recording: finite, shapes unchanged, figures within MARGIN x those of ``fused=False`` under the same
    autocast. Measured: 82 % (fused) and 83 % (all torch) of the slots hold the recording's token - bfloat16 scores order near-equal tokens
    differently - so every figure but the BatchNorm one is of order one for both paths (outputs 0.888 / 0.888, full gradients 0.930 / 0.812,
    norms 0.734 / 0.696, BatchNorm 1.75e-3 / 1.72e-3): this case says that the two paths are equally far from the recording, no more;
  - three optimisation steps with TrainSetCriterion and NativeAdamW on the reduced tiny configuration, then eval(): the launch plan sees the
    trained weights (100 queries per group at 192 x 256: the launch plan refuses the recording's 10 queries and 128 x 128 images).
"""
import numpy as np
import pytest
import torch

import lwdetr_amd
import train_model_ref as T
from helpers import case_batch, golden_state_dict, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_TOL = 1e-3

# Parameters whose gradient passes through a torch operator that torch documents as non-deterministic on the GPU: the bicubic F.interpolate of
# pos_embed (upsample_bicubic2d_backward adds with atomics). Nothing is downstream of it but this one tensor. (Measured on an MI355X at the
# recordings' 8 x 8 token grid: it did not differ either; the entry stays because torch does not promise it.)
NONDETERMINISTIC = ("backbone.0.encoder.pos_embed",)


def _counts():
    from lwdetr_amd import _native as N
    return dict(attn=N.attn_train_path_counts(), msda=N.msda_train_path_counts(), two_stage=N.two_stage_path_counts(), glue=N.train_glue_path_counts())


def _delta(before, after):
    return {fam: {k: after[fam][k] - before[fam][k] for k in after[fam] if after[fam][k] != before[fam][k]} for fam in after}


def _step(model, name, fused=None, autocast=False):
    with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
        out, idx = T.run_native(model, name, fused, device=DEV)
    q, _ = T.quantities(model, out, idx)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return q, grads


@pytest.mark.parametrize("name", list(T.RECORDINGS))
def test_float32_training_step_against_the_reference_recording(name):
    ref, ref_fig, names, seed = T.load_golden(name)
    yard = T.group_figures(ref_fig)
    model = T.build_native(name, seed, device=DEV)
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    before = _counts()
    q, grads = _step(model, name)
    torch.cuda.synchronize()
    d = _delta(before, _counts())
    assert torch.equal(q["idx"], ref["idx"])
    got = T.group_figures(T.figures(q, ref))
    for g in T.GROUPS:
        print(f"{name} {g}: figure {got[g]:.3e}, reference float32 figure {yard[g]:.3e}, bound {T.MARGIN * yard[g]:.3e}")
    # the fused forms served: ViT attention + grouped decoder self-attention, deformable attention, two-stage scoring / gather / scatter,
    # one LayerNorm2d per level in the token layout and the sine embed
    args = T.args_of(name)
    levels = len(args.projector_scale)
    assert sum(d["attn"].values()) >= 2 * (args.vit_encoder_num_layers + args.dec_layers), d["attn"]
    assert sum(d["msda"].values()) >= 2 * args.dec_layers, d["msda"]
    d_model = args.hidden_dim
    assert d["two_stage"] == {f"ts_scores_f32_d{d_model}": 1, "ts_gather_f32": 1, "ts_scatter_f32": 1}, d["two_stage"]
    assert d["glue"] == {"ln2d_fwd_tok_f32": levels, "ln2d_bwd_tok_f32": levels, "sine_fwd_f32": 1, "sine_bwd_f32": 1}, d["glue"]
    assert all(got[g] <= T.MARGIN * yard[g] for g in T.GROUPS), (got, yard)
    # two more steps from the same state give the same bits as each other. (The step above was the process's first: the convolution library
    # chooses its kernels while it runs them for the first time, so its bits are not those of later calls. deterministic = True asks the
    # library for its deterministic kernels, as torch documents for reproducible convolutions.)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        model.load_state_dict(state0)
        q1, grads1 = _step(model, name)
        model.load_state_dict(state0)
        q2, grads2 = _step(model, name)
    finally:
        torch.backends.cudnn.deterministic = was
    differing = [n for n in grads1 if not torch.equal(grads1[n], grads2[n])]
    print(f"{name}: parameters whose gradient differs between two steps: {differing}")
    for k in q1:
        if k.startswith(("out.", "bn.")) or k == "idx":
            assert torch.equal(q1[k], q2[k]), k
    assert set(differing) <= set(NONDETERMINISTIC), differing


def test_eval_mode_on_the_gpu_equals_the_inference_golden():
    from lwdetr_amd.models.train_forward import differentiable_forward
    g = load_golden("tiny_192x256")
    size, images, mask = case_batch("tiny_192x256")
    model, _, _ = lwdetr_amd.build_model(lwdetr_amd.get_args(size))
    model.load_state_dict(golden_state_dict(g), strict=True)
    model = model.to(DEV).eval()
    col = {}
    with torch.no_grad():
        out = differentiable_forward(model, lwdetr_amd.models.NestedTensor(images.to(DEV), mask.to(DEV)), collect=col)
    ours, ref_idx, ref_sc = col["topk_idx"][0].cpu().numpy(), g["topk_idx"], g["enc_class_max"]
    gap = float(np.abs(np.take_along_axis(ref_sc, ours, 1) - np.take_along_axis(ref_sc, ref_idx, 1)).max())
    assert gap < 5e-5, f"top-k picked a different (non-tied) token: reference-score gap {gap}"
    assert np.array_equal(ours, ref_idx), "the selection of this golden has no ties inside the top num_queries"
    d = {"pred_logits": out["pred_logits"], "pred_boxes": out["pred_boxes"], "enc_logits": out["enc_outputs"]["pred_logits"],
         "enc_boxes": out["enc_outputs"]["pred_boxes"]}
    for j, aux in enumerate(out["aux_outputs"]):
        d[f"aux{j}_logits"], d[f"aux{j}_boxes"] = aux["pred_logits"], aux["pred_boxes"]
    diffs = {k: float(np.abs(v.float().cpu().numpy() - g[k]).max()) for k, v in d.items()}
    print(diffs)
    assert max(diffs.values()) < FP32_TOL, diffs


def test_bfloat16_autocast_step():
    name = "tiny"
    ref, _, names, seed = T.load_golden(name)
    model = T.build_native(name, seed, device=DEV)
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    q_fused, _ = _step(model, name, fused=None, autocast=True)
    model.load_state_dict(state0)
    q_torch, _ = _step(model, name, fused=False, autocast=True)
    assert T.is_finite(q_fused)
    for k in ref:
        assert q_fused[k].shape == ref[k].shape, k
    # bfloat16 scores may order near-equal tokens differently from the float64 recording; then a slot holds another query and its figure is
    # of order one for either path. How many slots agree is printed with the figures.
    print("autocast: slots selected as in the recording - fused", float((q_fused["idx"] == ref["idx"]).float().mean()),
          "fused=False", float((q_torch["idx"] == ref["idx"]).float().mean()))
    got, yard = T.group_figures(T.figures(q_fused, ref)), T.group_figures(T.figures(q_torch, ref))
    for g in T.GROUPS:
        print(f"autocast {g}: fused figure {got[g]:.3e}, fused=False figure {yard[g]:.3e}, bound {T.MARGIN * yard[g]:.3e}")
    assert all(got[g] <= T.MARGIN * yard[g] for g in T.GROUPS), (got, yard)


def test_three_optimisation_steps_then_eval():
    from lwdetr_amd.models.criterion_train import build_train_criterion
    from lwdetr_amd.models.train_forward import differentiable_forward
    from lwdetr_amd.train import NativeAdamW
    from lwdetr_amd.synth import synth_images, synth_state_dict
    # the reduced tiny configuration at the shapes the inference launch plan takes: it refuses the recording's 10 queries per group (its
    # head-major GEMM outputs want a multiple of 4) and runs the goldens from 192 x 256 pixels up, so: tiny's own 100 queries, 192 x 256
    args = T.args_of("tiny")
    args.num_queries = args.num_select = 100
    model, _, _ = lwdetr_amd.build_model(args)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=0), strict=True)
    model = model.to(DEV)
    criterion = build_train_criterion(args, 91).to(DEV).train()
    images = synth_images(2, 192, 256, seed=T.IMAGE_SEED).to(DEV)
    targets = [{"labels": torch.tensor([3, 17], device=DEV), "boxes": torch.tensor([[0.3, 0.4, 0.2, 0.3], [0.7, 0.6, 0.25, 0.2]], device=DEV)},
               {"labels": torch.tensor([5], device=DEV), "boxes": torch.tensor([[0.5, 0.5, 0.4, 0.4]], device=DEV)}]
    model.eval()
    with torch.no_grad():
        before_eval = model(images)["pred_logits"].clone()
    model.train()
    p0 = {n: p.detach().clone() for n, p in model.named_parameters()}
    b0 = {k: v.clone() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    opt = NativeAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    losses = []
    for _ in range(3):
        out = model(images, targets)
        loss_dict = criterion(out, targets)
        loss = sum(loss_dict[k] * criterion.weight_dict[k] for k in loss_dict if k in criterion.weight_dict)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", losses)
    assert all(np.isfinite(losses))
    moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), p0[n])]
    assert len(moved) > 0.9 * len(p0), f"only {len(moved)} of {len(p0)} parameters moved"
    sd = model.state_dict()
    assert all(not torch.equal(sd[k], b0[k]) for k in b0)
    model.eval()
    with torch.no_grad():
        after_eval = model(images)
        want = differentiable_forward(model, images)
    assert not torch.equal(after_eval["pred_logits"], before_eval)
    dl = float((after_eval["pred_logits"].float() - want["pred_logits"].float()).abs().max())
    db = float((after_eval["pred_boxes"].float() - want["pred_boxes"].float()).abs().max())
    print("launch plan vs differentiable forward after training:", dl, db)
    assert dl < FP32_TOL and db < FP32_TOL, (dl, db)
