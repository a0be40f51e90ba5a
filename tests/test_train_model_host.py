"""CPU: the assembly of the differentiable model forward (lwdetr_amd/models/train_forward.py), all torch (``fused=False``).
  - train mode, float64, against both recordings of the unmodified reference's training step (tests/golden/train_model.npz,
    tools/gen_golden_train_model.py): the two-stage indices, every output, every gradient quantity and the BatchNorm running statistics to
    float64 rounding (F64_TOL, the sibling host tests' float64 bound; the figure of every group is printed);
  - eval mode, float32, against the inference goldens tiny_192x256 and small_padded within FP32_TOL = 1e-3, the gate of tests/test_gpu_model.py;
  - the contract: output keys and shapes under train(), _packed_weights() under train(), dropout and drop-path, state-dict keys.
"""
import numpy as np
import pytest
import torch

import lwdetr_amd
import train_model_ref as T
from helpers import case_batch, golden_state_dict, load_golden
from lwdetr_amd.models.train_forward import differentiable_forward

FP32_TOL = 1e-3


@pytest.mark.parametrize("name", list(T.RECORDINGS))
def test_float64_training_step_equals_the_reference_recording(name):
    ref, _, names, seed = T.load_golden(name)
    model = T.build_native(name, seed, torch.float64)
    assert [n for n, _ in model.named_parameters()] == names
    out, idx = T.run_native(model, name, fused=False, dtype=torch.float64)
    assert torch.equal(idx.cpu(), ref["idx"])
    q, _ = T.quantities(model, out, idx)
    assert set(q) == set(ref)
    fig = T.figures(q, ref)
    groups = T.group_figures(fig)
    print(f"{name}: float64 figures per group {({g: f'{v:.3e}' for g, v in groups.items()})}")
    worst = max(fig, key=fig.get)
    assert fig[worst] <= T.F64_TOL, (worst, fig[worst])


@pytest.mark.parametrize("name", ["tiny_192x256", "small_padded"])
def test_eval_mode_float32_equals_the_inference_golden(name):
    g = load_golden(name)
    size, images, mask = case_batch(name)
    model, _, _ = lwdetr_amd.build_model(lwdetr_amd.get_args(size))
    model.load_state_dict(golden_state_dict(g), strict=True)
    model.eval()
    col = {}
    with torch.no_grad():
        out = differentiable_forward(model, lwdetr_amd.models.NestedTensor(images, mask), fused=False, collect=col)
    assert np.array_equal(col["topk_idx"][0].numpy(), g["topk_idx"])
    d = {"pred_logits": out["pred_logits"], "pred_boxes": out["pred_boxes"], "enc_logits": out["enc_outputs"]["pred_logits"],
         "enc_boxes": out["enc_outputs"]["pred_boxes"]}
    for j, aux in enumerate(out["aux_outputs"]):
        d[f"aux{j}_logits"], d[f"aux{j}_boxes"] = aux["pred_logits"], aux["pred_boxes"]
    diffs = {k: float(np.abs(v.numpy() - g[k]).max()) for k, v in d.items()}
    print(name, diffs)
    assert max(diffs.values()) < FP32_TOL, diffs


def _tiny():
    model = T.build_native("tiny", 0)
    return model, T.args_of("tiny")


def test_train_mode_forward_returns_the_reference_keys_and_group_shapes():
    model, args = _tiny()
    keys = set(model.state_dict())
    B, Q, ncls = 2, args.group_detr * args.num_queries, 91
    out = model(T.images_of("tiny"), targets=[{"anything": 1}])
    assert set(out) == {"pred_logits", "pred_boxes", "aux_outputs", "enc_outputs"}
    assert out["pred_logits"].shape == (B, Q, ncls) and out["pred_boxes"].shape == (B, Q, 4)
    assert len(out["aux_outputs"]) == args.dec_layers - 1
    assert all(a["pred_logits"].shape == (B, Q, ncls) and a["pred_boxes"].shape == (B, Q, 4) for a in out["aux_outputs"])
    assert out["enc_outputs"]["pred_logits"].shape == (B, Q, ncls) and out["enc_outputs"]["pred_boxes"].shape == (B, Q, 4)
    assert out["pred_logits"].requires_grad and out["enc_outputs"]["pred_boxes"].requires_grad
    out["pred_logits"].sum().backward()
    assert model.class_embed.weight.grad is not None and model.backbone[0].encoder.patch_embed.proj.weight.grad is not None
    assert set(model.state_dict()) == keys
    # a dense tensor and a list of equal images are the same batch
    dense = torch.stack([T.images_of("tiny")[0]] * 2)
    a, b = model(dense), model(list(dense))
    assert torch.equal(a["pred_logits"], b["pred_logits"])


def test_packed_weights_still_raise_under_train():
    model, _ = _tiny()
    with pytest.raises(NotImplementedError, match="model.eval"):
        model._packed_weights()


def test_dropout_and_drop_path_are_refused_in_the_training_forward():
    model, args = _tiny()
    imgs = T.images_of("tiny")
    model.update_dropout(0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        model(imgs)
    model.update_dropout(0.0)
    model.update_drop_path(0.1, args.vit_encoder_num_layers)
    with pytest.raises(NotImplementedError, match="drop-path"):
        model(imgs)
    model.update_drop_path(0.0, args.vit_encoder_num_layers)
    model(imgs)
    model.update_dropout(0.1)
    model.eval()                                   # dropout is the identity in eval mode: nothing to refuse
    with torch.no_grad():
        differentiable_forward(model, imgs, fused=False)


def test_state_dict_keys_are_those_of_the_reference_recording():
    _, _, names, seed = T.load_golden("large")
    model = T.build_native("large", seed)
    assert [n for n, _ in model.named_parameters()] == names


def test_patch_decoder_and_layer_norm_2d_leave_other_configurations_alone():
    from lwdetr_amd.ops import patch_decoder, patch_layer_norm_2d
    model, _ = _tiny()
    keys = set(model.state_dict())
    assert patch_decoder(model.transformer) == 1
    model.transformer.decoder.lite_refpoint_refine = False
    assert patch_decoder(model.transformer) == 0
    assert patch_layer_norm_2d(model) == 0          # the containers' LayerNorm2d has no normalized_shape; token LayerNorms are nn.LayerNorm

    class ChannelsFirstNorm(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.weight, self.bias = torch.nn.Parameter(torch.ones(8)), torch.nn.Parameter(torch.zeros(8))
            self.eps, self.normalized_shape = 1e-6, (8,)

    holder = torch.nn.Sequential(ChannelsFirstNorm(), torch.nn.LayerNorm(8))
    assert patch_layer_norm_2d(holder) == 1
    assert set(model.state_dict()) == keys
