"""CPU: drop-path in the differentiable model forward, all torch (``fused=False``), and the drop-rate schedule.
  - train mode, float64, the recording's draw seed, against the recording of the reference's training step with drop-path 0.3
    (tests/golden/drop_path_model.npz, tools/gen_golden_drop_path.py): the six window masks equal the recorded ones, the two-stage indices too,
    and every figure is at most F64_TOL; replaying the recorded masks gives the same bits as drawing them;
  - the per-block rates after build and after update_drop_path are the reference's linspace values, block 0 holds nn.Identity, the state-dict
    keys are those of a model built without drop-path;
  - eval mode draws nothing (the generator's state is unchanged) and computes what a model without drop-path computes;
  - a model built with rate 0 still refuses a non-zero rate in training mode;
  - drop_scheduler equals the reference's arrays for the four recorded argument sets and asserts on bad modes;
  - the operator's torch formulation is timm's arithmetic, and the Function refuses CPU tensors.
"""
import numpy as np
import pytest
import torch
from torch import nn

import drop_path_ref as DR
import lwdetr_amd
import train_model_ref as T
from lwdetr_amd.models.train_forward import differentiable_forward


@pytest.fixture(scope="module")
def golden():
    return DR.load_golden()


@pytest.fixture(scope="module")
def drawn_step(golden):
    """The float64 step with the masks drawn under the recording's seed: (quantities, masks)."""
    _, _, names, seed, draw_seed, _, _ = golden
    model = DR.build_native(seed, torch.float64)
    assert [n for n, _ in model.named_parameters()] == names
    out, idx, used = DR.run_native(model, fused=False, dtype=torch.float64, draw_seed=draw_seed)
    q, _ = T.quantities(model, out, idx)
    return q, used


def test_float64_training_step_with_drop_path_equals_the_reference_recording(golden, drawn_step):
    ref, _, _, _, _, keep, _ = golden
    q, used = drawn_step
    assert len(used) == DR.DRAWS and all(m.dtype == torch.bool and tuple(m.shape) == (keep.shape[1],) for m in used)
    assert torch.equal(torch.stack(used), keep)
    assert all(0 < int(m.sum()) < m.numel() for m in used)          # every draw drops and keeps something: the recording exercises both
    assert torch.equal(q["idx"].cpu(), ref["idx"])
    assert set(q) == set(ref)
    fig = T.figures(q, ref)
    print(f"drop-path float64 figures per group {({g: f'{v:.3e}' for g, v in T.group_figures(fig).items()})}")
    worst = max(fig, key=fig.get)
    assert fig[worst] <= T.F64_TOL, (worst, fig[worst])


def test_replaying_the_recorded_masks_equals_drawing_them(golden, drawn_step):
    _, _, _, seed, _, keep, _ = golden
    q_drawn, _ = drawn_step
    model = DR.build_native(seed, torch.float64)
    torch.manual_seed(12345)                                        # the replay must not depend on the generator
    state = torch.get_rng_state()
    out, idx, used = DR.run_native(model, fused=False, dtype=torch.float64, keep=keep)
    assert torch.equal(torch.get_rng_state(), state)                # and must not consume it
    assert torch.equal(torch.stack(used), keep)
    q, _ = T.quantities(model, out, idx)
    for k in q_drawn:
        assert torch.equal(q[k], q_drawn[k]), k
    imgs = [t.double() for t in T.images_of(DR.NAME)]
    with pytest.raises(ValueError, match="fewer"):
        differentiable_forward(model, imgs, fused=False, drop_path_keep=list(keep[:3]))
    with pytest.raises(ValueError, match="more"):
        differentiable_forward(model, imgs, fused=False, drop_path_keep=list(keep) + [keep[0]])


def _rates(model):
    return [getattr(b.drop_path, "drop_prob", None) for b in model.backbone[0].encoder.blocks]


def test_rates_after_build_and_after_update_drop_path():
    args = DR.args_of()
    depth = args.vit_encoder_num_layers
    model, _, _ = lwdetr_amd.build_model(args)
    plain, _, _ = lwdetr_amd.build_model(T.args_of(DR.NAME))
    blocks = model.backbone[0].encoder.blocks
    assert type(blocks[0].drop_path) is nn.Identity
    assert all(len(list(b.drop_path.parameters())) == 0 and len(list(b.drop_path.buffers())) == 0 for b in blocks)
    want = [v.item() for v in torch.linspace(0, DR.DROP_PATH, depth)]
    assert _rates(model) == [None] + want[1:]
    assert list(model.state_dict()) == list(plain.state_dict())
    model.update_drop_path(0.15, depth)
    want = [v.item() for v in torch.linspace(0, 0.15, depth)]
    assert _rates(model) == [None] + want[1:]
    assert type(blocks[0].drop_path) is nn.Identity
    assert list(model.state_dict()) == list(plain.state_dict())
    # a model built with rate 0: every block holds nn.Identity and update_drop_path gives none of them a rate
    assert all(type(b.drop_path) is nn.Identity for b in plain.backbone[0].encoder.blocks)
    plain.update_drop_path(0.15, depth)
    assert _rates(plain) == [None] * depth


def test_eval_mode_draws_nothing(golden):
    _, _, _, seed, _, _, _ = golden
    model = DR.build_native(seed).eval()
    plain = T.build_native(DR.NAME, seed).eval()
    imgs = T.images_of(DR.NAME)
    torch.manual_seed(3)
    state = torch.get_rng_state()
    col = {}
    with torch.no_grad():
        out = differentiable_forward(model, imgs, fused=False, collect=col)
        want = differentiable_forward(plain, imgs, fused=False)
    assert torch.equal(torch.get_rng_state(), state)
    assert col["drop_path_keep"] == []
    assert torch.equal(out["pred_logits"], want["pred_logits"]) and torch.equal(out["pred_boxes"], want["pred_boxes"])
    # update_drop_path(0) on the model with containers: training mode draws nothing either
    model.train()
    model.update_drop_path(0.0, len(model.backbone[0].encoder.blocks))
    col = {}
    differentiable_forward(model, imgs, fused=False, collect=col)
    assert torch.equal(torch.get_rng_state(), state) and col["drop_path_keep"] == []


def test_a_model_built_without_drop_path_still_refuses_a_rate():
    model = T.build_native("tiny", 0)
    args = T.args_of("tiny")
    model.update_drop_path(0.1, args.vit_encoder_num_layers)
    with pytest.raises(NotImplementedError, match="drop-path") as e:
        model(T.images_of("tiny"))
    assert "args.drop_path > 0" in str(e.value) and "ignores" in str(e.value)
    model.update_drop_path(0.0, args.vit_encoder_num_layers)
    model(T.images_of("tiny"))


def test_dropout_is_still_refused_on_a_model_with_drop_path(golden):
    model = DR.build_native(golden[3])
    model.update_dropout(0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        model(T.images_of(DR.NAME))


def test_drop_scheduler_equals_the_reference_arrays(golden):
    from lwdetr_amd.train import drop_scheduler
    sched = golden[6]
    assert set(sched) == set(DR.SCHEDULES)
    for name, (rate, epochs, niter, cutoff, mode, schedule) in DR.SCHEDULES.items():
        got = drop_scheduler(rate, epochs, niter, cutoff_epoch=cutoff, mode=mode, schedule=schedule)
        assert isinstance(got, np.ndarray) and got.shape == (epochs * niter,) == sched[name].shape, name
        assert np.array_equal(np.asarray(got, dtype=np.float64), sched[name]), name
    assert np.array_equal(drop_scheduler(0.1, 2, 3), np.full(6, 0.1))                     # the defaults: standard, constant
    with pytest.raises(AssertionError):
        drop_scheduler(0.1, 2, 3, mode="sometimes")
    with pytest.raises(AssertionError):
        drop_scheduler(0.1, 2, 3, cutoff_epoch=1, mode="early", schedule="cosine")
    with pytest.raises(AssertionError):
        drop_scheduler(0.1, 2, 3, cutoff_epoch=1, mode="late", schedule="linear")


def test_torch_formulation_is_timms_arithmetic_and_the_function_refuses_the_cpu():
    from lwdetr_amd.ops import drop_path_keep, drop_path_residual, drop_path_residual_torch, drop_path_supports
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(6, 5, 7, generator=g, dtype=torch.float64), torch.randn(6, 5, 7, generator=g, dtype=torch.float64)
    gamma = torch.randn(7, generator=g, dtype=torch.float64)
    p = 0.3
    torch.manual_seed(11)
    keep = drop_path_keep(y, 6, p)
    torch.manual_seed(11)
    t = y.new_empty((6, 1, 1)).bernoulli_(1 - p)                    # timm's four lines
    assert keep.dtype == torch.bool and torch.equal(keep, t.reshape(6) != 0)
    t.div_(1 - p)
    assert torch.equal(drop_path_residual_torch(x, y, gamma, keep, p), x + (gamma * y) * t)
    assert torch.equal(drop_path_residual_torch(x, y, None, keep, p), x + y * t)
    assert not drop_path_supports(x, y) and not drop_path_supports(x.float(), y.float())
    with pytest.raises(RuntimeError, match="ROCm device"):
        drop_path_residual(x.float(), y.float(), gamma.float(), keep, p)
