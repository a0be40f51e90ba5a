"""TEST INFRASTRUCTURE ONLY - records tests/golden/drop_path_model.npz from the reference model built with drop-path (``models.build_model``, found
by oracle/ref_shims.py; it is absent where the tests run, so they read what this writes).

timm is not installed where this runs and oracle/ref_shims.py stands in an identity for its ``DropPath``, so this tool sets its own restatement
of timm's ``DropPath`` (``drop_path`` with ``scale_by_keep``: ``t = x.new_empty((x.shape[0], 1, 1)).bernoulli_(keep); t.div_(keep); x * t``;
the identity for rate 0 or in eval mode) in the shim module and in the reference's ``models.backbone.vit`` before the model is built. The
restatement records every mask it draws and can replay a list of masks instead of drawing.

The step is the one of tools/gen_golden_train_model.py (its quantities, figures, images and cotangents, by import) for the reduced ``large``
configuration with ``drop_path = 0.3`` (rates 0, 0.1, 0.2, 0.3: six draws of 32 windows), weights ``synth_state_dict(seed)`` with the seed of
tests/golden/train_model.npz. ``torch.manual_seed(draw_seed)`` is set immediately before the float64 forward; the float32 yardstick run replays
the float64 run's masks. The draw seed is the first from 7 up for which every draw holds at least one dropped and one kept window and the
float32 run selects the same tokens as the float64 run. The weights are those of the recording without drop-path, so the stricter
decided-selection rule of tools/gen_golden_train_model.py (a gap of 64 x the score bound) is not a condition here: dropping windows moves the
scores, and no draw seed below 64 met it. Its margin (smallest gap / (64 x bound)) is printed.

Also stored: the six masks, both seeds, and the arrays of the reference's ``util.drop_scheduler.drop_scheduler`` for the four argument sets of
``drop_path_ref.SCHEDULES``. The file holds data only.
Run:  python tools/gen_golden_drop_path.py
"""
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import drop_path_ref as DR  # noqa: E402
import train_model_ref as T  # noqa: E402
import gen_golden_train_model as G  # noqa: E402
from lwdetr_amd.synth import synth_state_dict  # noqa: E402
from oracle import ref_shims  # noqa: E402


class DropPath(nn.Module):
    """timm.models.layers.DropPath (scale_by_keep=True), restated. ``drawn`` collects the masks; ``replay`` (an iterator) replaces the draws."""
    drawn = []
    replay = None

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1 - self.drop_prob
        if DropPath.replay is None:
            t = x.new_empty((x.shape[0], 1, 1)).bernoulli_(keep)
        else:
            t = next(DropPath.replay).to(x.dtype).reshape(x.shape[0], 1, 1).clone()
        DropPath.drawn.append(t.reshape(-1) != 0)
        t.div_(keep)
        return x * t


def import_reference_with_drop_path():
    models = ref_shims.import_reference()
    import models.backbone.vit as vit
    sys.modules["timm.models.layers"].DropPath = DropPath
    vit.DropPath = DropPath
    return models


def run_reference(seed, dtype, draw_seed=None, replay=None):
    """-> (quantities, parameter names, what the transformer was handed, model, masks) of the reference's train-mode step in ``dtype``."""
    models = import_reference_with_drop_path()
    from models.ops.modules import MSDeformAttn
    from util.misc import nested_tensor_from_tensor_list
    args = DR.args_of()
    model, _, _ = models.build_model(args)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=seed), strict=True)
    for m in model.modules():
        if isinstance(m, MSDeformAttn):
            m._export = True
    model = model.to(dtype).train()
    rates = [getattr(b.drop_path, "drop_prob", 0.0) for b in model.backbone[0].encoder.blocks]
    assert [round(r, 6) for r in rates] == [0.0, 0.1, 0.2, 0.3], rates
    seen, picked = {}, []
    model.transformer.register_forward_pre_hook(lambda _m, a: seen.update(srcs=a[0], masks=a[1]))
    real_topk = torch.topk

    def topk(*a, **k):
        out = real_topk(*a, **k)
        picked.append(out[1].clone())
        return out

    samples = nested_tensor_from_tensor_list([t.to(dtype) for t in T.images_of(DR.NAME)])
    DropPath.drawn, DropPath.replay = [], (None if replay is None else iter(replay))
    torch.topk = topk
    try:
        if draw_seed is not None:
            torch.manual_seed(draw_seed)
        out = model(samples)
    finally:
        torch.topk = real_topk
        DropPath.replay = None
    masks = torch.stack(DropPath.drawn)
    assert masks.shape == (DR.DRAWS, 16 * len(T.images_of(DR.NAME))), masks.shape
    q, names = T.quantities(model, out, torch.stack(picked))
    return q, names, seen, model, masks


def schedules():
    import_reference_with_drop_path()
    from util.drop_scheduler import drop_scheduler
    return {k: np.asarray(drop_scheduler(a[0], a[1], a[2], cutoff_epoch=a[3], mode=a[4], schedule=a[5]), dtype=np.float64)
            for k, a in DR.SCHEDULES.items()}


def main():
    if not ref_shims.reference_available():
        raise SystemExit("the reference is not present: this fixture is recorded from it")
    seed = T.load_golden(DR.NAME)[3]
    for draw_seed in range(7, 64):
        q64, names, seen, model, masks = run_reference(seed, torch.float64, draw_seed=draw_seed)
        kept = masks.sum(1).tolist()
        if not all(0 < k < masks.shape[1] for k in kept):
            print(f"draw seed {draw_seed}: kept {kept} - a draw keeps or drops everything, next seed")
            continue
        _, margin, own = G.decided(DR.NAME, seen, model)
        assert torch.equal(q64["idx"], own), "the reference's top-k differs from the float64 restatement's"
        q32, names32, _, _, masks32 = run_reference(seed, torch.float32, replay=list(masks))
        assert names32 == names and torch.equal(masks32, masks)
        if not torch.equal(q32["idx"], q64["idx"]):
            print(f"draw seed {draw_seed}: the float32 and float64 reference runs selected different tokens, next seed")
            continue
        break
    else:
        raise SystemExit("no draw seed below 64 qualifies")
    fig = T.figures(q32, q64)
    print(f"weight seed {seed}, draw seed {draw_seed}: kept {kept} of {masks.shape[1]}; smallest gap / (64 x bound) {margin:.2f}; float32 figures per "
          "group:", {g: f"{v:.3e}" for g, v in T.group_figures(fig).items()})
    pre = DR.NAME + "__"
    rec = {pre + "seed": np.int64(seed), pre + "draw_seed": np.int64(draw_seed), pre + "drop_path": np.float64(DR.DROP_PATH),
           pre + "keep": masks.numpy(), pre + "param_names": np.array(names)}
    for k, v in q64.items():
        rec[pre + "q__" + k] = v.numpy()
    for k, v in fig.items():
        rec[pre + "f__" + k] = np.float64(v)
    for k, v in schedules().items():
        rec["sched__" + k] = v
    np.savez_compressed(DR.GOLDEN_PATH, **rec)
    print("wrote", DR.GOLDEN_PATH, os.path.getsize(DR.GOLDEN_PATH), "bytes")


if __name__ == "__main__":
    main()
