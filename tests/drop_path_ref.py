"""What the drop-path tests and tools/gen_golden_drop_path.py share: the configuration of the recording, its loader and the native runs.

The golden (tests/golden/drop_path_model.npz) is the training step of tests/train_model_ref.py - same quantities, figures, images, cotangents -
recorded from the reference's ``large`` model in the reduced configuration, built with ``drop_path = 0.3`` (4 blocks: rates 0, 0.1, 0.2, 0.3, so
six draws of 2 images x 16 windows) with timm's DropPath restated by the tool. ``torch.manual_seed(draw_seed)`` is set immediately before the
forward. The file also holds the six masks, both seeds and the reference scheduler's arrays for the argument sets of SCHEDULES.
"""
import os

import numpy as np
import torch

import train_model_ref as T

GOLDEN_PATH = os.path.join(T.ROOT, "tests", "golden", "drop_path_model.npz")
NAME = "large"
DROP_PATH = 0.3
DRAWS = 6
# name -> (drop_rate, epochs, niter_per_ep, cutoff_epoch, mode, schedule)
SCHEDULES = {"standard": (0.1, 3, 5, 0, "standard", "constant"), "early_constant": (0.1, 4, 3, 2, "early", "constant"),
             "early_linear": (0.2, 5, 4, 3, "early", "linear"), "late": (0.15, 4, 3, 1, "late", "constant")}


def args_of():
    args = T.args_of(NAME)
    args.drop_path = DROP_PATH
    return args


def load_golden():
    """-> (reference quantities, recorded float32 figures, parameter names, weight seed, draw seed, masks (DRAWS, B * 16) bool, schedules)."""
    z = np.load(GOLDEN_PATH, allow_pickle=False)
    pre = NAME + "__"
    ref = {k[len(pre) + 3:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith(pre + "q__")}
    fig = {k[len(pre) + 3:]: float(z[k]) for k in z.files if k.startswith(pre + "f__")}
    names = [str(s) for s in z[pre + "param_names"]]
    sched = {k[len("sched__"):]: np.asarray(z[k]) for k in z.files if k.startswith("sched__")}
    return ref, fig, names, int(z[pre + "seed"]), int(z[pre + "draw_seed"]), torch.from_numpy(np.asarray(z[pre + "keep"])), sched


def build_native(seed, dtype=torch.float32, device="cpu"):
    """This package's model for the recording, built with the recording's drop-path rate and loaded with its weights, in train mode."""
    import lwdetr_amd
    from lwdetr_amd.synth import synth_state_dict
    model, _, _ = lwdetr_amd.build_model(args_of())
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=seed), strict=True)
    return model.to(device=device, dtype=dtype).train()


def run_native(model, fused, device="cpu", dtype=torch.float32, keep=None, draw_seed=None):
    """-> (output dict, indices, masks used). ``keep``: masks to replay; else ``draw_seed`` seeds the default generators just before."""
    from lwdetr_amd.models.train_forward import differentiable_forward
    imgs = [t.to(device=device, dtype=dtype) for t in T.images_of(NAME)]
    col = {}
    if keep is None and draw_seed is not None:
        torch.manual_seed(draw_seed)
    out = differentiable_forward(model, imgs, fused=fused, collect=col, drop_path_keep=None if keep is None else list(keep))
    return out, col["topk_idx"], col["drop_path_keep"]
