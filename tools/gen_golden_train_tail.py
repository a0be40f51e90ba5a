"""Writes the two fixtures of the training-step-tail tests from the UNMODIFIED reference, on the CPU (needs the reference checkout, through
oracle/ref_shims.py):
    python tools/gen_golden_train_tail.py
tests/golden/train_tail_param_groups.json : for the reference's tiny and small models, what util/get_param_dicts.get_param_dict returns with
    non-trivial arguments (ARGS below), as name -> [lr, weight_decay] in the order of the groups; a group without a weight_decay key (every
    parameter outside the ViT encoder) is recorded with args.weight_decay, the value torch.optim.AdamW(weight_decay=args.weight_decay) gives it.
tests/golden/train_tail_ema.npz : a small Conv + BatchNorm module's state dict at four moments (model.<k>.<name>: the inputs) and the state
    of the reference's util/utils.ModelEma after set(model.0) and after each of three update(model.k) (ema.<k>.<name>), decay 0.9997,
    num_batches_tracked included (int64: the reference's copy_ truncates the f32 result).
Both files hold recorded results only.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import lwdetr_amd  # noqa: E402
from oracle import ref_shims  # noqa: E402

ARGS = dict(lr=1e-4, lr_encoder=1.5e-4, lr_vit_layer_decay=0.8, lr_component_decay=0.7, weight_decay=1e-4)
NBT = (5, 6, 4000, 40000)      # num_batches_tracked at set and at the three updates: 5 -> 5 (5.0003), -> 6 (6.198), -> 17 (17.998)


def param_groups(size):
    args = lwdetr_amd.get_args(size)
    for k, v in ARGS.items():
        setattr(args, k, v)
    model, _ = ref_shims.build_reference_model(args)
    from util.get_param_dicts import get_param_dict          # the reference's
    with contextlib.redirect_stdout(io.StringIO()):           # it prints two lines per encoder parameter
        groups = get_param_dict(args, model)
    names = {id(p): n for n, p in model.named_parameters()}
    out = {}
    for g in groups:
        p = g["params"]
        assert isinstance(p, torch.nn.Parameter) and names[id(p)] not in out
        out[names[id(p)]] = [float(g["lr"]), float(g.get("weight_decay", args.weight_decay))]
    assert len(out) == sum(p.requires_grad for p in model.parameters())
    return out


def ema_module():
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))


def ema_fixture():
    ref_shims.import_reference()
    from util.utils import ModelEma                            # the reference's
    g = torch.Generator().manual_seed(77)
    model = ema_module()
    ema = ModelEma(model, decay=0.9997)
    out = {}
    for k, nbt in enumerate(NBT):
        with torch.no_grad():
            for name, t in model.state_dict().items():
                t.copy_(torch.tensor(nbt) if t.dtype == torch.int64 else torch.randn(t.shape, generator=g) * (0.5 + k))
        (ema.set if k == 0 else ema.update)(model)
        for name, t in model.state_dict().items():
            out[f"model.{k}.{name}"] = t.numpy().copy()
        for name, t in ema.module.state_dict().items():
            out[f"ema.{k}.{name}"] = t.numpy().copy()
    assert [int(out[f"ema.{k}.1.num_batches_tracked"]) for k in range(4)] == [5, 5, 6, 17]
    return out


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    groups = {"args": ARGS, "tiny": param_groups("tiny"), "small": param_groups("small")}
    path = os.path.join(gold, "train_tail_param_groups.json")
    with open(path, "w") as f:
        json.dump(groups, f, indent=0)
    print(path, os.path.getsize(path), "bytes;", {k: len(v) for k, v in groups.items()})
    path = os.path.join(gold, "train_tail_ema.npz")
    np.savez_compressed(path, **ema_fixture())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
