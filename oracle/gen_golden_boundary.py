"""TEST INFRASTRUCTURE ONLY - record the reference's side of the drop-in boundaries into ``tests/golden/`` by running the
UNMODIFIED reference (``oracle/ref_shims.py`` finds it; it is absent where the tests run, so they read what this writes):

    python -m oracle.gen_golden_boundary

* B4 - ``models/ops/functions/ms_deform_attn_func.py`` imports ``MultiScaleDeformableAttention`` (pybind names
  ``models/ops/src/vision.cpp:13-16``) and calls it from its own ``MSDeformAttnFunction``: the module name, the file and
  every call it makes (function name, positional arguments as shape / dtype or value) are recorded through a stand-in module.
* B2 / f4 - ``engine.evaluate`` (``engine.py:93-164``) run as-is over a fake loader with our ``build_model()`` objects (the
  CPU oracle stands in for the HIP forward), a stub criterion and a recording CocoEvaluator: what the loop passed and
  produced (the detections keyed by image id) and the records ``datasets/coco_eval.py:91-113`` builds from them.

Writes ``tests/golden/reference_boundary.json`` and ``tests/golden/reference_boundary_dets.npz``; tests/test_reference_boundary.py
checks our side against them (through tests/ref_boundary_driver.py).
"""
import importlib
import json
import os
import sys
import types
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shims  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
REF = ref_shims.REFERENCE_ROOT
# the inputs of the B2 run; the test driver rebuilds them from these entries of the JSON
EVAL_CASE = {"size": "tiny", "state_dict_seed": 0, "images_seed": 7, "height": 192, "width": 256, "image_ids": [100, 101],
             "orig_size": [480, 640]}


def _describe(x):
    if isinstance(x, torch.Tensor):
        d = {"shape": list(x.shape), "dtype": str(x.dtype).split(".")[-1]}
        if not x.is_floating_point():
            d["values"] = x.tolist()
        return d
    return {"value": x}


def record_b4():
    ref_shims._install_shims()
    calls = []
    stub = types.ModuleType("MultiScaleDeformableAttention")

    def forward(*args):
        calls.append({"fn": "ms_deform_attn_forward", "args": [_describe(a) for a in args]})
        value, loc = args[0], args[3]
        return value.new_zeros(value.shape[0], loc.shape[1], value.shape[2] * value.shape[3])

    def backward(*args):
        calls.append({"fn": "ms_deform_attn_backward", "args": [_describe(a) for a in args]})
        return [torch.zeros_like(args[0]), torch.zeros_like(args[3]), torch.zeros_like(args[4])]
    stub.ms_deform_attn_forward, stub.ms_deform_attn_backward = forward, backward
    sys.modules["MultiScaleDeformableAttention"] = stub
    sys.path.insert(0, REF)
    f = importlib.import_module("models.ops.functions.ms_deform_attn_func")        # the reference's file, unmodified
    assert f.MSDA is stub
    v = torch.rand(1, 6, 2, 8, requires_grad=True)
    shapes = torch.tensor([[2, 3]], dtype=torch.long)
    lsi = torch.tensor([0], dtype=torch.long)
    loc = torch.rand(1, 4, 2, 1, 2, 2, requires_grad=True)
    aw = torch.rand(1, 4, 2, 1, 2, requires_grad=True)
    f.MSDeformAttnFunction.apply(v, shapes, lsi, loc, aw, 64).sum().backward()
    return {"module": f.MSDA.__name__, "func_file": os.path.relpath(f.__file__, REF), "calls": calls}


def record_evaluate():
    ref_shims._install_shims()
    sys.modules.pop("MultiScaleDeformableAttention", None)
    sys.path.insert(0, os.path.join(ROOT, "lw-detr_amd", "compat"))
    sys.path.insert(1, REF)
    # pycocotools is not installed: datasets/coco_eval.py only needs the names at import time (the evaluator is stubbed)
    for name in ("pycocotools", "pycocotools.cocoeval", "pycocotools.coco", "pycocotools.mask"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pycocotools.cocoeval"].COCOeval = object
    sys.modules["pycocotools.coco"].COCO = object
    sys.modules["pycocotools"].mask = sys.modules["pycocotools.mask"]
    pkg = types.ModuleType("datasets")                 # package shell: skips datasets/__init__.py (torchvision datasets)
    pkg.__path__ = [os.path.join(REF, "datasets")]
    sys.modules["datasets"] = pkg
    engine = importlib.import_module("engine")
    coco_eval = importlib.import_module("datasets.coco_eval")
    from util.misc import NestedTensor as RefNested

    import lwdetr_amd
    from lwdetr_amd.synth import synth_images, synth_state_dict
    from oracle import lwdetr_torch as O

    c = EVAL_CASE
    cfg = lwdetr_amd.get_args(c["size"])
    model, _, post = lwdetr_amd.build_model(cfg)
    sd = synth_state_dict(model.state_dict(), seed=c["state_dict_seed"])
    model.load_state_dict(sd)
    calls = {"forward_types": [], "updates": []}

    def host_forward(samples):      # the CPU oracle stands in for the HIP forward: this is about the call boundary
        calls["forward_types"].append(type(samples).__name__)
        return O.forward(sd, cfg, samples.tensors, samples.mask)
    model.forward = host_forward

    class Criterion:
        weight_dict = {"loss_ce": 2.0}

        def eval(self):
            return self

        def __call__(self, outputs, targets):
            assert set(outputs) >= {"pred_logits", "pred_boxes", "aux_outputs", "enc_outputs"}
            return {"loss_ce": outputs["pred_logits"].mean() * 0 + 1.0, "class_error": torch.tensor(0.0)}

    class Evaluator:
        def __init__(self, base_ds, iou_types):
            calls["iou_types"] = list(iou_types)
            self.coco_eval = {"bbox": Namespace(stats=torch.zeros(12))}

        def update(self, res):
            calls["updates"].append(res)

        def synchronize_between_processes(self):
            pass

        def accumulate(self):
            pass

        def summarize(self):
            pass
    engine.CocoEvaluator = Evaluator

    imgs = synth_images(len(c["image_ids"]), c["height"], c["width"], seed=c["images_seed"])
    loader = []
    for i, iid in enumerate(c["image_ids"]):
        samples = RefNested(imgs[i:i + 1], torch.zeros(1, c["height"], c["width"], dtype=torch.bool))
        loader.append((samples, [{"image_id": torch.tensor(iid), "orig_size": torch.tensor(c["orig_size"])}]))
    stats, _ = engine.evaluate(model, Criterion(), post, loader, None, torch.device("cpu"), Namespace(fp16_eval=False))
    res = {}
    for u in calls["updates"]:
        res.update(u)
    records = coco_eval.CocoEvaluator.prepare_for_coco_detection(None, res)
    ids = sorted(res)
    dets = {"image_ids": np.array(ids, dtype=np.int64)}
    for f in ("scores", "labels", "boxes"):
        dets[f] = np.stack([res[i][f].numpy() for i in ids])
    return {"case": c, "forward_types": calls["forward_types"], "iou_types": calls["iou_types"], "n_updates": len(calls["updates"]),
            "stats_keys": sorted(stats), "records": records}, dets


def main():
    if not ref_shims.reference_available():
        raise SystemExit(f"{REF} is not present: the boundary fixtures are recorded from the reference")
    if sys.argv[1:] == ["b4"]:
        print(json.dumps(record_b4()))
        return
    if sys.argv[1:] == ["evaluate"]:
        ev, dets = record_evaluate()
        np.savez_compressed(os.path.join(GOLDEN_DIR, "reference_boundary_dets.npz"), **dets)
        print(json.dumps(ev))
        return
    # each boundary in a child process of its own: the reference's top-level package names (models, util, datasets,
    # engine) and the two different MultiScaleDeformableAttention modules must not meet in one interpreter
    import subprocess
    out = {}
    for what in ("b4", "evaluate"):
        r = subprocess.run([sys.executable, "-m", "oracle.gen_golden_boundary", what], cwd=ROOT, capture_output=True, text=True, check=True)
        out[what] = json.loads(r.stdout.strip().splitlines()[-1])
    with open(os.path.join(GOLDEN_DIR, "reference_boundary.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", os.path.join(GOLDEN_DIR, "reference_boundary.json"), "and reference_boundary_dets.npz")


if __name__ == "__main__":
    main()
