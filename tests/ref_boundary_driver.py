"""TEST INFRASTRUCTURE. Runs in a child process of tests/test_reference_boundary.py: checks our side of the drop-in boundaries
SURVEY section 8(b) names - B4 (the native module name), B2 (engine.evaluate drives our objects), f4 (COCO result records) -
against what the UNMODIFIED reference did at them, recorded in tests/golden/reference_boundary.json / reference_boundary_dets.npz
(oracle/gen_golden_boundary.py). Prints one JSON object; the parent asserts on it."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)


def _golden():
    with open(os.path.join(GOLDEN, "reference_boundary.json")) as fh:
        return json.load(fh)


def _materialise(desc):
    """One recorded positional argument of the reference's call -> a host value of that shape / dtype (integer tensors
    carry their recorded values)."""
    import torch
    if "value" in desc:
        return desc["value"]
    dtype = getattr(torch, desc["dtype"])
    if "values" in desc:
        return torch.tensor(desc["values"], dtype=dtype).reshape(desc["shape"])
    return torch.rand(desc["shape"], dtype=dtype)


def check_b4():
    g = _golden()["b4"]
    # the name the reference's op file imports resolves to lw-detr_amd/compat exactly as INTEGRATION.md section 2 describes
    sys.path.insert(0, os.path.join(ROOT, "lw-detr_amd", "compat"))
    msda = importlib.import_module(g["module"])
    from lwdetr_amd.ops import functions as ours
    out = {"module": msda.__name__, "func_file": g["func_file"], "msda_file": msda.__file__,
           "fns": sorted({c["fn"] for c in g["calls"]}), "host_calls": {}}
    out["forward_is_ours"] = msda.ms_deform_attn_forward is ours.ms_deform_attn_forward
    out["backward_is_ours"] = msda.ms_deform_attn_backward is ours.ms_deform_attn_backward
    # every call the reference's MSDeformAttnFunction makes, with its recorded arguments on the host: it reaches our entry
    # point and trips OUR argument contract (not a TypeError over the arity, not an AttributeError)
    for c in g["calls"]:
        try:
            getattr(msda, c["fn"])(*[_materialise(d) for d in c["args"]])
            out["host_calls"][c["fn"]] = "no error"
        except Exception as e:      # noqa: BLE001
            out["host_calls"][c["fn"]] = f"{type(e).__name__}: {e}"
    return out


def check_evaluate():
    import torch
    import lwdetr_amd
    from lwdetr_amd import dist as D
    from lwdetr_amd.synth import synth_images, synth_state_dict
    from oracle import lwdetr_torch as O

    g = _golden()["evaluate"]
    dets = np.load(os.path.join(GOLDEN, "reference_boundary_dets.npz"))
    c = g["case"]
    cfg = lwdetr_amd.get_args(c["size"])
    model, _, post = lwdetr_amd.build_model(cfg)
    sd = synth_state_dict(model.state_dict(), seed=c["state_dict_seed"])
    model.load_state_dict(sd)

    # what engine.py:93-164's loop computes per batch with our objects: the CPU oracle forward (standing in for the HIP
    # forward, as in the recorded run) on the NestedTensor's tensors and mask, then our PostProcess on the stacked
    # orig_size of the targets, keyed by image id
    imgs = synth_images(len(c["image_ids"]), c["height"], c["width"], seed=c["images_seed"])
    res = {}
    with torch.no_grad():
        for i, iid in enumerate(c["image_ids"]):
            outputs = O.forward(sd, cfg, imgs[i:i + 1], torch.zeros(1, c["height"], c["width"], dtype=torch.bool))
            assert set(outputs) >= {"pred_logits", "pred_boxes", "aux_outputs", "enc_outputs"}
            results = post["bbox"](outputs, torch.stack([torch.tensor(c["orig_size"])], dim=0))
            res[iid] = results[0]
    ids = sorted(res)
    loop = {f: torch.stack([res[i][f] for i in ids]).numpy() for f in ("scores", "labels", "boxes")}
    loop_matches = (ids == dets["image_ids"].tolist() and np.array_equal(loop["labels"], dets["labels"])
                    and np.allclose(loop["scores"], dets["scores"], rtol=0, atol=2e-6)
                    and np.allclose(loop["boxes"], dets["boxes"], rtol=0, atol=2e-3))

    # f4 - lwdetr_amd.dist.to_coco_results / to_evaluator_update on exactly the detections the reference's loop produced
    # vs what datasets/coco_eval.py:91-113 built from them (records) and what the loop handed to the evaluator (update)
    rid = torch.from_numpy(dets["image_ids"])
    scores, labels, boxes = (torch.from_numpy(dets[f]) for f in ("scores", "labels", "boxes"))
    records = D.to_coco_results(rid, scores, labels, boxes)
    upd = D.to_evaluator_update(rid, scores, labels, boxes)
    same_update = sorted(upd) == rid.tolist() and all(
        torch.equal(upd[int(k)][f], t[j]) for j, k in enumerate(rid) for f, t in (("scores", scores), ("labels", labels), ("boxes", boxes)))
    return {"forward_types": g["forward_types"], "iou_types": g["iou_types"], "n_updates": g["n_updates"],
            "loop_matches": bool(loop_matches), "records_equal": records == g["records"], "n_records": len(records),
            "update_equal": bool(same_update), "stats_keys": g["stats_keys"], "first_record": records[0]}


if __name__ == "__main__":
    print(json.dumps(check_b4() if sys.argv[1] == "b4" else check_evaluate()))
