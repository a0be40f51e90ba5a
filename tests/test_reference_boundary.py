"""Drop-in boundaries against the UNMODIFIED reference, as recorded from it by oracle/gen_golden_boundary.py
(tests/golden/reference_boundary.json, reference_boundary_dets.npz). Each check runs tests/ref_boundary_driver.py in a child
process so the compat module name MultiScaleDeformableAttention never leaks into this test session."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _drive(what):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ref_boundary_driver.py"), what], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_b4_reference_op_file_binds_to_our_native_module():
    """models/ops/functions/ms_deform_attn_func.py:23 `import MultiScaleDeformableAttention as MSDA` (pybind names
    models/ops/src/vision.cpp:13-16) resolves to lw-detr_amd/compat, and the reference's own MSDeformAttnFunction calls
    straight into our operator (on host tensors it trips OUR argument contract, not an ImportError / AttributeError).
    The module name, the reference file and the calls it makes (with their arguments) are the recorded ones."""
    d = _drive("b4")
    assert d["module"] == "MultiScaleDeformableAttention"
    assert d["func_file"] == os.path.join("models", "ops", "functions", "ms_deform_attn_func.py")
    assert d["msda_file"].endswith(os.path.join("lw-detr_amd", "compat", "MultiScaleDeformableAttention.py"))
    assert d["fns"] == ["ms_deform_attn_backward", "ms_deform_attn_forward"]
    assert d["forward_is_ours"] and d["backward_is_ours"]
    assert d["host_calls"]["ms_deform_attn_forward"] == "RuntimeError: value must be a CUDA tensor"
    assert d["host_calls"]["ms_deform_attn_backward"] == "RuntimeError: value must be a CUDA tensor"


def test_b2_reference_evaluate_drives_our_model_and_postprocess():
    """The reference's engine.py:93-164, run as-is over a fake loader with our build_model() objects (the CPU oracle stands
    in for the HIP forward), a stub criterion and a recording CocoEvaluator, passed NestedTensors in and got PostProcess
    results keyed by image id: our forward + PostProcess in that loop's order give the detections it recorded; and f4 -
    lwdetr_amd.dist.to_coco_results / to_evaluator_update produce exactly what datasets/coco_eval.py:91-113,176-178 built
    from, and what the loop handed to the evaluator for, the same detections."""
    d = _drive("evaluate")
    assert d["forward_types"] == ["NestedTensor", "NestedTensor"] and d["iou_types"] == ["bbox"] and d["n_updates"] == 2
    assert d["loop_matches"]
    assert d["records_equal"] and d["n_records"] == 200 and d["update_equal"]
    assert "coco_eval_bbox" in d["stats_keys"]
    assert set(d["first_record"]) == {"image_id", "category_id", "bbox", "score"} and len(d["first_record"]["bbox"]) == 4
