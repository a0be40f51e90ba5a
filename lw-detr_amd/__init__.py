"""lwdetr_amd - MI355X-native LW-DETR inference forward path.

Public surface mirrors the reference's model API (``models/__init__.py:16-17``):
``build_model(args) -> (model, criterion, postprocessors)``; the operator API lives in
``lwdetr_amd.ops`` (``MSDeformAttnFunction``, ``MSDeformAttn``, ``ms_deform_attn_forward``).
"""
from .configs import SIZES, get_args  # noqa: F401

__version__ = "0.1.0"


def build_model(args):
    from .models import build_model as _build
    return _build(args)


def __getattr__(name):
    # the criterion classes of lwdetr_amd.models, resolved lazily as build_model resolves the model
    if name in ("HungarianMatcher", "SetCriterion", "build_criterion", "build_matcher", "GroupHungarianMatcher", "TrainSetCriterion",
                "build_group_matcher", "build_train_criterion"):
        from . import models
        return getattr(models, name)
    if name in ("CocoEvaluator", "CocoGroundTruth"):       # the native COCO box evaluator (coco_eval.py), resolved lazily as well
        from . import coco_eval
        return getattr(coco_eval, name)
    if name == "train":                                    # the training-step tail (train.py): NativeAdamW, ModelEma, clip_grad_norm_, get_param_dict
        import importlib
        return importlib.import_module(".train", __name__)
    if name == "augment":                                  # the training-time input transforms (augment.py): TrainTransform, sample_train_params, ...
        import importlib
        return importlib.import_module(".augment", __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
