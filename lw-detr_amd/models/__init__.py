"""Model API of the reference (``models/__init__.py:16-17``)."""
from .criterion import HungarianMatcher, SetCriterion, build_criterion, build_matcher  # noqa: F401
from .criterion_train import GroupHungarianMatcher, TrainSetCriterion, build_group_matcher, build_train_criterion  # noqa: F401
from .lwdetr import LWDETR, PostProcess, build  # noqa: F401
from .nested import NestedTensor, nested_tensor_from_tensor_list  # noqa: F401


def build_model(args):
    return build(args)
