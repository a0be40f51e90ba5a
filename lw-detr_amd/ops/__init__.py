"""Operator API of the reference (``models/ops/functions/__init__.py:13``, ``models/ops/modules/__init__.py:9``)."""
from .attention import Attention, FusedAttentionFunction, fused_attention, patch_vit_attention  # noqa: F401
from .deform_train import FusedMSDeformAttnFunction, MSDeformAttnTrain, patch_deformable_attention  # noqa: F401
from .functions import (MSDeformAttnFunction, ms_deform_attn_backward, ms_deform_attn_core_pytorch,  # noqa: F401
                        ms_deform_attn_forward)
from .modules import MSDeformAttn  # noqa: F401
from .train_glue import (LayerNorm2dFunction, SineEmbedFunction, layer_norm_2d, patch_layer_norm_2d,  # noqa: F401
                         query_sine_embed)
from .drop_path import (DropPathResidualFunction, drop_path_keep, drop_path_residual, drop_path_residual_torch,  # noqa: F401
                        drop_path_supports)
from .decoder_train import (decoder_forward, decoder_layer_forward, grouped_self_attention, patch_decoder)  # noqa: F401
from .two_stage import SelectRowsFunction, patch_two_stage, two_stage_scores, two_stage_select  # noqa: F401
