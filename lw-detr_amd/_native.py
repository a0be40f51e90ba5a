"""ctypes binding of ``liblwdetr_hip.so`` (C ABI declared in ``include/lwdetr_hip.h``).

There is deliberately NO fallback: every entry point of the product path goes through this library, and
``lib()`` raises if it has not been built (``python -c 'import __graft_entry__ as g; g.build()'`` or
``make -C lw-detr_amd/csrc``).
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# LWDETR_HIP_LIB: tuning builds of the same library (tools/); the product always loads the in-tree one
LIB_PATH = os.environ.get("LWDETR_HIP_LIB") or os.path.join(_HERE, "liblwdetr_hip.so")
_lib = None

DT_F32, DT_F16, DT_BF16, DT_F64 = 0, 1, 2, 3
A_PLAIN, A_CONV3x3, A_PATCH16 = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU = 0, 1, 2, 3
OUT_LINEAR, OUT_HEADS, OUT_HEADS_T, OUT_TOKMAP, OUT_DECONV2x2 = 0, 1, 2, 3, 4
ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_LAUNCH = -1, -2, -3
ERRORS = {-1: "bad argument", -2: "unsupported configuration", -3: "kernel launch failed"}


class NativeError(RuntimeError):
    pass


class TokLayout(C.Structure):
    _fields_ = [("winmajor", C.c_int), ("Hp", C.c_int), ("Wp", C.c_int), ("Twp", C.c_int)]


class GemmSeg(C.Structure):
    _fields_ = [("out", C.c_void_p), ("out2", C.c_void_p), ("res", C.c_void_p), ("bias", C.c_void_p),
                ("gamma", C.c_void_p), ("rowmask", C.c_void_p), ("scale", C.c_float), ("act", C.c_int),
                ("mode", C.c_int), ("n_begin", C.c_int), ("n_end", C.c_int), ("ldo", C.c_long), ("ld2", C.c_long),
                ("ldres", C.c_long), ("res_mod", C.c_int), ("rowmask_after", C.c_int), ("p0", C.c_int), ("p1", C.c_int), ("p2", C.c_int),
                ("in_tok", TokLayout), ("out_tok", TokLayout), ("out_batch_stride", C.c_long),
                ("out_row_offset", C.c_long), ("ln_stats", C.c_void_p), ("ln_colsum", C.c_void_p)]


class GemmDesc(C.Structure):
    _fields_ = [("A", C.c_void_p), ("A2", C.c_void_p), ("W", C.c_void_p), ("M", C.c_int), ("N", C.c_int),
                ("K", C.c_int), ("lda", C.c_long), ("a_mode", C.c_int), ("a_tok", TokLayout),
                ("conv_cin", C.c_int), ("conv_stride", C.c_int), ("a_col0", C.c_int), ("conv_hout", C.c_int),
                ("conv_wout", C.c_int), ("img_h", C.c_int), ("img_w", C.c_int), ("nseg", C.c_int),
                ("seg", GemmSeg * 3), ("splitk_ws", C.c_void_p), ("splitk", C.c_int)]


class AttnDesc(C.Structure):
    _fields_ = [("Q", C.c_void_p), ("K", C.c_void_p), ("VT", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_long),
                ("B", C.c_int), ("heads", C.c_int), ("hd", C.c_int), ("Tp", C.c_int), ("seqs_per_img", C.c_int),
                ("seq_tok_stride", C.c_int), ("keys_per_seq", C.c_int), ("sub_stride", C.c_int),
                ("sub_len", C.c_int), ("kind", C.c_int), ("vt_slack", C.c_int)]


class AttnTrainDesc(C.Structure):
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("q_sb", C.c_long), ("q_sn", C.c_long), ("q_sh", C.c_long),
                ("k_sb", C.c_long), ("k_sn", C.c_long), ("k_sh", C.c_long), ("v_sb", C.c_long), ("v_sn", C.c_long), ("v_sh", C.c_long),
                ("o", C.c_void_p), ("o_ld", C.c_long), ("lse", C.c_void_p), ("B", C.c_int), ("heads", C.c_int), ("N", C.c_int),
                ("hd", C.c_int), ("scale", C.c_float)]


class MsdaTrainDesc(C.Structure):
    _fields_ = [("value", C.c_void_p), ("value_ld", C.c_long), ("offsets", C.c_void_p), ("offsets_ld", C.c_long), ("logits", C.c_void_p),
                ("logits_ld", C.c_long), ("ref", C.c_void_p), ("mask", C.c_void_p), ("shapes", C.c_void_p), ("level_start", C.c_void_p),
                ("B", C.c_int), ("S", C.c_int), ("M", C.c_int), ("D", C.c_int), ("L", C.c_int), ("Q", C.c_int), ("P", C.c_int), ("dtype", C.c_int)]


CHAIN_FULL, CHAIN_SIDE = 0, 1
CHAIN_RES, CHAIN_RELU, CHAIN_LN, CHAIN_STORE, CHAIN_ADDQ = 1, 2, 4, 8, 16


class ChainStage(C.Structure):
    _fields_ = [("kind", C.c_int), ("n", C.c_int), ("flags", C.c_int), ("eps", C.c_float), ("out", C.c_void_p), ("ldo", C.c_long)]


class ChainDesc(C.Structure):
    _fields_ = [("inp", C.c_void_p), ("ld_in", C.c_long), ("k_in", C.c_int), ("res", C.c_void_p), ("ld_res", C.c_long),
                ("qpos", C.c_void_p), ("ld_q", C.c_long), ("wstream", C.c_void_p), ("vec", C.c_void_p), ("M", C.c_long),
                ("D", C.c_int), ("nst", C.c_int), ("st", ChainStage * 6)]


CRIT_MAX_LAYERS, MATCH_MAX_NQ, CRIT_QCHUNK = 8, 1024, 32
LOSS_FOCAL, LOSS_IA_BCE = 0, 1
LOSS_VARIFOCAL, LOSS_POSITION_SUPERVISED = 2, 3


class CritLayer(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("boxes", C.c_void_p), ("class_error", C.c_int), ("reserved", C.c_int)]


COCOEVAL_MAX_DETS, COCOEVAL_MAX_GROUP, COCOEVAL_MAX_CATS, COCOEVAL_KEEP = 1024, 256, 1024, 100


class CocoGt(C.Structure):
    _fields_ = [("grp_off", C.c_void_p), ("box", C.c_void_p), ("area", C.c_void_p), ("crowd", C.c_void_p), ("cat", C.c_void_p),
                ("cat_lut", C.c_void_p), ("n_images", C.c_int), ("n_cats", C.c_int), ("lut_size", C.c_int), ("n_ann", C.c_int),
                ("max_group", C.c_int), ("reserved", C.c_int)]


MT_CHUNK = 1024
MT_PARAM, MT_EMA_F32, MT_EMA_I64 = 0, 1, 2
MT_SCALE_GRADS, MT_ADAMW, MT_EMA, MT_EMA_SET = 1, 2, 4, 8


class MtTensor(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("ema", C.c_void_p), ("numel", C.c_int64),
                ("kind", C.c_int32), ("skip", C.c_int32), ("decay_mul", C.c_float), ("neg_step_size", C.c_float), ("bc2_sqrt", C.c_float),
                ("reserved", C.c_int32)]


class MtChunk(C.Structure):
    _fields_ = [("tensor", C.c_int32), ("count", C.c_int32), ("offset", C.c_int64)]


class MtHyper(C.Structure):
    _fields_ = [("one_minus_beta1", C.c_float), ("beta2", C.c_float), ("one_minus_beta2", C.c_float), ("eps", C.c_float),
                ("ema_decay", C.c_float), ("ema_one_minus_decay", C.c_float)]


def is_built() -> bool:
    return os.path.exists(LIB_PATH)


def lib():
    """The loaded shared library; raises NativeError when it is missing (no CPU / eager fallback exists)."""
    global _lib
    if _lib is None:
        if not is_built():
            raise NativeError(f"lwdetr_amd: HIP extension {LIB_PATH} is missing - build it with "
                              "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
                              "There is no CPU fallback for the forward path.")
        l = C.CDLL(LIB_PATH)
        vp, i, lg, f = C.c_void_p, C.c_int, C.c_long, C.c_float
        l.lwdetr_msda_forward.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, vp]
        l.lwdetr_msda_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, vp]
        l.lwdetr_msda_fused_forward.argtypes = [vp, vp, vp, vp, lg, i, vp, vp, vp, i, i, i, i, i, i, i, i, vp]
        l.lwdetr_gemm.argtypes = [C.POINTER(GemmDesc), i, vp]
        l.lwdetr_gemm_few.argtypes = [C.POINTER(GemmDesc), i, vp]
        l.lwdetr_attention.argtypes = [C.POINTER(AttnDesc), i, vp]
        l.lwdetr_gemm_tuning.argtypes = [i]
        l.lwdetr_gemm_tuning.restype = None
        l.lwdetr_has_experiments.argtypes = []
        l.lwdetr_gemm_pt_tuning.argtypes = [i]
        l.lwdetr_gemm_pt_tuning.restype = None
        l.lwdetr_gemm_pt_count.argtypes = []
        l.lwdetr_gemm_pt_count.restype = C.c_long
        l.lwdetr_gemm_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_gemm_path_name.argtypes = [i]
        l.lwdetr_gemm_path_name.restype = C.c_char_p
        l.lwdetr_vit_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_vit_path_name.argtypes = [i]
        l.lwdetr_vit_path_name.restype = C.c_char_p
        l.lwdetr_msda_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_msda_path_name.argtypes = [i]
        l.lwdetr_msda_path_name.restype = C.c_char_p
        l.lwdetr_attn_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_attn_path_name.argtypes = [i]
        l.lwdetr_attn_path_name.restype = C.c_char_p
        l.lwdetr_mlp_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_mlp_path_name.argtypes = [i]
        l.lwdetr_mlp_path_name.restype = C.c_char_p
        l.lwdetr_chain_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_chain_path_name.argtypes = [i]
        l.lwdetr_chain_path_name.restype = C.c_char_p
        l.lwdetr_attention_tuning.argtypes = [i]
        l.lwdetr_attention_tuning.restype = None
        l.lwdetr_attention_tuning_cfg.argtypes = [i]
        l.lwdetr_attention_tuning_cfg.restype = None
        l.lwdetr_layernorm.argtypes = [vp, lg, vp, vp, vp, lg, lg, i, f, lg, lg, lg, i, vp]
        l.lwdetr_layernorm_chain.argtypes = [vp, lg, vp, vp, f, vp, lg, vp, vp, f, vp, lg, lg, i, i, vp]
        l.lwdetr_row_stats.argtypes = [vp, lg, lg, i, f, vp, i, vp]
        l.lwdetr_ffn_splits.argtypes = [lg, i, i, i]
        l.lwdetr_ffn_partial.argtypes = [vp, lg, vp, vp, vp, vp, lg, i, i, i, vp]
        l.lwdetr_ffn_finish.argtypes = [vp, lg, vp, i, vp, vp, vp, f, vp, lg, vp, vp, f, vp, lg, lg, i, i, vp]
        l.lwdetr_mlp_fused.argtypes = [vp, lg, vp, vp, vp, vp, vp, vp, lg, vp, lg, i, f, f, vp, lg, vp, vp, vp,
                                       vp, vp, vp, vp, vp, f, i, i, i, i, vp]
        l.lwdetr_vit_block_few.argtypes = [vp, lg, vp, vp, vp, vp, vp, vp, lg, vp, lg, i, f, f, vp, lg, vp, vp, vp,
                                       vp, vp, vp, vp, vp, f, i, i, i, i, vp]
        l.lwdetr_vit_block.argtypes = [vp, lg, vp, lg, vp, vp, vp, lg, vp, lg, i, f, f, i, vp, vp, vp, f, i, i, i, i, vp]
        l.lwdetr_vit_block_stream_bytes.argtypes = [i, i]
        l.lwdetr_vit_block_stream_bytes.restype = C.c_long
        l.lwdetr_vit_block_vec_floats.argtypes = [i]
        l.lwdetr_vit_block_vec_floats.restype = C.c_long
        l.lwdetr_vit_qkv.argtypes = [vp, lg, vp, vp, lg, i, f, vp, vp, vp, f, i, i, i, i, vp]
        l.lwdetr_vit_stem.argtypes = [vp, i, i, i, i, i, i, vp, lg, vp, lg, vp, vp, lg, i, f, vp, vp, vp, f, i, i, i, vp]
        l.lwdetr_vit_stem_stream_bytes.argtypes = [i]
        l.lwdetr_vit_stem_stream_bytes.restype = C.c_long
        l.lwdetr_vit_stem_vec_floats.argtypes = [i]
        l.lwdetr_vit_stem_vec_floats.restype = C.c_long
        l.lwdetr_vit_qkv_stream_bytes.argtypes = [i]
        l.lwdetr_vit_qkv_stream_bytes.restype = C.c_long
        l.lwdetr_vit_qkv_vec_floats.argtypes = [i]
        l.lwdetr_vit_qkv_vec_floats.restype = C.c_long
        l.lwdetr_enc_chain.argtypes = [vp, lg, i, vp, vp, vp, lg, vp, vp, i, vp, vp, vp, vp, lg, i, i, i, i, lg, i, f, f, i, vp]
        l.lwdetr_enc_chain_vec_floats.argtypes = [i, i]
        l.lwdetr_enc_chain_vec_floats.restype = C.c_long
        l.lwdetr_enc_chain_pieces.argtypes = [i, i, i]
        l.lwdetr_enc_chain_pieces.restype = C.c_long
        l.lwdetr_enc_chain_class_cols.argtypes = [i]
        l.lwdetr_enc_chain_class_cols.restype = C.c_long
        l.lwdetr_enc_chain_vec_floats_cls.argtypes = [i, i, i]
        l.lwdetr_enc_chain_vec_floats_cls.restype = C.c_long
        l.lwdetr_enc_chain_pieces_cls.argtypes = [i, i, i, i]
        l.lwdetr_enc_chain_pieces_cls.restype = C.c_long
        l.lwdetr_enc_chain_check.argtypes = [vp, lg, i, vp, vp, vp, lg, vp, vp, i, vp, vp, vp, vp, lg, i, i, i, i, lg, i, i]
        l.lwdetr_row_chain.argtypes = [C.POINTER(ChainDesc), i, vp]
        l.lwdetr_row_chain_pieces.argtypes = [C.POINTER(ChainDesc)]
        l.lwdetr_row_chain_pieces.restype = C.c_long
        l.lwdetr_row_chain_vec_floats.argtypes = [C.POINTER(ChainDesc)]
        l.lwdetr_row_chain_vec_floats.restype = C.c_long
        l.lwdetr_select_gather.argtypes = [vp, vp, lg, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]
        l.lwdetr_decoder_inputs.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]
        l.lwdetr_box_reparam.argtypes = [vp, vp, lg, vp, lg, i, vp]
        l.lwdetr_rowmax.argtypes = [vp, lg, lg, i, vp, i, vp]
        l.lwdetr_topk.argtypes = [vp, i, i, i, vp, vp, i, vp]
        l.lwdetr_postprocess.argtypes = [vp, vp, vp, i, i, i, i, vp, vp, vp, i, vp]
        l.lwdetr_postprocess_packed.argtypes = [vp, vp, vp, i, i, i, i, vp, i, vp]
        l.lwdetr_finalize_outputs.argtypes = [vp, vp, lg, vp, lg, vp, lg, i, vp, lg, i, vp]
        l.lwdetr_resize_normalize.argtypes = [vp, i, i, vp, vp, vp, vp, i, i, vp]
        l.lwdetr_augment_normalize.argtypes = [vp, vp, i, vp, lg, vp, lg, vp, vp, vp, i, i, i, vp]
        pl = C.POINTER(CritLayer)
        l.lwdetr_match_cost.argtypes = [pl, i, i, i, i, vp, vp, vp, vp, f, f, f, f, vp, i, vp]
        l.lwdetr_match_assign.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, vp, vp]
        l.lwdetr_match_assign_host.argtypes = [vp, i, i, vp, vp, vp, vp]
        l.lwdetr_criterion_partials_floats.argtypes = [i, i, i]
        l.lwdetr_criterion_partials_floats.restype = C.c_long
        l.lwdetr_criterion_partials.argtypes = [pl, i, i, i, i, vp, vp, vp, vp, vp, vp, i, f, vp, i, vp]
        l.lwdetr_criterion_finish.argtypes = [vp, pl, vp, vp, i, i, i, i, f, vp, vp]
        l.lwdetr_match_assign_groups.argtypes = [vp, vp, vp, i, i, i, i, vp, vp, vp, vp, vp]
        l.lwdetr_criterion_train_partials.argtypes = [pl, i, i, i, i, vp, vp, vp, vp, vp, vp, i, i, f, vp, i, vp]
        l.lwdetr_criterion_train_finish.argtypes = [vp, pl, vp, vp, i, i, i, i, i, f, vp, vp]
        l.lwdetr_criterion_backward.argtypes = [pl, pl, i, i, i, i, vp, vp, vp, vp, vp, vp, i, i, f, f, vp, i, vp]
        l.lwdetr_criterion_grad_host.argtypes = [vp, vp, i, i, vp, vp, i, vp, vp, i, i, f, f, vp, vp, vp]
        pg = C.POINTER(CocoGt)
        l.lwdetr_cocoeval_match.argtypes = [pg, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp]
        l.lwdetr_cocoeval_match_host.argtypes = [pg, vp, vp, i, i, vp, vp, vp, vp, vp, vp]
        l.lwdetr_cocoeval_npig.argtypes = [pg, vp, i, vp, vp]
        l.lwdetr_cocoeval_curves.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, lg, vp, vp, vp, vp]
        ph, u = C.POINTER(MtHyper), C.c_uint
        l.lwdetr_mt_check.argtypes = [vp, i, vp, i]
        l.lwdetr_mt_sumsq.argtypes = [vp, i, vp, i, vp, vp]
        l.lwdetr_mt_norm_finish.argtypes = [vp, i, C.c_double, vp, vp]
        l.lwdetr_mt_step.argtypes = [vp, i, vp, i, ph, u, vp, vp]
        l.lwdetr_mt_norm_host.argtypes = [vp, i, vp, i, C.c_double, vp]
        l.lwdetr_mt_step_host.argtypes = [vp, i, vp, i, ph, u, vp]
        l.lwdetr_mt_launch_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_mt_launch_name.argtypes = [i]
        l.lwdetr_mt_launch_name.restype = C.c_char_p
        pt = C.POINTER(AttnTrainDesc)
        l.lwdetr_attn_train_forward.argtypes = [pt, i, vp]
        l.lwdetr_attn_train_forward.restype = C.c_int
        l.lwdetr_attn_train_workspace_bytes.argtypes = [i, i, i, i, i]
        l.lwdetr_attn_train_workspace_bytes.restype = C.c_long
        l.lwdetr_attn_train_backward.argtypes = [pt, vp, lg, vp, vp, vp, lg, lg, lg, lg, lg, lg, lg, lg, lg, vp, i, vp]
        l.lwdetr_attn_train_backward.restype = C.c_int
        l.lwdetr_attn_train_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_attn_train_path_counts.restype = C.c_int
        l.lwdetr_attn_train_path_name.argtypes = [i]
        l.lwdetr_attn_train_path_name.restype = C.c_char_p
        pm = C.POINTER(MsdaTrainDesc)
        l.lwdetr_msda_train_forward.argtypes = [pm, vp, vp]
        l.lwdetr_msda_train_forward.restype = C.c_int
        l.lwdetr_msda_train_workspace_bytes.argtypes = [pm]
        l.lwdetr_msda_train_workspace_bytes.restype = C.c_long
        l.lwdetr_msda_train_backward.argtypes = [pm, vp, vp, vp, vp, vp, vp, lg, vp]
        l.lwdetr_msda_train_backward.restype = C.c_int
        l.lwdetr_msda_train_backward_host.argtypes = [vp, lg, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp, lg, vp, vp, vp]
        l.lwdetr_msda_train_backward_host.restype = C.c_int
        l.lwdetr_msda_train_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_msda_train_path_counts.restype = C.c_int
        l.lwdetr_msda_train_path_name.argtypes = [i]
        l.lwdetr_msda_train_path_name.restype = C.c_char_p
        l.lwdetr_two_stage_scores.argtypes = [vp, lg, vp, vp, vp, vp, vp, vp, vp, vp, lg, i, i, i, i, vp]
        l.lwdetr_two_stage_scores_check.argtypes = [vp, lg, vp, vp, vp, vp, vp, vp, vp, vp, lg, i, i, i, i]
        l.lwdetr_two_stage_gather.argtypes = [vp, lg, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]
        l.lwdetr_two_stage_gather_check.argtypes = [vp, lg, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i]
        l.lwdetr_two_stage_scatter_backward.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, vp]
        l.lwdetr_two_stage_scatter_backward_check.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i]
        for fn in ("lwdetr_two_stage_scores", "lwdetr_two_stage_scores_check", "lwdetr_two_stage_gather", "lwdetr_two_stage_gather_check",
                   "lwdetr_two_stage_scatter_backward", "lwdetr_two_stage_scatter_backward_check"):
            getattr(l, fn).restype = C.c_int
        l.lwdetr_two_stage_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_two_stage_path_counts.restype = C.c_int
        l.lwdetr_two_stage_path_name.argtypes = [i]
        l.lwdetr_two_stage_path_name.restype = C.c_char_p
        l.lwdetr_ln2d_forward.argtypes = [vp, vp, vp, vp, vp, vp, i, i, lg, f, i, i, vp]
        l.lwdetr_ln2d_forward.restype = C.c_int
        l.lwdetr_ln2d_workspace_floats.argtypes = [i, i, lg]
        l.lwdetr_ln2d_workspace_floats.restype = C.c_long
        l.lwdetr_ln2d_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, lg, i, i, lg, i, i, vp]
        l.lwdetr_ln2d_backward.restype = C.c_int
        l.lwdetr_sine_embed_forward.argtypes = [vp, lg, vp, vp, vp, lg, i, i, vp]
        l.lwdetr_sine_embed_forward.restype = C.c_int
        l.lwdetr_sine_embed_backward.argtypes = [vp, lg, vp, vp, vp, vp, lg, i, i, vp]
        l.lwdetr_sine_embed_backward.restype = C.c_int
        l.lwdetr_train_glue_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_train_glue_path_counts.restype = C.c_int
        l.lwdetr_train_glue_path_name.argtypes = [i]
        l.lwdetr_train_glue_path_name.restype = C.c_char_p
        l.lwdetr_drop_path_forward.argtypes = [vp, lg, vp, lg, vp, vp, vp, lg, lg, i, lg, i, i, vp]
        l.lwdetr_drop_path_forward.restype = C.c_int
        l.lwdetr_drop_path_workspace_floats.argtypes = [lg, i]
        l.lwdetr_drop_path_workspace_floats.restype = C.c_long
        l.lwdetr_drop_path_backward.argtypes = [vp, lg, vp, lg, vp, vp, vp, lg, vp, vp, lg, lg, i, lg, i, i, vp]
        l.lwdetr_drop_path_backward.restype = C.c_int
        l.lwdetr_drop_path_check.argtypes = [i, vp, lg, vp, lg, vp, vp, vp, lg, vp, vp, lg, lg, i, lg, i, i]
        l.lwdetr_drop_path_check.restype = C.c_int
        l.lwdetr_drop_path_path_counts.argtypes = [C.POINTER(C.c_long), i]
        l.lwdetr_drop_path_path_counts.restype = C.c_int
        l.lwdetr_drop_path_path_name.argtypes = [i]
        l.lwdetr_drop_path_path_name.restype = C.c_char_p
        l.lwdetr_tuning_set.argtypes = [C.c_char_p, lg, i]
        l.lwdetr_prof_enable.argtypes = [i]
        l.lwdetr_prof_num_kernels.argtypes = []
        l.lwdetr_prof_kernel_name.argtypes = [i]
        l.lwdetr_prof_kernel_name.restype = C.c_char_p
        l.lwdetr_prof_collect.argtypes = [vp, vp, vp, vp, i]
        for fn in ("lwdetr_msda_forward", "lwdetr_msda_backward", "lwdetr_msda_fused_forward", "lwdetr_gemm", "lwdetr_attention",
                   "lwdetr_layernorm", "lwdetr_layernorm_chain", "lwdetr_row_stats", "lwdetr_enc_chain", "lwdetr_enc_chain_check", "lwdetr_row_chain", "lwdetr_mlp_fused", "lwdetr_vit_block_few", "lwdetr_vit_block", "lwdetr_vit_qkv", "lwdetr_vit_stem", "lwdetr_ffn_splits", "lwdetr_ffn_partial", "lwdetr_ffn_finish", "lwdetr_select_gather", "lwdetr_decoder_inputs",
                   "lwdetr_box_reparam", "lwdetr_rowmax", "lwdetr_topk", "lwdetr_postprocess", "lwdetr_postprocess_packed", "lwdetr_finalize_outputs", "lwdetr_resize_normalize", "lwdetr_augment_normalize", "lwdetr_match_cost", "lwdetr_match_assign", "lwdetr_match_assign_host",
                   "lwdetr_criterion_partials", "lwdetr_criterion_finish", "lwdetr_match_assign_groups", "lwdetr_criterion_train_partials",
                   "lwdetr_criterion_train_finish", "lwdetr_criterion_backward", "lwdetr_criterion_grad_host", "lwdetr_cocoeval_match", "lwdetr_cocoeval_match_host", "lwdetr_cocoeval_npig",
                   "lwdetr_cocoeval_curves", "lwdetr_mt_check", "lwdetr_mt_sumsq", "lwdetr_mt_norm_finish", "lwdetr_mt_step", "lwdetr_mt_norm_host",
                   "lwdetr_mt_step_host", "lwdetr_mt_launch_counts", "lwdetr_mlp_path_counts", "lwdetr_chain_path_counts", "lwdetr_prof_enable", "lwdetr_prof_num_kernels", "lwdetr_prof_collect"):
            getattr(l, fn).restype = C.c_int
        _lib = l
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        raise NativeError(f"lwdetr_amd: {what} failed: {ERRORS.get(rc, rc)}")


def dtype_code(dt: torch.dtype) -> int:
    try:
        return {torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16, torch.float64: DT_F64}[dt]
    except KeyError:
        raise NativeError(f"lwdetr_amd: unsupported dtype {dt}") from None


def stream_ptr(device=None) -> int:
    """The current torch stream's hipStream_t, so kernels order with torch ops and get captured in HIP graphs."""
    return torch.cuda.current_stream(device).cuda_stream


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NativeError("lwdetr_amd: tensors must live on a ROCm device (cuda:N); there is no CPU path")


# ----------------------------------------------------------------------------------------------- profiling
def gemm_path_counts() -> dict:
    """{kernel family name: launches so far} of lwdetr_gemm / lwdetr_gemm_few in this process (lwdetr_gemm_path_counts)."""
    l = lib()
    n = l.lwdetr_gemm_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_gemm_path_counts(buf, n)
    return {l.lwdetr_gemm_path_name(i).decode(): int(buf[i]) for i in range(n)}


def vit_path_counts() -> dict:
    """{kernel instantiation name: launches so far} of lwdetr_vit_block / lwdetr_vit_qkv / lwdetr_vit_stem in this process (lwdetr_vit_path_counts)."""
    l = lib()
    n = l.lwdetr_vit_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_vit_path_counts(buf, n)
    return {l.lwdetr_vit_path_name(i).decode(): int(buf[i]) for i in range(n)}


def msda_path_counts() -> dict:
    """{kernel instantiation name: launches so far} of lwdetr_msda_forward / lwdetr_msda_backward / lwdetr_msda_fused_forward in this process (lwdetr_msda_path_counts)."""
    l = lib()
    n = l.lwdetr_msda_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_msda_path_counts(buf, n)
    return {l.lwdetr_msda_path_name(i).decode(): int(buf[i]) for i in range(n)}


def attn_path_counts() -> dict:
    """{kernel instantiation name: launches so far} of lwdetr_attention in this process (lwdetr_attn_path_counts)."""
    l = lib()
    n = l.lwdetr_attn_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_attn_path_counts(buf, n)
    return {l.lwdetr_attn_path_name(i).decode(): int(buf[i]) for i in range(n)}


def attn_train_path_counts() -> dict:
    """{kernel instantiation name: launches so far} of lwdetr_attn_train_forward / lwdetr_attn_train_backward in this process (lwdetr_attn_train_path_counts)."""
    l = lib()
    n = l.lwdetr_attn_train_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_attn_train_path_counts(buf, n)
    return {l.lwdetr_attn_train_path_name(i).decode(): int(buf[i]) for i in range(n)}


def msda_train_path_counts() -> dict:
    """{kernel instantiation name: launches so far} of lwdetr_msda_train_forward / lwdetr_msda_train_backward in this process (lwdetr_msda_train_path_counts)."""
    l = lib()
    n = l.lwdetr_msda_train_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_msda_train_path_counts(buf, n)
    return {l.lwdetr_msda_train_path_name(i).decode(): int(buf[i]) for i in range(n)}


def two_stage_path_counts() -> dict:
    """{kernel instantiation name: launches so far} of lwdetr_two_stage_scores / _gather / _scatter_backward in this process (lwdetr_two_stage_path_counts)."""
    l = lib()
    n = l.lwdetr_two_stage_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_two_stage_path_counts(buf, n)
    return {l.lwdetr_two_stage_path_name(i).decode(): int(buf[i]) for i in range(n)}


def train_glue_path_counts() -> dict:
    """{kernel instantiation name: launches so far} of lwdetr_ln2d_forward / _backward and lwdetr_sine_embed_forward / _backward in this process (lwdetr_train_glue_path_counts)."""
    l = lib()
    n = l.lwdetr_train_glue_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_train_glue_path_counts(buf, n)
    return {l.lwdetr_train_glue_path_name(i).decode(): int(buf[i]) for i in range(n)}


def drop_path_path_counts() -> dict:
    """{kernel instantiation name: launches so far} of lwdetr_drop_path_forward / _backward in this process (lwdetr_drop_path_path_counts)."""
    l = lib()
    n = l.lwdetr_drop_path_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_drop_path_path_counts(buf, n)
    return {l.lwdetr_drop_path_path_name(i).decode(): int(buf[i]) for i in range(n)}


def mlp_path_counts() -> dict:
    """{kernel instantiation name: launches so far} of lwdetr_mlp_fused / lwdetr_vit_block_few / lwdetr_ffn_partial in this process (lwdetr_mlp_path_counts)."""
    l = lib()
    n = l.lwdetr_mlp_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_mlp_path_counts(buf, n)
    return {l.lwdetr_mlp_path_name(i).decode(): int(buf[i]) for i in range(n)}


def chain_path_counts() -> dict:
    """{kernel instantiation name: launches so far} of lwdetr_enc_chain / lwdetr_row_chain in this process (lwdetr_chain_path_counts)."""
    l = lib()
    n = l.lwdetr_chain_path_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_chain_path_counts(buf, n)
    return {l.lwdetr_chain_path_name(i).decode(): int(buf[i]) for i in range(n)}


def mt_launch_counts() -> dict:
    """{entry name: launches so far} of lwdetr_mt_sumsq / lwdetr_mt_norm_finish / lwdetr_mt_step in this process (lwdetr_mt_launch_counts)."""
    l = lib()
    n = l.lwdetr_mt_launch_counts(None, 0)
    buf = (C.c_long * n)()
    l.lwdetr_mt_launch_counts(buf, n)
    return {l.lwdetr_mt_launch_name(i).decode(): int(buf[i]) for i in range(n)}


def tuning_set(name: str, value=None):
    """Override (value: int) or clear (None) one launch-path switch of the library (lwdetr_tuning_set; the LWDETR_* environment is read once per
    process, so tests and tools that switch inside a process go through here)."""
    check(lib().lwdetr_tuning_set(name.encode(), 0 if value is None else int(value), 0 if value is None else 1), f"tuning_set({name})")


def prof_enable(on: bool):
    check(lib().lwdetr_prof_enable(1 if on else 0), "prof_enable")


def prof_collect():
    """{kernel name: dict(ms, flops, bytes, count)} accumulated since the last call (synchronises recorded events)."""
    l = lib()
    n = l.lwdetr_prof_num_kernels()
    ms, fl, by = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
    cnt = (C.c_longlong * n)()
    check(l.lwdetr_prof_collect(ms, fl, by, cnt, n), "prof_collect")
    return {l.lwdetr_prof_kernel_name(k).decode(): dict(ms=ms[k], flops=fl[k], bytes=by[k], count=cnt[k])
            for k in range(n) if cnt[k]}
