"""ctypes binding of libmae_hip.so (C ABI declared in include/mae_hip.h).

The product path has no CPU fallback: if the shared library is missing or a symbol is absent this module raises,
loudly, at import time.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C ssrl_vit_mae_jepa_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("MAE_HIP_LIB") or _HERE / "lib" / "libmae_hip.so")  # MAE_HIP_LIB: an alternate build of the same library (kernel experiments)

MAE_F32, MAE_BF16, MAE_U8 = 0, 1, 2
PARAM_TRAINABLE, PARAM_FROZEN, PARAM_UNUSED, PARAM_MATRIX = 1, 2, 4, 8
LOSS_MSE, LOSS_SMOOTH_L1 = 0, 1
POOL_CLS, POOL_MEAN, POOL_MEAN_PATCHES, POOL_CLS_MEAN_PATCHES = 0, 1, 2, 3
FEAT_NONE, FEAT_L2 = 0, 1
ATTN_QUERY_CLS, ATTN_QUERY_MEAN = 0, 1
EPI_NONE, EPI_GELU, EPI_RESID, EPI_DGELU, EPI_GELU_GRAD, EPI_MUL, EPI_GELU_ACT = 0, 1, 2, 3, 4, 5, 6
AUG_NONE, AUG_AUTOCONTRAST, AUG_EQUALIZE, AUG_INVERT, AUG_POSTERIZE, AUG_SOLARIZE, AUG_SOLARIZE_ADD, AUG_COLOR, AUG_CONTRAST, AUG_BRIGHTNESS, \
    AUG_SHARPNESS, AUG_AFFINE = range(12)
AUG_GEOMETRIC = 0x100  # MAE_AUG_GEOMETRIC, or-ed into out_dtype
AUG_BILINEAR, AUG_BICUBIC, AUG_BILINEAR_ROUND, AUG_BICUBIC_ROUND = 0, 1, 2, 3  # AFFINE modes
ABI_VERSION = 4
NORM_PIX_EPS = 1e-6  # MAE_NORM_PIX_EPS
GRAD_ACC_BLOCKS = 2048  # MAE_GRAD_ACC_BLOCKS: grid cap of mae_engine_grad_accumulate (256 threads x 4 floats a block: one sweep covers 1024 x this many floats)


class MaeConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "image_size", "patch_size", "in_chans", "embed_dim", "depth", "num_heads",
        "decoder_embed_dim", "decoder_depth", "decoder_num_heads", "mlp_ratio", "act_dtype", "pred_dim", "norm_pix_loss")] + [
        ("reserved", C.c_int32 * 3)]


class MaeHipError(RuntimeError):
    pass


def _load() -> C.CDLL:
    if not LIB_PATH.exists():
        raise ImportError(
            f"libmae_hip.so not found at {LIB_PATH}: the HIP extension is not built. "
            "Run `make -C ssrl_vit_mae_jepa_amd/csrc` (needs hipcc, --offload-arch=gfx950). "
            "There is no CPU fallback for this path.")
    return C.CDLL(os.fspath(LIB_PATH), mode=C.RTLD_GLOBAL)


lib = _load()

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
_pp = C.POINTER

# name -> (restype, argtypes); every symbol of include/mae_hip.h
SIGNATURES = {
    "mae_last_error": (C.c_char_p, []),
    "mae_abi_version": (C.c_int, []),
    "mae_engine_create": (C.c_int, [_pp(MaeConfig), _pp(_vp)]),
    "mae_engine_destroy": (None, [_vp]),
    "mae_engine_num_params": (_i64, [_vp]),
    "mae_engine_arena_elems": (_i64, [_vp]),
    "mae_engine_trainable_elems": (_i64, [_vp]),
    "mae_engine_param_info": (C.c_int, [_vp, _i64, _pp(C.c_char_p), _pp(_i64), _pp(_i64), _pp(_i32), _i64 * 4, _pp(_i32)]),
    "mae_engine_workspace_bytes": (_i64, [_vp, _i32, _i32]),
    "mae_engine_wcache_bytes": (_i64, [_vp]),
    "mae_engine_refresh_weights": (C.c_int, [_vp, _vp, _vp, _vp]),
    "mae_mask_from_noise": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mae_engine_forward_encoder": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _vp, _vp]),
    "mae_engine_forward_decoder": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "mae_patchify_gather": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mae_patchify_gather_norm": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mae_norm_pix_restore": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mae_mse_loss_norm_pix": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _i32, _vp, _vp]),
    "mae_augment_crop_flip_u8": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "mae_resize_crop_flip": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "mae_mse_loss": (C.c_int, [_vp, _vp, _i64, _f32, _vp, _vp, _vp, _vp]),
    "mae_engine_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "mae_engine_loss_and_grads": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _f32, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "mae_engine_encoder_grad_elems": (_i64, [_vp]),
    "mae_engine_backward_decoder": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp]),
    "mae_engine_backward_encoder": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _vp, _vp]),
    "mae_engine_decoder_decode": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp]),
    "mae_engine_grad_ready_points": (_i32, [_vp, _pp(_i64), _i32]),
    "mae_engine_loss_and_grads_phased": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _f32, _vp, _i64, _vp, _vp, _vp, _vp, _pp(_vp), _i32, _vp]),
    "mae_engine_optimizer_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _f32, _i64, _vp, _vp, _vp]),
    "mae_engine_jepa_workspace_bytes": (_i64, [_vp, _i32, _i32, _i32, _i32]),
    "mae_engine_jepa_loss_and_grads": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _i64,
                                                 _vp, _vp, _vp, _vp, _pp(_vp), _i32, _vp]),
    "mae_engine_grad_sumsq_range": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "mae_engine_clip_from_sumsq": (C.c_int, [_vp, _vp, _f32, _vp, _vp]),
    "mae_engine_adamw_range": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _i64, _vp, _i64, _i64, _vp]),
    "mae_engine_grad_accumulate": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, _vp]),
    "mae_engine_classifier_workspace_bytes": (_i64, [_vp, _i32, _i32]),
    "mae_engine_classifier_forward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "mae_engine_classifier_loss_and_grads": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _i64,
                                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mae_engine_classifier_workspace_bytes_ex": (_i64, [_vp, _i32, _i32, _i32]),
    "mae_engine_classifier_forward_ex": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "mae_engine_classifier_loss_and_grads_ex": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _i64,
                                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mae_engine_classifier_loss_and_grads_soft": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _i64,
                                                            _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp]),
    "mae_engine_classifier_loss_and_grads_sd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _i64,
                                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp]),
    "mae_mix_batch": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mae_augment_ops_u8": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _vp]),
    "mae_engine_grad_sumsq_buffer": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "mae_engine_adamw_buffer": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _i64, _vp, _vp]),
    "mae_engine_refresh_transposed_range": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp]),
    "mae_engine_features_workspace_bytes": (_i64, [_vp, _i32, _i32]),
    "mae_engine_extract_features": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "mae_engine_extract_layer_features": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _pp(_i32), _i32, _vp, _i64, _vp, _vp]),
    "mae_reconstruct_scratch_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "mae_reconstruct_compose": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mae_engine_reconstruct": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _f32, _i32, _vp, _i64, _vp, _vp, _vp, _vp,
                                         _vp, _i64, _vp]),
    "mae_knn_scratch_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "mae_knn_topk": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "mae_knn_vote": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _i32, _f32, _vp, _vp, _vp]),
    "mae_engine_optimizer_step_ema": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _f32, _i64, _vp, _vp, _vp, _vp, _f32, _vp]),
    "mae_engine_timers_enable": (C.c_int, [_vp, _i32]),
    "mae_engine_timer_count": (_i32, [_vp]),
    "mae_engine_timer_name": (C.c_char_p, [_vp, _i32]),
    "mae_engine_timer_read": (C.c_int, [_vp, _i32, _pp(C.c_double), _pp(_i64), _pp(C.c_double), _pp(C.c_double)]),
    "mae_engine_timers_reset": (C.c_int, [_vp]),
    "mae_layernorm_fwd": (C.c_int, [_vp, _vp, _vp, _vp, _f32, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mae_add_layernorm_fwd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mae_layernorm_bwd": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mae_add_layernorm_fwd_scaled": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "mae_layernorm_bwd_scaled": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "mae_classifier_head_scratch_bytes": (_i64, [_i32, _i32, _i32]),
    "mae_classifier_head": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mae_classifier_head_ex": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mae_classifier_head_soft": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                           _vp, _vp, _f32, _vp]),
    "mae_batchnorm_scratch_bytes": (_i64, [_i64, _i32]),
    "mae_batchnorm_fwd": (C.c_int, [_vp, _i64, _i32, _f32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mae_lars_step": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _f32, _f32, _f32, _f32, _vp, _vp, _vp]),
    "mae_batchnorm_stats": (C.c_int, [_vp, _i64, _i32, _f32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mae_probe_sweep_scratch_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "mae_probe_sweep_head": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mae_lars_step_groups": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _i64, _i32, _vp, _vp, _f32, _f32, _vp, _vp, _i64, _vp]),
    "mae_attn_pool_fwd": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp]),
    "mae_attn_pool_bwd_scratch_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "mae_attn_pool_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _i64, _vp]),
    "mae_attn_probe_fold": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "mae_attn_probe_fold_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "mae_attn_probe_project": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "mae_attn_probe_project_bwd_scratch_bytes": (_i64, [_i64, _i32, _i32]),
    "mae_attn_probe_project_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "mae_engine_tokens_workspace_bytes": (_i64, [_vp, _i32, _i32]),
    "mae_engine_extract_tokens": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "mae_engine_attention_workspace_bytes": (_i64, [_vp, _i32, _i32]),
    "mae_engine_extract_attention": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _pp(_i32), _i32, _vp, _vp, _vp, _i64, _vp]),
    "mae_linear_fwd": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mae_linear_wgrad_scratch_bytes": (_i64, [_i64, _i32, _i32]),
    "mae_linear_wgrad": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mae_linear_wgrad_pair_scratch_bytes": (C.c_int64, [_i64, _i32, _i32, _i32, _i32]),
    "mae_linear_wgrad_pair": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _i32, _vp, _vp]),
    "mae_attention_fwd": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mae_attention_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mae_attention_colsum_max_tokens": (_i32, [_i32, _i32]),
    "mae_attention_colsum": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "mae_tsne_pitch": (_i32, [_i32]),
    "mae_tsne_scratch_bytes": (_i64, [_i32, _i32]),
    "mae_tsne_affinities": (C.c_int, [_vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "mae_tsne_gradient": (C.c_int, [_vp, _vp, _i32, _f32, _vp, _vp, _vp, _i64, _vp]),
    "mae_tsne_update": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _f32, _f32, _f32, _vp]),
    "mae_tsne_step": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _f32, _f32, _f32, _f32, _vp, _vp, _vp, _i64, _vp]),
    "mae_umap_scratch_bytes": (_i64, [_i32, _i32, _i32]),
    "mae_umap_fuzzy_knn": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "mae_umap_epoch": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _f32, _f32, _f32, _i32, _i32, C.c_uint32, _vp]),
    "mae_gather_patches": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mae_assemble_visible": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "mae_visible_grad_split": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mae_build_inverse": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "mae_build_row_map": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "mae_decoder_assemble": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mae_decoder_assemble_bwd": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mae_zero_unpredicted_rows": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mae_mse_loss_from_images": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _i32, _vp, _i32, _vp]),
    "mae_predictor_assemble": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mae_predictor_assemble_bwd": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "mae_build_tail_row_map": (C.c_int, [_i32, _i32, _i32, _vp, _vp]),
    "mae_rows_from_tokens": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "mae_smooth_l1_loss": (C.c_int, [_vp, _vp, _i64, _f32, _vp, _vp, _i32, _vp, _vp]),
    "mae_full_grad_split": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mae_full_grad_split_partial_floats": (_i64, [_i32, _i32, _i32]),
    "mae_zero_token_rows": (C.c_int, [_i64, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mae_features_pool": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _f32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mae_features_tap": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _f32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "mae_cast": (C.c_int, [_vp, _i32, _vp, _i32, _i64, _vp]),
    "mae_add_rows_pos": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "mae_add_into": (C.c_int, [_vp, _vp, _i32, _i64, _vp]),
    "mae_linear_dgrad": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
}

for _name, (_res, _args) in SIGNATURES.items():
    try:
        _fn = getattr(lib, _name)
    except AttributeError as exc:  # pragma: no cover
        raise ImportError(f"libmae_hip.so does not export {_name}; rebuild the extension") from exc
    _fn.restype = _res
    _fn.argtypes = _args

if lib.mae_abi_version() != ABI_VERSION:  # pragma: no cover
    raise ImportError(f"libmae_hip.so ABI {lib.mae_abi_version()} != binding {ABI_VERSION}; rebuild the extension")


# Tensors whose addresses were handed to the library by ptr() stay referenced here until the call has returned (check()
# runs right after it): a temporary created inline in the call expression, e.g. ptr(x.float()), would otherwise be
# freed -- and its block possibly re-issued by the caching allocator for the next argument -- before the launch.
# Holding it until the launch is ENQUEUED is enough: the allocator reuses blocks in stream order.
_alive = threading.local()


def ptr(t, dtype=None) -> C.c_void_p:
    """Device address of a contiguous CUDA tensor (None -> NULL); the tensor is kept alive until the next check()."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise RuntimeError("libmae_hip works on device tensors only (no CPU fallback); move the tensor to cuda")
    if not t.is_contiguous():
        raise RuntimeError("libmae_hip needs contiguous tensors")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    keep = getattr(_alive, "tensors", None)
    if keep is None:
        keep = _alive.tensors = []
    keep.append(t)
    return C.c_void_p(t.data_ptr())


def check(rc: int) -> None:
    """Raise with the library's own message when a call returned non-zero."""
    keep = getattr(_alive, "tensors", None)
    if keep:
        keep.clear()
    if rc != 0:
        msg = lib.mae_last_error()
        raise MaeHipError(msg.decode("utf-8", "replace") if msg else f"libmae_hip error {rc}")
