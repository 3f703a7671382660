"""ctypes binding of libd4hip.so (C-ABI declared in include/d4hip.h).

The shared object is built in-tree by `dreamer4_amd.build.build()` (plain hipcc, no torch
headers).  Loading fails loudly when it is missing: there is no CPU / eager fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libd4hip.so')

D4_MAX_ACTION_TYPES = 8

GEMM_RMS_ROWSCALE, GEMM_SILU, GEMM_SWIGLU, GEMM_TRANS_A, GEMM_TRANS_B, GEMM_ACCUMULATE = 1, 2, 4, 8, 16, 32


class Config(C.Structure):
    _fields_ = [
        ('dim', C.c_int32), ('dim_latent', C.c_int32), ('num_latent_tokens', C.c_int32), ('depth', C.c_int32),
        ('time_block_every', C.c_int32), ('attn_heads', C.c_int32), ('attn_dim_head', C.c_int32),
        ('attn_softclamp_value', C.c_float),
        ('num_spatial_tokens', C.c_int32), ('num_register_tokens', C.c_int32), ('max_steps', C.c_int32),
        ('num_tasks', C.c_int32), ('num_discrete_action_types', C.c_int32),
        ('num_discrete_actions', C.c_int32 * D4_MAX_ACTION_TYPES), ('num_continuous_actions', C.c_int32),
        ('multi_token_pred_len', C.c_int32),
        ('policy_head_mlp_depth', C.c_int32), ('value_head_mlp_depth', C.c_int32),
        ('terminal_mlp_depth', C.c_int32), ('predict_terminals', C.c_int32),
        ('reward_num_bins', C.c_int32), ('value_num_bins', C.c_int32), ('reward_encoder_type', C.c_int32), ('matmul_bf16', C.c_int32), ('head_mlp_recipe', C.c_int32), ('continuous_beta_param', C.c_int32),
        ('pool_heads', C.c_int32), ('pool_dim_head', C.c_int32),
        ('gae_discount_factor', C.c_float), ('gae_lambda', C.c_float), ('ppo_eps_clip', C.c_float),
        ('policy_entropy_weight', C.c_float), ('use_delight_gating', C.c_int32),
        ('delight_temperature', C.c_float), ('pmpo_pos_to_neg_weight', C.c_float),
        ('pmpo_kl_div_loss_weight', C.c_float), ('pmpo_reverse_kl', C.c_int32),
        ('hl_gauss_sigma_to_bin_ratio', C.c_float), ('hl_gauss_eps', C.c_float),
        ('value_min', C.c_float), ('value_max', C.c_float),
        ('mode', C.c_int32), ('patch_size', C.c_int32), ('channels', C.c_int32), ('image_height', C.c_int32), ('image_width', C.c_int32),
        ('decoder_flow_steps', C.c_int32), ('decoder_pos_mlp_depth', C.c_int32),
        ('max_batch', C.c_int32), ('max_frames', C.c_int32), ('max_parallel_frames', C.c_int32),
        ('max_learn_rows', C.c_int32),
        ('wide_frames', C.c_int32),
    ]


class RolloutIO(C.Structure):
    _fields_ = [
        ('batch', C.c_int32), ('time_steps', C.c_int32), ('prompt_frames', C.c_int32), ('num_steps', C.c_int32),
        ('use_time_cache', C.c_int32), ('sample_terminals', C.c_int32), ('sample_actions', C.c_int32),
        ('context_signal_noise', C.c_float), ('discrete_temperature', C.c_float), ('continuous_temperature', C.c_float),
        ('noise_latent', C.c_void_p), ('noise_context', C.c_void_p), ('gumbel_u', C.c_void_p), ('bern_u', C.c_void_p),
        ('beta_noise', C.c_void_p), ('tasks', C.c_void_p),
        ('latents', C.c_void_p), ('actions', C.c_void_p), ('actions_cont', C.c_void_p), ('rewards', C.c_void_p), ('ctx_hist', C.c_void_p),
        ('agent_embed', C.c_void_p), ('log_probs', C.c_void_p), ('log_probs_cont', C.c_void_p), ('cont_params', C.c_void_p),
        ('values', C.c_void_p), ('action_logits', C.c_void_p),
        ('lens', C.c_void_p), ('terminals', C.c_void_p),
    ]


class GemmDesc(C.Structure):
    """d4_gemm_desc: the GemmArgs fields the engine sets (include/d4hip.h)."""
    _fields_ = [
        ('A', C.c_void_p), ('lda', C.c_int32), ('W', C.c_void_p), ('ldw', C.c_int32), ('C', C.c_void_p), ('ldc', C.c_int32),
        ('bias', C.c_void_p), ('R', C.c_void_p), ('ldr', C.c_int32),
        ('M', C.c_int32), ('N', C.c_int32), ('K', C.c_int32), ('flags', C.c_int32), ('rms_eps', C.c_float),
        ('C2', C.c_void_p), ('ldc2', C.c_int32), ('c2_S', C.c_int32), ('c2_lo', C.c_int32), ('c2_hi', C.c_int32), ('c2_last', C.c_int32),
        ('batch', C.c_int32), ('strideA', C.c_int64), ('strideW', C.c_int64), ('strideC', C.c_int64),
        ('Ab', C.c_void_p), ('Wb', C.c_void_p), ('Cb', C.c_void_p), ('C2b', C.c_void_p),
        ('wplane', C.c_int64), ('wscale', C.c_void_p), ('strideWs', C.c_int64), ('aexp', C.c_void_p),
    ]


class AssembleDesc(C.Structure):
    """d4_assemble_desc: the AssembleArgs fields (include/d4hip.h)."""
    _fields_ = [
        ('tokens', C.c_void_p), ('space', C.c_void_p), ('signal_embed', C.c_void_p), ('step_embed', C.c_void_p), ('registers', C.c_void_p),
        ('agent_embed', C.c_void_p), ('task_embed', C.c_void_p), ('action_embed', C.c_void_p), ('action_learned', C.c_void_p),
        ('signal_levels', C.c_void_p), ('signal_uniform', C.c_int32), ('prev_actions', C.c_void_p), ('prev_cont', C.c_void_p),
        ('cont_embed', C.c_void_p), ('tasks', C.c_void_p), ('action_offsets', C.c_void_p),
        ('B', C.c_int32), ('Tq', C.c_int32), ('S', C.c_int32), ('D', C.c_int32), ('ns', C.c_int32), ('nr', C.c_int32), ('na', C.c_int32),
        ('nc', C.c_int32), ('step_log2', C.c_int32), ('compact', C.c_void_p), ('has_agent', C.c_int32),
    ]


class PolicyLossDesc(C.Structure):
    """d4_policy_loss_desc: the learner's PolicyLossArgs (include/d4hip.h)."""
    _fields_ = [
        ('logits', C.c_void_p), ('ld', C.c_int32), ('actions', C.c_void_p), ('old_log_probs', C.c_void_p), ('old_logits', C.c_void_p), ('ldo', C.c_int32),
        ('advantages', C.c_void_p), ('mask', C.c_void_p), ('action_sizes', C.c_void_p), ('rows', C.c_int32), ('na', C.c_int32), ('total', C.c_int32),
        ('cparams', C.c_void_p), ('ldc', C.c_int32), ('actions_cont', C.c_void_p), ('old_log_probs_cont', C.c_void_p), ('old_cparams', C.c_void_p),
        ('nc', C.c_int32), ('beta_param', C.c_int32), ('objective', C.c_int32), ('normalize', C.c_int32), ('use_gate', C.c_int32), ('reverse_kl', C.c_int32),
        ('eps', C.c_float), ('clip', C.c_float), ('ent_w', C.c_float), ('gate_temp', C.c_float), ('pmpo_alpha', C.c_float), ('kl_w', C.c_float),
        ('loss', C.c_void_p), ('dlogits', C.c_void_p), ('dcparams', C.c_void_p), ('row_pl', C.c_void_p), ('row_ent', C.c_void_p), ('row_aux', C.c_void_p),
        ('scratch', C.c_void_p),
    ]


# d4_gemm_run families / d4_gemm_run_pair targets
GEMM_TILE, GEMM_V2, GEMM_V2_KSPLIT, GEMM_X3, GEMM_X3SK, GEMM_H2, GEMM_SKINNY, GEMM_BF16, GEMM_BF16A = range(9)
PAIR_SKINNY, PAIR_BF16A, PAIR_V2 = range(3)

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p)


class LearnIO(C.Structure):
    _fields_ = [
        ('batch', C.c_int32), ('time', C.c_int32), ('objective', C.c_int32), ('normalize_advantages', C.c_int32),
        ('eps', C.c_float), ('use_delight_gating', C.c_int32), ('delight_temperature', C.c_float),
        ('agent_embed', C.c_void_p), ('actions', C.c_void_p), ('old_log_probs', C.c_void_p),
        ('actions_cont', C.c_void_p), ('old_log_probs_cont', C.c_void_p), ('old_cont_params', C.c_void_p), ('old_values', C.c_void_p),
        ('rewards', C.c_void_p), ('old_action_logits', C.c_void_p), ('lens', C.c_void_p), ('is_truncated', C.c_void_p),
        ('terminals', C.c_void_p),
        ('allreduce_sum', ALLREDUCE_FN), ('allreduce_user', C.c_void_p),
        ('losses', C.c_void_p), ('returns', C.c_void_p),
        ('d_agent_embed_policy', C.c_void_p), ('d_agent_embed_value', C.c_void_p),
        ('ema_returns', C.c_void_p), ('reward_ema_decay', C.c_double), ('q_lo', C.c_float), ('q_hi', C.c_float),
        ('clip_values', C.c_int32), ('value_clip', C.c_float),
    ]


class ValueLossDesc(C.Structure):
    """d4_value_loss_desc (include/d4hip.h)."""
    _fields_ = [
        ('logits', C.c_void_p), ('ld', C.c_int32), ('returns', C.c_void_p), ('old_values', C.c_void_p), ('mask', C.c_void_p), ('support', C.c_void_p),
        ('rows', C.c_int32), ('bins', C.c_int32), ('vmin', C.c_float), ('vmax', C.c_float), ('sigma', C.c_float), ('eps', C.c_float),
        ('two_hot', C.c_int32), ('clip_values', C.c_int32), ('value_clip', C.c_float),
        ('loss', C.c_void_p), ('row_loss', C.c_void_p), ('dlogits', C.c_void_p), ('scratch', C.c_void_p),
    ]


# every symbol include/d4hip.h declares: (restype, argtypes)
_P, _I, _F, _L, _D = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.c_double
SYMBOLS = {
    'd4_last_error': (C.c_char_p, []),
    'd4_version': (_I, []),
    'd4_engine_create': (_I, [C.POINTER(Config), C.POINTER(_P)]),
    'd4_engine_destroy': (None, [_P]),
    'd4_engine_workspace_bytes': (C.c_size_t, [_P]),
    'd4_engine_set_workspace': (_I, [_P, _P, C.c_size_t]),
    'd4_engine_bind': (_I, [_P, C.c_char_p, _P, _P, _L]),
    'd4_engine_prepare': (_I, [_P, _P]),
    'd4_engine_cache_frames': (_I, [_P]),
    'd4_engine_cache_reset': (_I, [_P, _I]),
    'd4_engine_cache_export': (_I, [_P, _P, _I, _P]),
    'd4_engine_cache_import': (_I, [_P, _P, _I, _I, _P]),
    'd4_wm_forward': (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    'd4_decoder_forward': (_I, [_P, _P, _P, _I, _I, _I, _P, _P]),
    'd4_ff_workspace_bytes': (C.c_size_t, [_I, _I, _I]),
    'd4_train_arith_set': (_I, [_I]),
    'd4_train_wide_set': (_I, [_I]),
    'd4_train_attn_products_set': (_I, [_I]),
    'd4_train_arith_get': (_I, []),
    'd4_train_scratch_bind': (_I, [_P, C.c_size_t]),
    'd4_ff_bf16_scratch_bytes': (C.c_size_t, [_I] * 3),
    'd4_attn_bf16_scratch_bytes': (C.c_size_t, [_I] * 4),
    'd4_cross_attn_bf16_scratch_bytes': (C.c_size_t, [_I] * 7),
    'd4_ff_forward': (_I, [_P] * 6 + [_I, _I, _I, _P, _P, C.c_size_t, _P]),
    'd4_ff_backward': (_I, [_P] * 6 + [_I, _I, _I] + [_P] * 6 + [_P, C.c_size_t, _P]),
    'd4_ff_backward_saved': (_I, [_P] * 6 + [_I, _I, _I] + [_P] * 6 + [_P, C.c_size_t, _P]),
    'd4_attn_workspace_bytes': (C.c_size_t, [_I] * 5),
    'd4_space_attn_forward': (_I, [_P] * 11 + [_I] * 5 + [_F, _I, _I, _P, _P, C.c_size_t, _P]),
    'd4_space_attn_backward': (_I, [_P] * 12 + [_I] * 5 + [_F, _I, _I] + [_P] * 11 + [_P, C.c_size_t, _P]),
    'd4_space_attn_backward_saved': (_I, [_P] * 12 + [_I] * 5 + [_F, _I, _I] + [_P] * 11 + [_P, C.c_size_t, _P]),
    'd4_time_attn_workspace_bytes': (C.c_size_t, [_I] * 6),
    'd4_time_attn_forward': (_I, [_P] * 12 + [_I] * 6 + [_F, _I, _P, _P, C.c_size_t, _P]),
    'd4_time_attn_backward': (_I, [_P] * 13 + [_I] * 6 + [_F, _I] + [_P] * 11 + [_P, C.c_size_t, _P]),
    'd4_time_attn_backward_saved': (_I, [_P] * 13 + [_I] * 6 + [_F, _I] + [_P] * 11 + [_P, C.c_size_t, _P]),
    'd4_cross_attn_workspace_bytes': (C.c_size_t, [_I] * 7),
    'd4_cross_attn_forward': (_I, [_P] * 10 + [_I] * 8 + [_F, _P, _P, C.c_size_t, _P]),
    'd4_cross_attn_backward': (_I, [_P] * 11 + [_I] * 8 + [_F] + [_P] * 10 + [_P, C.c_size_t, _P]),
    'd4_cross_attn_backward_saved': (_I, [_P] * 11 + [_I] * 8 + [_F] + [_P] * 10 + [_P, C.c_size_t, _P]),
    'd4_encoder_forward': (_I, [_P, _P, _I, _I, _P, _P]),
    'd4_euler_step': (_I, [_P, _P, _L, _F, _F, _P]),
    'd4_rollout': (_I, [_P, C.POINTER(RolloutIO), _P]),
    'd4_learn': (_I, [_P, C.POINTER(LearnIO), _P]),
    'd4_adamw_clip': (_I, [_P, _P, _P, _P, _L, _I, _F, _F, _F, _F, _F, _F, _F, _P, _P]),
    'd4_profile_bf16_enable': (_I, [_I]),
    'd4_profile_bf16_read': (_I, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'd4_profile_enable': (_I, [_I]),
    'd4_profile_read': (_I, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), _I]),
    'd4_profile_classes': (_I, []),
    'd4_gemm_force_config': (_I, [_I]),
    'd4_debug_switch': (_I, [C.c_char_p, _I]),
    'd4_frame_fused_set': (_I, [_I]),
    'd4_profile_class_name': (C.c_char_p, [_I]),
    'd4_profile_glue_enable': (_I, [_I]),
    'd4_profile_glue_read': (_I, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), _I]),
    'd4_profile_glue_classes': (_I, []),
    'd4_profile_glue_read_flops': (_I, [C.POINTER(C.c_double), _I]),
    'd4_measure_peaks': (_I, [_P, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    'd4_profile_glue_class_name': (C.c_char_p, [_I]),
    'd4_debug_buffer': (_I, [_P, C.c_char_p, C.POINTER(_P)]),
    'd4_gemm': (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    'd4_gemm_tn': (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, C.c_int64, _I, _I, _P]),
    'd4_gemm_tn_bf16': (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, C.c_int64, _I, _P]),
    'd4_gemm_pair': (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    'd4_gemm_batched': (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _I, _L, _L, _L, _P]),
    'd4_gemm_bf16': (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    'd4_gemm_bf16a': (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P]),
    'd4_cvt_bf16': (_I, [_P, _P, _L, _P]),
    'd4_gemm_bf16a_compact': (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    'd4_gemm_bf16a_batched': (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _L, _L, _L, _I, _P]),
    'd4_cvt_rows_bf16': (_I, [_P, _L, _P, _L, _I, _I, _P]),
    'd4_split_bf16x3': (_I, [_P, _P, _L, _L, _P]),
    'd4_gemm_split': (_I, [_P, _I, _P, _L, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P]),
    'd4_split_f16x2': (_I, [_P, _P, _I, _I, _I, _L, _P, _P]),
    'd4_row_scale_exp': (_I, [_P, _L, _I, _I, _P, _P]),
    'd4_gemm_split2': (_I, [_P, _I, _P, _L, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P, _P]),
    'd4_rmsnorm': (_I, [_P, _I, _P, _P, _I, _I, _I, _F, _P]),
    'd4_small_attn': (_I, [_P, _L, _L] * 4 + [_P] + [_P, _L, _L] * 3 + [_P] + [_I] * 4 + [_F] + [_I] * 6 + [_P]),
    'd4_small_attn_wide': (_I, [_P, _L, _L] * 4 + [_P] + [_P, _L, _L] * 3 + [_P] + [_I] * 4 + [_F] + [_I] * 6 + [_P]),
    'd4_small_attn_wide_bf16': (_I, [_P, _L, _L] * 4 + [_P] + [_P, _L, _L] * 3 + [_P] + [_I] * 4 + [_F] + [_I] * 6 + [_P]),
    'd4_pool_mix': (_I, [_P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    'd4_pool_mix_deep': (_I, [_P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P, _P]),
    'd4_time_attn_decode': (_I, [_P, _I, _P, _I, _P, _P, _P, _P, _I, _P] + [_I] * 8 + [_P, _F, _I, _I, _P]),
    'd4_gemm_family_configs': (_I, [_I]),
    'd4_gemm_route': (_I, [C.POINTER(GemmDesc), _I]),
    'd4_gemm_run': (_I, [C.POINTER(GemmDesc), _I, _I, _P]),
    'd4_gemm_run_rowmap': (_I, [C.POINTER(GemmDesc), _I, _I, _I, _I, _I, _I, _P]),
    'd4_gemm_run_pair': (_I, [C.POINTER(GemmDesc), C.POINTER(GemmDesc), _I, _I, _P]),
    'd4_gemm_fill_capacity': (_I, [C.POINTER(GemmDesc)]),
    'd4_gemm_run_fill': (_I, [C.POINTER(GemmDesc), C.POINTER(GemmDesc), _I, _P]),
    'd4_gemm_run_fill_rowmap': (_I, [C.POINTER(GemmDesc), C.POINTER(GemmDesc), _I, _I, _I, _I, _I, _P]),
    'd4_tile16_weights': (_I, [_P, _I, _P, _I, _I, _P]),
    'd4_frame_attn_out': (_I, [_P, _L, _L] * 4 + [_P] + [_P, _L, _L] * 2 + [_P] + [_I] * 3 + [_F] + [_I] * 3 + [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P]),
    'd4_attn_out_cols': (_I, [_P, _L, _L] * 4 + [_P] + [_P, _L, _L] * 2 + [_P] + [_I] * 3 + [_F] + [_I] * 3 + [_P, _I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P]),
    'd4_frame_pool': (_I, [_P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _I, _I, _I, _F, _P, _P, _I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P]),
    'd4_frame_pool_tail': (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P]),
    'd4_lqap_in': (_I, [_P, _I, _P, _I, _P, _P, _P, _P] + [_I] * 5 + [_F, _P]),
    'd4_lqap_out': (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _I] + [_I] * 5 + [_P]),
    'd4_debug_last_form': (C.c_char_p, [C.c_char_p]),
    'd4_debug_forms': (_I, [C.c_char_p, _I, C.POINTER(C.c_char_p)]),
    'd4_train_attn_core_plane_floats': (C.c_size_t, [_I] * 3),
    'd4_train_xattn_core_plane_floats': (C.c_size_t, [_I] * 4),
    'd4_train_attn_core': (_I, [_P, _I] + [_P] * 7 + [_I] * 4 + [_F, _I, _I, _I, _L, _L, _I, _P, _I, _P, C.c_size_t, _P]),
    'd4_train_xattn_core': (_I, [_P, _I, _P, _I] + [_P] * 6 + [_I] * 6 + [_F, _I, _P, C.c_size_t, _P]),
    'd4_train_attn_core_bf16_plane_floats': (C.c_size_t, [_I] * 4),
    'd4_train_xattn_core_bf16_plane_floats': (C.c_size_t, [_I] * 5),
    'd4_train_attn_core_bf16': (_I, [_P, _I] + [_P] * 7 + [_I] * 4 + [_F, _I, _I, _I, _L, _L, _I, _P, _I, _P, C.c_size_t, _P]),
    'd4_train_xattn_core_bf16': (_I, [_P, _I, _P, _I] + [_P] * 6 + [_I] * 6 + [_F, _I, _P, C.c_size_t, _P]),
    'd4_rmsnorm_backward': (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _F, _P]),
    'd4_layernorm_rows': (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _F, _I, _P]),
    'd4_assemble_tokens': (_I, [C.POINTER(AssembleDesc), _P]),
    'd4_gather_space_double_norm': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    'd4_colsum': (_I, [_P, _I, _I, _I, _P, _P, C.c_size_t, _P]),
    'd4_colsum_batch': (_I, [_I, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_P), _P]),
    'd4_rmsnorm_bwd': (_I, [_P, _P, _P, _P, _P, _I, _I, _F, _P]),
    'd4_euler_step_rows': (_I, [_P, _I, _P, _I, _I, _I, _F, _F, _P]),
    'd4_splitk_reduce': (_I, [_P, _I, _I, _I, _P, _I, _P, _I, _P]),
    'd4_mean_tokens': (_I, [_P, _P, _I, _I, _I, _P]),
    'd4_hl_gauss_scalar_strided': (_I, [_P, _I, _P, _P, _I, _I, _I, _P]),
    'd4_unary_rows': (_I, [_I, _P, _P, _L, _P]),
    'd4_fold_rows': (_I, [_P, _P, _P, _I, _I, _I, _P]),
    'd4_swiglu_pack_rows': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    'd4_build_latent_input': (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _F, _P]),
    'd4_copy_rows': (_I, [_P, _I, _P, _I, _I, _I, _P]),
    'd4_pad_cols': (_I, [_P, _P, _I, _I, _I, _P]),
    'd4_video_patches': (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    'd4_cache_transfer': (_I, [_P, _P] + [_I] * 9 + [_P]),
    'd4_cunembed': (_I, [_I, _P, _P, _I, _I, _I, _P]),
    'd4_coord_grid': (_I, [_P, _I, _I, _I, _P]),
    'd4_pack_tokens': (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'd4_prep_eval_inputs': (_I, [_P, _P, _P] + [_I] * 7 + [_P, _P, _I, _P]),
    'd4_layernorm_silu_bwd': (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _F, _P]),
    'd4_silu_bwd': (_I, [_P, _P, _P, _L, _P]),
    'd4_swiglu': (_I, [_I, _P, _P, _P, _I, _I, _I, _P]),
    'd4_multi_copy': (_I, [_I, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64), _P]),
    'd4_zero_pad_cols': (_I, [_P, _I, _I, _I, _I, _P]),
    'd4_cvt_pad_bf16': (_I, [_P, _L, _P, _L, _I, _I, _I, _P]),
    'd4_cvt_transpose_bf16': (_I, [_P, _I, _P, _I, _I, _I, _I, _P]),
    'd4_hl_gauss_scalar': (_I, [_P, _I, _P, _P, _I, _I, _P]),
    'd4_ppo_policy_loss': (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P]),
    'd4_gae': (_I, [_P, _P, _P, _P, _P, _F, _F, _I, _I, _P, _P]),
    'd4_gae_adv': (_I, [_P, _P, _P, _P, _P, _F, _F, _I, _I, _P, _P, _P, _P]),
    'd4_policy_loss': (_I, [C.POINTER(PolicyLossDesc), _P]),
    'd4_return_stats': (_I, [_P, _P, _P, _L, _P, C.c_double, _F, _F, _P, _P, _P]),
    'd4_value_loss': (_I, [C.POINTER(ValueLossDesc), _P]),
    'd4_categorical_sample_logp': (_I, [_P, _I, _P, _I, _P, _I, _I, _F, _P, _P, _P]),
    'd4_hl_gauss_ce': (_I, [_P, _I, _P, _P, _P, _I, _I, _F, _F, _F, _F, _I, _P, _P, _P, _P]),
    'd4_flow_noised_patches': (_I, [_P] * 4 + [_I] * 6 + [_P]),
    'd4_tok_rows_part_floats': (C.c_size_t, [_I, _I]),
    'd4_layernorm_rows_bwd': (_I, [_P, _I, _P, _P, _P, _P, _P, C.c_size_t, _I, _I, _F, _P]),
    'd4_mask_rows_fwd': (_I, [_P] * 4 + [_I, _I, _P]),
    'd4_mask_rows_bwd': (_I, [_P] * 5 + [C.c_size_t, _I, _I, _P]),
    'd4_recon_loss_fwd_bwd': (_I, [_P] * 4 + [_I] * 7 + [_P, _P, _P, C.c_size_t, _P]),
    'd4_sigreg_part_floats': (C.c_size_t, [_I] * 4),
    'd4_sigreg_fwd_bwd': (_I, [_P, _P] + [_I] * 4 + [_F, _F, _I, _P, _P, _P, C.c_size_t, _P]),
    'd4_latent_ortho_part_floats': (C.c_size_t, [_I]),
    'd4_latent_ortho_fwd_bwd': (_I, [_P] + [_I] * 3 + [_P, _P, _P, C.c_size_t, _P]),
    'd4_pack_tokens_bf16': (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    'd4_muon_plan_create': (_I, [_I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(_P)]),
    'd4_muon_plan_create_products': (_I, [_I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t, _I, C.POINTER(_P)]),
    'd4_muon_plan_products': (_I, [_P]),
    'd4_muon_plan_destroy': (None, [_P]),
    'd4_muon_plan_workspace_bytes': (C.c_size_t, [_P]),
    'd4_muon_plan_passes': (_I, [_P]),
    'd4_muon_step': (_I, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_F), _P, C.c_size_t, _D, _D, _D, _I, _I, _F, _F, _F, _F, _P, _F, _P]),
    'd4_newton_schulz': (_I, [_P, C.POINTER(_P), C.POINTER(_P), _P, C.c_size_t, _I, _F, _F, _F, _F, _P]),
    'd4_multi_table_bytes': (C.c_size_t, [_I, C.POINTER(_L)]),
    'd4_sumsq_multi': (_I, [_I, C.POINTER(_L), C.POINTER(_P), _P, C.c_size_t, _I, _P, _P]),
    'd4_adam_atan2_multi': (_I, [_I, C.POINTER(_L), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _P, C.c_size_t, _I, _I,
                                 _D, _D, _D, _D, _D, _D, _P, _F, _P]),
}

_lib = None


class D4Error(RuntimeError):
    pass


def load():
    """Load libd4hip.so; raises when it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise D4Error(f'{LIB_PATH} is missing: run `python -m dreamer4_amd.build` (hipcc, gfx950). '
                      'There is no CPU fallback for the imagination path.')
    # tile choices of the benchmark configurations measured on MI355X, shipped with the package: preloaded by the GEMM dispatcher so
    # that those shapes never time anything at first use (reproducible performance, no first-call synchronisation)
    default_table = os.path.join(_HERE, 'gemm_tune_default.txt')
    if os.path.isfile(default_table):
        os.environ.setdefault('D4_GEMM_TUNE_DEFAULT', default_table)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().d4_last_error()
        raise D4Error(f'd4hip error {rc}: {msg.decode() if msg else "?"}')


def ptr(t):
    """Device (or host) pointer of a torch tensor, None -> NULL."""
    if t is None:
        return None
    assert t.is_contiguous(), 'd4hip expects contiguous tensors'
    return C.c_void_p(t.data_ptr())
