/*
 * d4hip — C-ABI of the MI355X-native (gfx950) implementation of dreamer4's imagination hot path.
 *
 * The reference (lucidrains/dreamer4, /root/reference/dreamer4/dreamer4.py = "D4") has no FFI or
 * operator boundary: its API is the Python nn.Module surface.  This header is the boundary a
 * maintainer would bind instead of the ATen op sequences of
 *
 *   DynamicsWorldModel.generate               D4:6308-6774   -> d4_rollout
 *   DynamicsWorldModel.forward (inference)    D4:6792-7295   -> d4_wm_forward
 *   DynamicsWorldModel.learn_from_experience  D4:5893-6305   -> d4_learn (+ d4_optim_step)
 *
 * Conventions
 *   - plain C, no torch types: device pointers + sizes; `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 on success; otherwise a non-zero code and d4_last_error() holds the
 *     message (shape / config / HIP errors).  Nothing is retried or silently replaced by a fallback.
 *   - all tensors are dense fp32 row-major unless stated; integer tensors are int64 (actions, lens,
 *     tasks) to match torch.long on the Python side; booleans are uint8.
 *   - the engine never allocates device memory: the caller owns one workspace buffer
 *     (d4_engine_workspace_bytes) and all weight / IO tensors.  Kernels are enqueued on `stream`
 *     with no host synchronisation, so calls are hipGraph-capturable.
 *   - weights are bound by the reference's state_dict key names (weight interchange = flat
 *     {key: tensor}), see d4_engine_bind.
 */
#ifndef D4HIP_H
#define D4HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D4_MAX_ACTION_TYPES 8
#define D4_MODE_DYNAMICS 0
#define D4_MODE_DECODER 1
#define D4_MODE_ENCODER 2
#define D4_MLP_PRE_RMS 0        /* RMSNorm -> Linear -> SiLU                        (x_mlps_pytorch create_mlp: recipe unpinned) */
#define D4_MLP_POST_LAYER 1     /* Linear -> LayerNorm -> SiLU, bare last Linear */
/* Link of the Beta policy head's raw outputs (discrete_continuous_embed_readout BetaDist, unimodal=True at D4:1172-1173: alpha, beta >= 1).
 * The package is absent from the image, so the link is a descriptor like the MLP recipe (csrc/beta.h). */
#define D4_BETA_SOFTPLUS_P1 0   /* alpha = softplus(raw0) + 1, beta = softplus(raw1) + 1 */
#define D4_BETA_EXP_P1 1        /* alpha = exp(raw0) + 1,      beta = exp(raw1) + 1 */

/* Constructor arguments of DynamicsWorldModel (supported subset; names as D4:4662-4778). */
typedef struct d4_config {
    int32_t dim, dim_latent, num_latent_tokens, depth, time_block_every;
    int32_t attn_heads, attn_dim_head;          /* attn_dim_head: 16, 32 or 64 (a head row lives in one wavefront) */
    float attn_softclamp_value;
    int32_t num_spatial_tokens, num_register_tokens, max_steps, num_tasks;
    int32_t num_discrete_action_types;
    int32_t num_discrete_actions[D4_MAX_ACTION_TYPES];
    int32_t num_continuous_actions;             /* Beta policy head: continuous_dist_type='beta', no norm stats (D4:1131, 1172-1196) */
    int32_t multi_token_pred_len;
    int32_t policy_head_mlp_depth, value_head_mlp_depth, terminal_mlp_depth, predict_terminals;
    int32_t reward_num_bins, value_num_bins;
    int32_t reward_encoder_type;                /* 0 = hl_gauss (default, D4:1041), 1 = symexp_two_hot (D4:947): bins = symexp(linspace), two-hot targets */
    int32_t matmul_bf16;                        /* trunk GEMM arithmetic.  0: fp32 on the f32-input MFMA; 2: fp32 on the bf16 matrix cores by operand
                                                   splitting (three bf16 planes per operand, six products, fp32 accumulate: fp32 accuracy,
                                                   csrc/gemm_x3.hip) — the Python mirror's default; 1: bf16 MFMA (bf16-rounded weights +
                                                   activations, fp32 accumulate, fp32 norms / softmax / residual stream); 3: opt-in fp32-class mode on
                                                   the fp16 matrix cores (two fp16 planes per operand under exact row scales, three products:
                                                   csrc/gemm_h2.hip, see d4_gemm_split2).  Decoder / encoder mode: 0 or 1 (the trunk's Linears; the
                                                   four end projections stay fp32), 2 and 3 are refused */
    int32_t head_mlp_recipe;                    /* D4_MLP_PRE_RMS / D4_MLP_POST_LAYER: layer recipe of the policy / value / terminal MLPs (engine.h) */
    int32_t continuous_beta_param;              /* D4_BETA_SOFTPLUS_P1 / D4_BETA_EXP_P1: link of the Beta head's raw parameters (csrc/beta.h) */
    int32_t pool_heads, pool_dim_head;          /* AttentionPool defaults 4 x 64 (D4:2147-2148) */
    /* learn_from_experience hyper-parameters (D4:4731-4744) */
    float gae_discount_factor, gae_lambda, ppo_eps_clip, policy_entropy_weight;
    int32_t use_delight_gating;
    float delight_temperature, pmpo_pos_to_neg_weight, pmpo_kl_div_loss_weight;
    int32_t pmpo_reverse_kl;
    float hl_gauss_sigma_to_bin_ratio, hl_gauss_eps, value_min, value_max;
    /* mode D4_MODE_DECODER / D4_MODE_ENCODER: the engine is the video tokenizer's decoder (VideoDecoderNetwork, D4:3490-3682) or its
     * encoder (encoder_transformer, D4:3912-3933) instead of the dynamics model — the same trunk kernels over [patches | latent tokens] per frame; constructor arguments of VideoTokenizer (D4:3686-3764). */
    int32_t mode;
    int32_t patch_size, channels, image_height, image_width, decoder_flow_steps, decoder_pos_mlp_depth;
    /* capacities the workspace is sized for */
    int32_t max_batch;            /* trajectories per call */
    int32_t max_frames;           /* KV-cache capacity in frames (prompt + generated) */
    int32_t max_parallel_frames;  /* frames evaluated in one parallel pass (1 = cached decode only) */
    int32_t max_learn_rows;       /* batch * time rows of one learn_from_experience call (0 = no learner) */
    /* Wide frames: 0 (a zero-initialised struct) the engine takes at most 64 latent / spatial tokens and 64 tokens per frame
     * (decoder / encoder mode: 160), as ever; != 0 each may reach 1024 in every mode, and an attention with more than 64 items on a side runs
     * the tiled matrix-pipe core of csrc/attn_wide_mfma.hip (at <= 64 the same kernels and the same bits as with 0).
     * A bit set: bit 0 (value 1) is the above; bit 1 on top of it (value 3) runs those attentions on the bf16-product form of
     * the core (csrc/attn_wide_bf16.hip), with any matmul_dtype.  2 (bit 1 alone) and values above 3 are refused by d4_engine_create. */
    int32_t wide_frames;
} d4_config;

typedef struct d4_engine d4_engine;

const char* d4_last_error(void);
int d4_version(void);

int d4_engine_create(const d4_config* cfg, d4_engine** out);
void d4_engine_destroy(d4_engine* e);

/* Bytes of device workspace the engine needs (prepared weights + activations + KV cache). */
size_t d4_engine_workspace_bytes(const d4_engine* e);
int d4_engine_set_workspace(d4_engine* e, void* device_ptr, size_t bytes);

/* Bind one parameter/buffer by its reference state_dict key, e.g.
 * "transformer.layers.3.2.fn.to_q.weight" (layout list: DESIGN.md "Weight interchange").
 * `grad` may be NULL; when given, d4_learn writes d(loss)/d(param) there (policy / value heads).
 * Pseudo-keys for buffers the reference builds in its constructor:
 *   "reward_encoder.centers" [reward_num_bins], "value_encoder.centers" [value_num_bins],
 *   "value_encoder.support" [value_num_bins + 1]   (hl_gauss);
 *   symexp_two_hot reads the reference's own buffers "reward_encoder.bin_values" / "value_encoder.bin_values" [num_bins]. */
int d4_engine_bind(d4_engine* e, const char* key, const float* device_ptr, float* grad, int64_t numel);

/* Build the fused / gamma-folded weight images in the workspace.  Call after binding, and again
 * whenever a trunk weight changes (head MLP weights are read in place and need no re-prepare). */
int d4_engine_prepare(d4_engine* e, void* stream);

/* Number of frames currently held by the time KV cache (token_count of D4:3261). */
int d4_engine_cache_frames(const d4_engine* e);
int d4_engine_cache_reset(d4_engine* e, int frames);   /* set the frame counter: 0 = empty, < current = truncate; moving it forward
                                                          again is valid while the slots in between have not been rewritten */
/* Export / import the cache in the reference layout (time_layers, 2, B*S, heads, t, 64)  D4:2075, 3256. */
int d4_engine_cache_export(d4_engine* e, float* dst, int batch, void* stream);
int d4_engine_cache_import(d4_engine* e, const float* src, int batch, int frames, void* stream);

/* DynamicsWorldModel.forward(latents=..., signal_levels=..., step_sizes=..., discrete_actions=...,
 * time_cache=..., latent_is_noised=True, return_pred_only=True, return_intermediates=True)
 * D4:6792-7295.  Evaluates `frames` new frames per trajectory (row order b, t):
 *   latents        [batch][frames][n][dl]
 *   signal_levels  [batch][frames] int32 in [0, max_steps)
 *   prev_actions   [batch][frames][action_types] int64: the action token of each frame, i.e. the
 *                  action taken at the previous frame; a negative first entry means "no action"
 *                  (zero token, D4:7110-7126).  NULL = zero tokens everywhere (models with discrete actions).
 *   prev_cont      [batch][frames][num_continuous_actions] float, same pairing; "no action" = NaN in the first
 *                  entry (only consulted when the model has no discrete actions).  NULL allowed as above.
 *   tasks          [batch] int64 or NULL
 *   use_cache      attend over the frames already in the KV cache (their count is the rotary offset)
 *   commit_cache   keep the new frames' K/V in the cache (the "extra clean step" of D4:6545)
 * Outputs: pred [batch][frames][n][dl], agent_embed [batch][frames][dim]. */
int d4_wm_forward(d4_engine* e, const float* latents, const int32_t* signal_levels, int step_size,
                  const int64_t* prev_actions, const float* prev_cont, const int64_t* tasks, int batch, int frames,
                  int use_cache, int commit_cache, float* pred, float* agent_embed, void* stream);

/* VideoTokenizer.decode_step (D4:4137-4184) on an engine created with mode = D4_MODE_DECODER: one evaluation of the decoder.
 *   latents       [batch][frames][n][dl]
 *   noised_video  [batch][channels][frames][H][W]   the flow sample being denoised (pure noise on the first step, D4:4212)
 *   time_index    flow step i in [0, decoder_flow_steps)   (time_embed row, D4:4155)
 * Output: pred_video [batch][channels][frames][H][W] (the predicted clean video).  VideoTokenizer.decode's Euler update between
 * steps (D4:4226-4230) is d4_euler_step. */
int d4_decoder_forward(d4_engine* e, const float* latents, const float* noised_video, int time_index, int batch, int frames,
                       float* pred_video, void* stream);
/* VideoTokenizer.tokenize (D4:4107-4113 -> forward(return_latents=True) in eval mode, D4:4239-4433) on an engine created with
 * mode = D4_MODE_ENCODER (depth = encoder_depth): video [batch][channels][frames][H][W] -> latents [batch][frames][n][dl] in (-1, 1). */
int d4_encoder_forward(d4_engine* e, const float* video, int batch, int frames, float* latents, void* stream);
/* x += (pred - x) / one_minus_t * dt, elementwise over n floats: the flow-matching Euler step of generate (D4:6567-6580) and of
 * VideoTokenizer.decode (D4:4226-4230). */
int d4_euler_step(float* x, const float* pred, int64_t n, float one_minus_t, float dt, void* stream);

/* DynamicsWorldModel.generate(...) D4:6308-6774 with every random draw injected. */
typedef struct d4_rollout_io {
    int32_t batch;
    int32_t time_steps;            /* total frames incl. prompt (while latents.shape[1] < time_steps) */
    int32_t prompt_frames;         /* frames already present in `latents` (teacher forcing, D4:6392) */
    int32_t num_steps;             /* denoising steps K (power of two) */
    int32_t use_time_cache;        /* D4:6321 */
    int32_t sample_terminals;      /* return_terminals && predict_terminals (D4:6454) */
    int32_t sample_actions;        /* return_agent_actions (D4:6625): policy head + Gumbel sample + value head */
    float context_signal_noise;    /* D4:6319 */
    float discrete_temperature;
    float continuous_temperature;
    /* injected noise, one slice per generated frame f = 0 .. time_steps - prompt_frames - 1 */
    const float* noise_latent;     /* [F][batch][n][dl] normal   (D4:6475) */
    const float* noise_context;    /* [F][batch][n][dl] normal   (D4:6670); may be NULL when use_time_cache */
    const float* gumbel_u;         /* [F][batch][A] uniform (0,1) (MultiCategorical.sample) */
    const float* bern_u;           /* [F][batch] uniform         (D4:6611); NULL unless sample_terminals */
    const float* beta_noise;       /* [F][batch][nc][2][6][2] (normal, uniform) per gamma rejection round (Readout.sample_continuous) */
    const int64_t* tasks;          /* [batch] or NULL */
    /* in/out histories, time-major stride = time_steps; prompt entries pre-filled by the caller */
    float* latents;                /* [batch][time_steps][n][dl]  (unclamped; caller clamps, D4:6686) */
    int64_t* actions;              /* [batch][time_steps][action_types] */
    float* actions_cont;           /* [batch][time_steps][nc] continuous actions in the Beta's native (0, 1) range */
    float* rewards;                /* [batch][time_steps] */
    float* ctx_hist;               /* [batch][time_steps][n][dl] fixed context noise per frame (prompt entries =
                                      the prompt latents, D4:6400); NULL allowed when use_time_cache */
    /* outputs for generated frames only, index = frame - prompt_frames, stride = F */
    float* agent_embed;            /* [batch][F][dim] */
    float* log_probs;              /* [batch][F][action_types] */
    float* log_probs_cont;         /* [batch][F][nc] */
    float* cont_params;            /* [batch][F][nc][2] raw Beta parameters (old_action_unembeds.continuous, D4:6749-6750) */
    float* values;                 /* [batch][F]; written, like `rewards`, once after the last frame (nothing inside the rollout reads them) */
    float* action_logits;          /* [batch][F][A]   (old_action_unembeds, D4:6749-6750) */
    int64_t* lens;                 /* [batch]  pre-filled with time_steps */
    uint8_t* terminals;            /* [batch]  pre-filled with 0 */
} d4_rollout_io;

int d4_rollout(d4_engine* e, const d4_rollout_io* io, void* stream);

/* DynamicsWorldModel.learn_from_experience(experience, only_learn_policy_value_heads=True,
 * objective=...) D4:5893-6305 with stored agent embeds: losses AND gradients of the policy head
 * (policy MLP + discrete_action_unembed) and the value head into the `grad` buffers given at bind. */
typedef struct d4_learn_io {
    int32_t batch, time;
    int32_t objective;             /* 0 = ppo, 1 = spo, 2 = pmpo */
    int32_t normalize_advantages;  /* -1 = default (objective != pmpo) */
    float eps;                     /* z-score epsilon (1e-6, D4:5903) */
    int32_t use_delight_gating;    /* -1 = engine config default */
    float delight_temperature;     /* <= 0 = engine config default */
    const float* agent_embed;      /* [batch][time][dim] */
    const int64_t* actions;        /* [batch][time][action_types] */
    const float* old_log_probs;    /* [batch][time][action_types] */
    const float* actions_cont;     /* [batch][time][nc] */
    const float* old_log_probs_cont;   /* [batch][time][nc] */
    const float* old_cont_params;  /* [batch][time][nc][2] (pmpo KL) or NULL */
    const float* old_values;       /* [batch][time] */
    const float* rewards;          /* [batch][time] */
    const float* old_action_logits;/* [batch][time][A] (pmpo KL) or NULL */
    const int64_t* lens;           /* [batch] */
    const uint8_t* is_truncated;   /* [batch] */
    const uint8_t* terminals;      /* [batch] */
    /* global-batch statistics for data parallel runs: host callback that sum-reduces `n` floats in
     * place across ranks (NULL = single process).  Called on the host between kernel phases. */
    int (*allreduce_sum)(float* device_buf, int n, void* user);
    void* allreduce_user;
    float* losses;                 /* device [2]: total_policy_loss, value_loss */
    float* returns;                /* optional device [batch][time] */
    /* optional device [batch][time][dim] each: d total_policy_loss / d agent_embed and d value_loss / d agent_embed, for
     * learn_from_experience(only_learn_policy_value_heads=False) (D4:6045-6075): the caller backpropagates them through the world model
     * that produced agent_embed (dreamer4_amd/trunk_ops.py).  NULL (the default path): not computed. */
    float* d_agent_embed_policy;
    float* d_agent_embed_value;
    /* ---- appended; all zero = off, the launches and bits of before ----
     * keep_reward_ema_stats (D4:5985-6015): device [2] = ema_returns_mean, ema_returns_var, updated in place on the stream (no host
     * synchronisation); NULL = off.  The masked returns are clamped to their q_lo / q_hi quantiles (torch.quantile, linear), their mean and
     * biased variance go into the pair by lerp with weight 1 - reward_ema_decay, and the advantage becomes
     * (returns - mean) / std - (old_values - mean) / std with std = sqrt(max(var, 1e-5)).  No learnable step: the pair is left as it is.
     * Single process only: refused together with allreduce_sum. */
    float* ema_returns;
    double reward_ema_decay;
    float q_lo, q_hi;
    /* clip_values (D4:6283-6291): value loss = max(CE(values), -sum p log max(encode(old + clamp(values - old, +-value_clip)), 1e-20)) per row */
    int32_t clip_values;
    float value_clip;
} d4_learn_io;

int d4_learn(d4_engine* e, const d4_learn_io* io, void* stream);

/* clip_grad_norm_(params, max_norm) followed by one torch.optim.AdamW step on a flat parameter group,
 * as DreamTrainer does per head (trainers.py:1436-1452).  `grad_scale` multiplies the gradient first
 * (1/world_size after a SUM all-reduce of per-rank-mean gradients; 1 with global statistics).
 * exp_avg / exp_avg_sq: caller-owned optimiser state (zero-initialised); scratch: >= 1025 floats;
 * scratch[0] receives the (scaled) total gradient norm. */
int d4_adamw_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                  float lr, float beta1, float beta2, float eps, float weight_decay, float max_grad_norm,
                  float grad_scale, float* scratch, void* stream);

/* Measurement hook (bench.py roofline leg): `mask` bit c (c < 27) enables tile configuration c of the GEMM kernels; every
 * (mask >> 27)-th launch (0 -> every launch) of an enabled configuration carries a HIP event pair on its dispatch (launch stream); d4_profile_read sums elapsed ms / algorithmic flops /
 * launches per configuration and clears the log.  d4_profile_classes() configurations exist; d4_profile_class_name(c) is the
 * prefix of the kernel name rocprofv3 reports for configuration c ("gemm_kernel<BM, BN, WGM, WGN, BK, 1"). */
/* bf16 path: every `stride`-th bf16 GEMM launch carries an event pair (0 = off); read sums ms / flops / launches and clears. */
int d4_profile_bf16_enable(int stride);
int d4_profile_bf16_read(double* ms, double* flops, int64_t* count);
int d4_profile_enable(int mask);
int d4_profile_read(double* ms, double* flops, int64_t* count, int nclass);
int d4_profile_classes(void);
const char* d4_profile_class_name(int c);
/* The same for the non-GEMM kernel classes of the rollout (within-frame / time attention, KV append, attention-pool mix, the small
 * attention forms, token assembly, split-K reduce): d4_profile_glue_read sums elapsed ms / ALGORITHMIC HBM bytes / launches per class.
 * Mask and stride as d4_profile_enable.  (bench.py's HBM roofline leg; replaces nothing in the reference.) */
int d4_profile_glue_enable(int mask);
int d4_profile_glue_read(double* ms, double* bytes, int64_t* count, int nclass);
int d4_profile_glue_classes(void);
int d4_profile_glue_read_flops(double* flops, int nclass);      /* matrix work the per-frame fused classes carry; call before d4_profile_glue_read */
const char* d4_profile_glue_class_name(int c);

/* Measured denominators for the roofline fractions (nothing of the reference is replaced: it has no measurement layer): what THIS device
 * sustains on a float4 stream copy through `scratch` (two halves; >= 1 GiB so that the 256 MB Infinity Cache cannot serve it; read + write GB/s) and on
 * bare v_mfma_f32_16x16x4_f32 / v_mfma_f32_32x32x16_bf16 streams with random operands (TFLOP/s).  Well under a second; synchronises the stream. */
int d4_measure_peaks(void* scratch, size_t scratch_bytes, double* hbm_copy_gbs, double* mfma_f32_tflops, double* mfma_bf16_tflops, void* stream);

/* Test hook: run GEMM tile configuration `id` wherever it is valid instead of the tuned / static choice (-1 restores it);
 * 100 + c: configuration c of the second fp32 family (gemm2.hip); 200 + c: configuration c of the bf16 kernel; 300 + c: tile c of the
 * split-operand fp32 family (gemm_x3.hip); 400 + c: tile c of the fp16x2 family (gemm_h2.hip); 500 + c: tile c of the bf16-activation kernel (gemm_bf16a.hip).
 * 199: the few-row / long-K form of the second family (gemm2_ksplit_kernel) on every call it can run (normally taken by a rule on the shape).
 * ONE family is forced at a time: every call first clears the hooks of the other families (so forcing, say, 400 + c also switches off the special forms
 * that only run un-forced: the persistent split-operand kernel, the pair launches).  Returns the number of configurations of the family addressed
 * (id = -1: of the first family).  Every configuration of a family must produce the same bits (tests/test_gpu_kernels.py). */
/* Test hook for the per-frame fused block tails (csrc/frame_fused.hip; default 1): 0 separate kernels, 1 fused, 2 fused tails with the
 * pool mix as its own kernel.  Returns the previous mode.  Which path runs is otherwise a rule on the call's shape. */
int d4_frame_fused_set(int mode);
/* Test hook for the two bit-identical launch fusions of the cached decode (each is asserted bitwise against its two-launch form): name =
 * "time_attn_fused_append" (KV append inside the time attention, csrc/attn.hip) or "attn_out_cols" (attention inside the column-split output
 * projection at <= 4 frames, csrc/frame_fused.hip); value 1 (default) fused, 0 two launches.  Returns the previous value, -1 for an unknown name.
 * "pool_wide_keys" (bf16 engine only; NOT bit-identical: the queries become bf16): 1 (default) a hidden is projected once, when produced, onto the key
 * weights of every later attention pool and the query weights of the pool it feeds; 0 a query launch + a key launch over the whole stack per pool.
 * Read when a frame is ENQUEUED: a captured hipGraph keeps the form it was captured with.
 * "time_attn_tiled" (training time attention, csrc/attn_tiled.hip; NOT bit-identical: another summation order): 0 (default) the tiled core
 * runs above 64 frames only, 1 at any length, so that it can be checked at shapes the LDS core also handles.  Read by
 * d4_time_attn_workspace_bytes too: size the workspace with the value the calls will run under.
 * "space_attn_tiled" / "cross_attn_tiled" (training space / cross attention; NOT bit-identical either): 0 (default) the tiled core runs above
 * 64 items per side with d4_train_wide_set(1) only, 1 at any size.  Read by d4_attn_workspace_bytes / d4_cross_attn_workspace_bytes too.
 * "small_attn_wide" (inference attention, csrc/attn_wide_mfma.hip; NOT bit-identical: another summation order): 0 (default) a call with the wide
 * option (d4_small_attn_wide, d4_config.wide_frames) takes the wide core above 64 items on a side only, 1 at any size (with the bf16-product
 * option, d4_small_attn_wide_bf16 / wide_frames 3: that form of the core).  Read when a frame is enqueued, like "pool_wide_keys".
 * "pool_mix_deep" (engine attention pools, csrc/pool_mix_deep.hip; NOT bit-identical: another summation order): 0 (default) a pool takes the
 * chunked mix above 64 hiddens only (d4_config.wide_frames, depth >= 32), 1 every pool of the mix path does, as its own kernel in front of the
 * fused tail where that applies.  Read when a frame is enqueued.
 * "rollout_clean_agent_row" (d4_rollout; bit-identical): 1 (default) the clean evaluation of a frame — the one that feeds the heads; its latent
 * prediction is never read — skips to_latent_pred and, on the fp32 engines with 4 pool heads and dim <= 1024, runs its final stage on the agent
 * row alone; 0 it computes the prediction as d4_wm_forward does.  Part of the key of a captured frame graph.
 * "rollout_batched_heads" (d4_rollout): 1 (default) the value and reward heads run once after the frame loop over all batch * F agent rows
 * (values / rewards: fp32 rounding apart from the per-frame path at F > 1, bit-identical with the same launches at F == 1; everything else
 * bit-identical); 0 after every frame.
 * "layer0_const_rows" / "pool_const_keys" (fp32 dynamics engine): 1 (default) the register rows of a frame, which are a parameter, keep their share
 * of layer 0's fused projection / of the in-loop pools' keys of slab 0 from d4_engine_prepare, and an evaluation projects the other rows only
 * (bit-identical); 0 the full launches.
 * "launch_count" (not a switch): returns the number of kernel launches the library has enqueued since the counter was last set, and sets it to
 * `value` (launches inside a replayed hipGraph are not seen). */
int d4_debug_switch(const char* name, int value);
int d4_gemm_force_config(int id);

/* Test hook: device address of an engine-internal activation buffer (names: engine.hip d4_debug_buffer). */
int d4_debug_buffer(d4_engine* e, const char* name, float** ptr);

/* ---- single-kernel entry points (parity tests call the same launchers the engine uses) ---- */
int d4_gemm(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias,
            const float* R, int ldr, int M, int N, int K, int flags, float rms_eps, void* stream);
/* Two independent Linear layers of equal in-features (the AttentionPool's query and key projections, dreamer4.py:2143-2160) in ONE
 * launch: C1 = f(A1 W1^T), C2 = f(A2 W2^T), W row-major [N][K] (ldw = K), `flags` as d4_gemm (row scale only).  Bit-identical to two
 * d4_gemm calls; falls back to them when the grouped form does not apply. */
int d4_gemm_pair(const float* A1, int lda1, const float* W1, float* C1, int ldc1, int M1, int N1, const float* A2, int lda2, const float* W2, float* C2,
                 int ldc2, int M2, int N2, int K, int flags, float rms_eps, void* stream);
/* Gradient of a Linear's weight (backward of dreamer4.py:2079-2116, 1968-2075): C[M][N] = A^T B, A [K][lda] (the output gradient, M columns),
 * B [K][ldb] (the layer input, N columns), both row-major with the contraction over their ROWS.  M, N, lda, ldb, ldc multiples of 4, 16-byte
 * aligned operands.  `part` (part_floats floats, or NULL) holds the partial products when the rows are split into slices; tile_n / slices = 0
 * take the shape rule (csrc/gemm_tn.hip), other values force the 64 x (64 tile_n) tile and the slice count (benchmarks).  Deterministic. */
int d4_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, float* part, int64_t part_floats,
               int tile_n, int slices, void* stream);
/* The same product on the bf16 matrix pipe (the weight gradient of the bf16 training arithmetic, csrc/gemm_tn_bf16.hip): A [K][lda] and B [K][ldb]
 * are bf16 images (round to nearest even) of the output gradient and the layer input, C [M][N] fp32 with fp32 accumulation.  lda, ldb multiples
 * of 8 that cover M, N rounded up to 8; 16-byte aligned images; any M, N, K >= 1 (ragged edges are zero-padded inside the kernel, C outside
 * M x N is not touched).  `part` as for d4_gemm_tn; slices = 0 takes the shape rule.  Deterministic. */
int d4_gemm_tn_bf16(const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc, int M, int N, int K, float* part, int64_t part_floats,
                    int slices, void* stream);
/* strided-batch form (the AttentionPool's per-head value projection, D4:2143-2177): problem b reads A + b*strideA,
 * W + b*strideW and writes C (and R) + b*strideC   (strides in elements). */
int d4_gemm_batched(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias,
                    const float* R, int ldr, int M, int N, int K, int flags, float rms_eps, int batch,
                    int64_t strideA, int64_t strideW, int64_t strideC, void* stream);
/* the bf16 MFMA kernel alone: A fp32 [M][lda] (rounded to bf16 on the way in), Wb bf16 [N][ldw] (raw 16-bit patterns), C fp32 */
int d4_gemm_bf16(const float* A, int lda, const uint16_t* Wb, int ldw, float* C, int ldc, const float* bias,
                 const float* R, int ldr, int M, int N, int K, int flags, float rms_eps, void* stream);
/* The same Linear with the activations already in bf16 (the producer's bf16 copy): Ab bf16 [M][lda], Wb bf16 [N][ldw], C fp32 [M][ldc], Cb (optional)
 * = bf16(C) at the same leading dimension for the next layer.  K % 64 == 0, lda / ldw % 8 == 0.  LDS-DMA ring kernel (csrc/gemm_bf16a.hip); `config`
 * = -1: tile by the shape rule, else one of its configurations.  d4_cvt_bf16: fp32 -> bf16 (round to nearest even), n elements. */
int d4_gemm_bf16a(const uint16_t* Ab, int lda, const uint16_t* Wb, int ldw, float* C, int ldc, uint16_t* Cb, const float* bias, const float* R, int ldr,
                  int M, int N, int K, int flags, float rms_eps, int config, void* stream);
int d4_cvt_bf16(const float* src, uint16_t* dst, int64_t n, void* stream);
/* The producer -> consumer hand-off of the bf16 engine (the reference keeps one activation tensor per nn.Linear input, dreamer4.py:1983-2068,
 * 2105-2116, 2143-2177; here a bf16 IMAGE of it is what the next Linear reads): C may be NULL when only the bf16 image Cb is wanted; `batch` > 1 runs
 * `batch` independent products A + b * strideA, Wb + b * strideW -> C / Cb + b * strideC (the attention pool's per-head value projection).
 * d4_cvt_rows_bf16: rows x cols of a strided fp32 matrix -> bf16 (round to nearest even), the pass behind producers that cannot write the image. */
/* ... with the engine's second, ROW-COMPACTED copy of the output (the rows the final attention pool and the latent head read: token rows s = m % c2_S with
 * c2_lo <= s < c2_hi, plus the last token of a frame when c2_last; fp32 `C2` and optionally its bf16 image `C2b`, [frames * (c2_hi - c2_lo + c2_last)][ldc2]).
 * It replaces the reference's indexing of the layer hiddens at D4:3242-3246 / 7251 (the trunk keeps every token row; only these are consumed). */
int d4_gemm_bf16a_compact(const uint16_t* Ab, int lda, const uint16_t* Wb, int ldw, float* C, int ldc, uint16_t* Cb, const float* bias, const float* R, int ldr,
                          int M, int N, int K, int flags, float rms_eps, float* C2, uint16_t* C2b, int ldc2, int c2_S, int c2_lo, int c2_hi, int c2_last,
                          int config, void* stream);
int d4_gemm_bf16a_batched(const uint16_t* Ab, int lda, const uint16_t* Wb, int ldw, float* C, int ldc, uint16_t* Cb, const float* bias, const float* R, int ldr,
                          int M, int N, int K, int flags, float rms_eps, int batch, int64_t strideA, int64_t strideW, int64_t strideC, int config, void* stream);
int d4_cvt_rows_bf16(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int rows, int cols, void* stream);
/* fp32 GEMM on the bf16 matrix cores (csrc/gemm_x3.hip; the trunk's default `Linear` arithmetic): every fp32 operand is the exact sum of three
 * bf16 numbers and a product is accumulated from its six leading bf16 x bf16 terms in fp32 — fp32 accuracy (error against float64 no
 * larger than the f32-input MFMA kernels'), 6/16 of their matrix-pipe time.  d4_split_bf16x3 writes the three planes of W
 * (dst[p * plane_stride + i], p = 0..2; plane_stride % 8 == 0); d4_gemm_split takes A in fp32 and splits it on the fly.  `config` = -1: the
 * dispatcher's choice, 0..5 one tile configuration of the family (all give the same bits), 6 the persistent form the engine uses (csrc/gemm_x3sk.hip:
 * one workgroup per CU, a last partial round of at most half the workgroups as 128 x 64 half tiles — the same bits). */
int d4_split_bf16x3(const float* src, uint16_t* dst, int64_t n, int64_t plane_stride, void* stream);
int d4_gemm_split(const float* A, int lda, const uint16_t* W3, int64_t plane_stride, int ldw, float* C, int ldc, const float* bias,
                  const float* R, int ldr, int M, int N, int K, int flags, float rms_eps, int config, void* stream);
/* fp32-class GEMM on the fp16 matrix cores (csrc/gemm_h2.hip; round 5; the engine's OPT-IN `matmul_bf16 = 3` arithmetic for every nn.Linear of
 * D4:1983-2068, 2105-2116, 2143-2210): each operand row is scaled by an exact power of two into fp16's range and written as two fp16 planes
 * (hi, lo 2^11: a 23-bit image of the operand), a product is accumulated from its three leading fp16 x fp16 terms in fp32 and the scales are undone
 * by one exponent shift.  Against float64 its error on dot products of >= 16 terms is BELOW the f32-input MFMA kernels' (0.45x at K = 512) at
 * x1.2-2.0 their speed, but a single product carries a relative error of up to 2^-21 where fp32 has 2^-24: on operands spanning 2^120 inside a
 * row (every output one product) it reads 5.5e-7 of sum |a w| against the f32-input MFMA's 3.1e-7 — which is why it is NOT the default fp32 path
 * (profiles/r05_x3_products.txt).  d4_split_f16x2 writes the two planes of a weight matrix W [rows][ld] (dst[p * plane_stride + r * ld + c], p = 0..1;
 * ld % 8 == 0, plane_stride % 8 == 0) and inv_scale[r] = the power of two that undoes row r's scale; d4_row_scale_exp the scale exponents of an
 * activation matrix's rows (once for every GEMM that reads it); d4_gemm_split2 takes A in fp32 and splits it on the fly (a_exp null: the kernel
 * finds the exponents itself, a pass over A per column tile).  `config` = -1: the family's static choice, 0..6 one tile (all give the same bits). */
int d4_split_f16x2(const float* src, uint16_t* dst, int rows, int cols, int ld, int64_t plane_stride, float* inv_scale, void* stream);
int d4_row_scale_exp(const float* A, int64_t lda, int rows, int K, int32_t* exp_out, void* stream);
int d4_gemm_split2(const float* A, int lda, const uint16_t* W2, int64_t plane_stride, int ldw, const float* w_inv_scale, float* C, int ldc, const float* bias,
                   const float* R, int ldr, int M, int N, int K, int flags, float rms_eps, int config, const int32_t* a_exp, void* stream);
/* ---- trunk backward, first slice (SURVEY.md 8f-3 groundwork; not on the imagination path) ----
 * FeedForward block (dreamer4.py:2079-2116) on the reference parameter layout: y = proj_out(a * silu(g)) with [a | g] = proj_in(RMSNorm(x));
 * x / y / dy / dx [rows][dim], norm_w [dim], w_in [2*inner][dim], b_in [2*inner], w_out [dim][inner], b_out [dim].  The backward
 * recomputes the forward intermediates (nothing is saved between the two calls).  workspace: 256-byte aligned device memory.
 * Every `*_backward_saved` entry (FeedForward and the three attention blocks below) takes the SAME arguments as its `*_backward` but requires
 * `workspace` to be the very buffer the matching `*_forward` call ran in, untouched since: the forward intermediates it holds (normalised input,
 * concatenated weight images, projections) are used as they are and nothing is recomputed (one GEMM in four of a block's backward). */
size_t d4_ff_workspace_bytes(int rows, int dim, int inner);
/* Training arithmetic of the four blocks (FeedForward, space / time / cross attention): 0 = fp32 (default), 1 = bf16.
 * bf16: the forward, input-gradient and weight-gradient products of every Linear with at least 16 input and 16 output features run on bf16
 * images of their operands (fp32 accumulate, fp32 results); norms, attention cores, SiLU-GLU, the heads-wide gate / mix projections, biases
 * and every gradient output stay fp32.
 *
 * d4_train_arith_set is process-wide and returns the previous value: a caller sets it immediately before EACH forward / backward call of a
 * block (a `*_backward_saved` call must run in the arithmetic of its forward) and restores it after.
 *
 * Scratch: in bf16 mode a block call needs memory for the bf16 operand images.  d4_train_scratch_bind(scratch, bytes) binds 256-byte aligned
 * device memory of at least the block's `*_bf16_scratch_bytes` to the CALLING thread (NULL unbinds).  Nothing in it outlives the call, so it
 * can be freed (stream-ordered) right after.  d4_attn_bf16_scratch_bytes serves the space and the time block (rows = all token rows of the
 * call).  The blocks' workspaces and their size queries are the same in both arithmetics.
 *
 * NOT thread-safe across concurrent training threads: two host threads that drive blocks in different arithmetics at the same time can see
 * each other's setting.  Both mismatches are refused, neither computes silently in the wrong arithmetic: a call that finds the switch at bf16
 * without a scratch bound on its thread fails, and so does a call that finds the switch at fp32 while its thread has a scratch bound.  One
 * training loop per process, with autograd's single backward thread, is the supported use. */
int d4_train_arith_set(int arith);
int d4_train_arith_get(void);
/* Wide frames: 0 (default) the space and cross attention blocks take at most 64 items per group and side, as ever; 1 they take
 * up to 1024, and above 64 items on a side run the tiled core of csrc/attn_tiled.hip (at <= 64 the same kernels and the same bits as with 0).
 * d4_attn_workspace_bytes / d4_cross_attn_workspace_bytes answer for the CURRENT setting (larger above 64 items with 1, unchanged otherwise),
 * so a caller sets the switch around the size query and around EACH forward / backward call alike (a `*_backward_saved` call must meet the
 * setting of its forward) and restores it after.  Process-wide like d4_train_arith_set; returns the previous value.  The inference engine is
 * not concerned: its own option is d4_config.wide_frames (up to 1024 tokens per frame; more than 64 pooled hiddens stay refused). */
int d4_train_wide_set(int on);
/* Products of the tiled attention core of the training path: 0 (default) fp32, all six on the f32-input MFMA as ever; 1 bf16:
 * every block launch that takes the tiled core (the time layers above 64 frames, space / cross attention under the d4_train_wide_set(1) rule,
 * any of the three under its d4_debug_switch hook) runs the core's bf16-product form (csrc/attn_tiled_bf16.hip: bf16-rounded q, k', v, dO, P
 * and dS on the bf16 MFMA, fp32 accumulate, everything else fp32).  The whole-problem-in-LDS kernels at <= 64 items are not concerned.  The
 * three workspace size queries answer for the CURRENT setting (the bf16 images follow the unchanged carve-up wherever the tiled core runs), so
 * a caller sets the switch around the size query and EACH forward / backward call alike, like d4_train_wide_set.  Process-wide; returns the
 * previous value; any other value returns -1, changes nothing and is named in d4_last_error.
 * What follows the switch: d4_time_attn_*, d4_space_attn_*, d4_cross_attn_* (forward, backward, backward_saved) and their three workspace size
 * queries.  What does not: the operator entries below.  d4_train_attn_core / d4_train_xattn_core run the LDS kernel (core 0) or the fp32 tiled
 * core (core 1) on planes of d4_train_*_core_plane_floats floats whatever the switch says, and d4_train_attn_core_bf16 /
 * d4_train_xattn_core_bf16 always run the bf16 form. */
int d4_train_attn_products_set(int products);
int d4_train_scratch_bind(void* scratch, size_t bytes);
size_t d4_ff_bf16_scratch_bytes(int rows, int dim, int inner);
size_t d4_attn_bf16_scratch_bytes(int rows, int dim, int heads, int dim_head);
size_t d4_cross_attn_bf16_scratch_bytes(int groups, int nq, int nk, int dim, int dim_ctx, int heads, int dim_head);
int d4_ff_forward(const float* x, const float* norm_w, const float* w_in, const float* b_in, const float* w_out, const float* b_out,
                  int rows, int dim, int inner, float* y, float* workspace, size_t workspace_bytes, void* stream);
int d4_ff_backward(const float* x, const float* dy, const float* norm_w, const float* w_in, const float* b_in, const float* w_out,
                   int rows, int dim, int inner, float* dx, float* d_norm_w, float* d_w_in, float* d_b_in, float* d_w_out, float* d_b_out,
                   float* workspace, size_t workspace_bytes, void* stream);
int d4_ff_backward_saved(const float* x, const float* dy, const float* norm_w, const float* w_in, const float* b_in, const float* w_out,
                   int rows, int dim, int inner, float* dx, float* d_norm_w, float* d_w_in, float* d_b_in, float* d_w_out, float* d_b_out,
                   float* workspace, size_t workspace_bytes, void* stream);
/* Space attention block (Attention.forward, dreamer4.py:1968-2075, self attention within a frame): x / y [frames*tokens][dim],
 * residual_values [frames*tokens][heads*dim_head] or null (then w_mix / b_mix and their gradients are unused), wq / wk / wv
 * [heads*dim_head][dim], wo [dim][heads*dim_head], w_gates / w_mix [heads][dim], b_mix [heads], k_gamma [heads][dim_head];
 * tokens <= 64 per frame (<= 1024 with d4_train_wide_set(1)), dim_head 16 / 32 / 64; num_special trailing tokens are hidden from the ordinary queries (dreamer4.py:1769-1783). */
size_t d4_attn_workspace_bytes(int frames, int tokens, int dim, int heads, int dim_head);
int d4_space_attn_forward(const float* x, const float* residual_values, const float* norm_w, const float* wq, const float* wk, const float* wv,
                          const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma,
                          int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int num_special, int belief,
                          float* y, float* workspace, size_t workspace_bytes, void* stream);
int d4_space_attn_backward(const float* x, const float* residual_values, const float* dy, const float* norm_w, const float* wq, const float* wk,
                           const float* wv, const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma,
                           int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int num_special, int belief,
                           float* dx, float* d_residual_values, float* d_norm_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                           float* d_w_gates, float* d_w_mix, float* d_b_mix, float* d_k_gamma,
                           float* workspace, size_t workspace_bytes, void* stream);
int d4_space_attn_backward_saved(const float* x, const float* residual_values, const float* dy, const float* norm_w, const float* wq, const float* wk,
                           const float* wv, const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma,
                           int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int num_special, int belief,
                           float* dx, float* d_residual_values, float* d_norm_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                           float* d_w_gates, float* d_w_mix, float* d_b_mix, float* d_k_gamma,
                           float* workspace, size_t workspace_bytes, void* stream);
/* Time attention block (the same Attention with rotary positions and a causal mask along time, one problem per token column,
 * dreamer4.py:3176-3215 / 1626-1659): x / y [batch][frames][tokens][dim] row-major, frames <= 1024 (no KV cache: the training form);
 * inv_freq [dim_head / 2] = time_rotary.inv_freq.  Up to 64 frames the core keeps a whole (trajectory column, head) problem in LDS; above,
 * a tiled core (csrc/attn_tiled.hip: online softmax forward, P recomputed from the saved log-sum-exp in the backward, all products on the
 * f32-input MFMA) runs over per-row planes that d4_time_attn_workspace_bytes adds behind the block's workspace: memory linear in the
 * frames, nothing of size frames x frames.  More than 1024 frames is an error. */
size_t d4_time_attn_workspace_bytes(int batch, int frames, int tokens, int dim, int heads, int dim_head);
int d4_time_attn_forward(const float* x, const float* residual_values, const float* norm_w, const float* wq, const float* wk, const float* wv,
                         const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma, const float* inv_freq,
                         int batch, int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int belief,
                         float* y, float* workspace, size_t workspace_bytes, void* stream);
int d4_time_attn_backward(const float* x, const float* residual_values, const float* dy, const float* norm_w, const float* wq, const float* wk,
                          const float* wv, const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma,
                          const float* inv_freq, int batch, int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int belief,
                          float* dx, float* d_residual_values, float* d_norm_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                          float* d_w_gates, float* d_w_mix, float* d_b_mix, float* d_k_gamma,
                          float* workspace, size_t workspace_bytes, void* stream);
int d4_time_attn_backward_saved(const float* x, const float* residual_values, const float* dy, const float* norm_w, const float* wq, const float* wk,
                          const float* wv, const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma,
                          const float* inv_freq, int batch, int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int belief,
                          float* dx, float* d_residual_values, float* d_norm_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                          float* d_w_gates, float* d_w_mix, float* d_b_mix, float* d_k_gamma,
                          float* workspace, size_t workspace_bytes, void* stream);
/* Cross-attention block (Attention.forward with a context: the AttentionPool over the layer hiddens dreamer4.py:2143-2177, the final
 * special-token cross attention :3227-3234, the learned-query pools :2179-2210): q_tokens [groups*nq][dim], ctx [groups*nk][dim_ctx] with key
 * j of group g at row g*nk + j, or at row j*groups + g when ctx_item_major (the stack of hiddens); norm_ctx_w may be null (context not
 * normalised); wk / wv [heads*dim_head][dim_ctx]; nq, nk <= 64 (<= 1024 with d4_train_wide_set(1)).  No value residual and no belief projection (as the reference with a context). */
size_t d4_cross_attn_workspace_bytes(int groups, int nq, int nk, int dim, int dim_ctx, int heads, int dim_head);
int d4_cross_attn_forward(const float* q_tokens, const float* ctx, const float* norm_w, const float* norm_ctx_w, const float* wq, const float* wk,
                          const float* wv, const float* wo, const float* w_gates, const float* k_gamma, int groups, int nq, int nk, int ctx_item_major,
                          int dim, int dim_ctx, int heads, int dim_head, float softclamp, float* y, float* workspace, size_t workspace_bytes, void* stream);
int d4_cross_attn_backward(const float* q_tokens, const float* ctx, const float* dy, const float* norm_w, const float* norm_ctx_w, const float* wq,
                           const float* wk, const float* wv, const float* wo, const float* w_gates, const float* k_gamma, int groups, int nq, int nk,
                           int ctx_item_major, int dim, int dim_ctx, int heads, int dim_head, float softclamp,
                           float* d_q_tokens, float* d_ctx, float* d_norm_w, float* d_norm_ctx_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                           float* d_w_gates, float* d_k_gamma, float* workspace, size_t workspace_bytes, void* stream);
int d4_cross_attn_backward_saved(const float* q_tokens, const float* ctx, const float* dy, const float* norm_w, const float* norm_ctx_w, const float* wq,
                           const float* wk, const float* wv, const float* wo, const float* w_gates, const float* k_gamma, int groups, int nq, int nk,
                           int ctx_item_major, int dim, int dim_ctx, int heads, int dim_head, float softclamp,
                           float* d_q_tokens, float* d_ctx, float* d_norm_w, float* d_norm_ctx_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                           float* d_w_gates, float* d_k_gamma, float* workspace, size_t workspace_bytes, void* stream);
int d4_rmsnorm(const float* x, int ldx, const float* gamma, float* y, int ldy, int rows, int dim,
               float eps, void* stream);
/* backward of nn.RMSNorm (autograd of y = x / rms(x) * gamma): dx [rows][dim], d_gamma [dim]; scratch = rows * dim floats. */
/* Operator-level entry points of the inference attention cores (test / tooling use; the engine calls the same launchers).  Arguments are the
 * fields of the launchers' argument structs (csrc/kernels.h: SmallAttnArgs, PoolMixArgs, TimeAttnArgs); strides and leading dimensions in floats.
 *   d4_small_attn        attention of `groups` x `heads` units, nq queries over nk keys: value-residual mix, key norm, softclamp, special-token mask,
 *                        belief projection, head gates; (q_lo, q_hi, q_last) restricts the query set (self attention over 8..16 tokens only).
 *   d4_pool_mix          AttentionPool core: per-head softmax over L hiddens -> gated mix of the normalised hiddens, u [M][heads][D].
 *   d4_time_attn_decode  time attention over the KV cache [2][cache_batch * cache_S][H][Tcap][dh]; mode 0: append + attend (the engine's call),
 *                        1: append only, 2: attend only.  t0_dev (device int, may be null) overrides t0 on the device. */
int d4_small_attn(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                  const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                  const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                  int64_t m_item_stride, float* out, int64_t o_group_stride, int64_t o_item_stride, uint16_t* out_b, int groups, int heads, int nq, int nk,
                  float softclamp, int mask_special, int belief, int q_lo, int q_hi, int q_last, int dh, void* stream);
/* d4_small_attn with the wide option (SmallAttnArgs::wide = 1, what an engine with d4_config.wide_frames passes): more than 64 queries or keys
 * run wide_attn_kernel<dh> (csrc/attn_wide_mfma.hip: up to 1024 per side, dh 16 / 32 / 64, 16-byte aligned q / k / v / output
 * rows, no query restriction, belief with nq == nk only); at <= 64 per side the forms of d4_small_attn, bit for bit.  Forms are recorded under
 * the family "wide_attn". */
int d4_small_attn_wide(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                  const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                  const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                  int64_t m_item_stride, float* out, int64_t o_group_stride, int64_t o_item_stride, uint16_t* out_b, int groups, int heads, int nq, int nk,
                  float softclamp, int mask_special, int belief, int q_lo, int q_hi, int q_last, int dh, void* stream);
/* d4_small_attn_wide with both products on the bf16 matrix pipe (SmallAttnArgs::wide = 2, what an engine with d4_config.wide_frames = 3 passes):
 * more than 64 queries or keys run wide_attn_bf16_kernel<dh> (csrc/attn_wide_bf16.hip) — k' and v' computed in fp32 and rounded to
 * bf16, q and the per-tile p = exp(s - running max) rounded to bf16, fp32 accumulation, softmax, row sum, belief projection and head gate in
 * fp32.  The limits and refusals of d4_small_attn_wide, with its messages; at <= 64 per side the forms of d4_small_attn, bit for bit.  Forms are
 * recorded under the family "wide_attn_bf16". */
int d4_small_attn_wide_bf16(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                  const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                  const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                  int64_t m_item_stride, float* out, int64_t o_group_stride, int64_t o_item_stride, uint16_t* out_b, int groups, int heads, int nq, int nk,
                  float softclamp, int mask_special, int belief, int q_lo, int q_hi, int q_last, int dh, void* stream);
int d4_pool_mix(const float* q, int ldq, const float* x, int ldx, const float* gate_w, const float* k, int ldk, const float* hid, int D,
                const float* k_gamma, float* u, int M, int L, int heads, float eps, uint16_t* u_b, const uint16_t* k_b, const uint16_t* q_b,
                const uint16_t* hid_b, void* stream);
/* d4_pool_mix over 1 <= L <= 1024 hiddens (csrc/pool_mix_deep.hip; what an engine with d4_config.wide_frames runs for its pools of more than 64
 * hiddens): same arguments, same arithmetic, the hiddens walked in chunks of 64 with an online-softmax carry (another summation order than
 * d4_pool_mix at L <= 64, same values).  D % 4 == 0, D <= 1024, heads == 4; anything else is refused before any launch.  Forms are recorded
 * under the family "pool_mix_deep". */
int d4_pool_mix_deep(const float* q, int ldq, const float* x, int ldx, const float* gate_w, const float* k, int ldk, const float* hid, int D,
                     const float* k_gamma, float* u, int M, int L, int heads, float eps, uint16_t* u_b, const uint16_t* k_b, const uint16_t* q_b,
                     const uint16_t* hid_b, void* stream);
int d4_time_attn_decode(const float* proj, int ldp, const float* vres, int ldv, const float* k_gamma, const float* inv_freq, float* cache, float* out,
                        int ldo, uint16_t* out_b, int B, int S, int H, int Tq, int t0, int Tcap, int cache_batch, int cache_S, const int* t0_dev,
                        float softclamp, int dh, int mode, void* stream);
/* Which kernel form the launchers of a family ("small_attn", "pool_mix", "time_kv_append", "time_attn", "wide_attn", "train_attn", "train_xattn",
 * "pool_mix_deep", "wide_attn_bf16") picked at their last call (NULL: unknown
 * family or no call yet), and the family's full list: d4_debug_forms returns the number of forms (-1: unknown family), *name = form i or NULL. */
const char* d4_debug_last_form(const char* family);
int d4_debug_forms(const char* family, int i, const char** name);

/* Operator-level entry points of the attention cores of the training path (test / tooling use; the blocks above call the same cores).  Arguments are
 * the fields of the cores' argument blocks (csrc/attn_tiled.h: AttnBwdArgs, XAttnArgs; hp4 = heads rounded up to 4); core 0 is the
 * whole-problem-in-LDS kernel (<= 64 items per side), core 1 the tiled core (<= 1024) on `planes` of at least the *_plane_floats floats (16-byte
 * aligned; rows = groups * items, q_rows = groups * nq, k_rows = groups * nk).  d_o3 null: forward only, o3 alone is written.  With d_o3 the
 * self core writes the q / k / v, gate and mix columns of dproj (mix: +0 without rv), d_rv (with rv) and dgamma_part [groups][heads * dim_head]; the cross
 * core the q and gate columns of dprojq, the k / v columns of dprojk, and dgamma_part.  Nothing else is written.  Forms are recorded under the
 * families "train_attn" and "train_xattn" (by the block calls too).  These two entries do not follow d4_train_attn_products_set: core 1 is
 * always the fp32 form, on planes of the size below. */
size_t d4_train_attn_core_plane_floats(int rows, int heads, int dim_head);
size_t d4_train_xattn_core_plane_floats(int q_rows, int k_rows, int heads, int dim_head);
int d4_train_attn_core(const float* proj, int ldp, const float* rv, const float* gamma, const float* d_o3,
                       float* o3, float* dproj, float* d_rv, float* dgamma_part,
                       int groups, int items, int heads, int dim_head, float softclamp, int num_special, int belief,
                       int g_inner, int64_t g_outer_stride, int64_t item_stride, int causal, const float* inv_freq,
                       int core, float* planes, size_t plane_floats, void* stream);
int d4_train_xattn_core(const float* projq, int ldq, const float* projk, int ldk, const float* gamma, const float* d_o3,
                        float* o3, float* dprojq, float* dprojk, float* dgamma_part,
                        int groups, int nq, int nk, int heads, int dim_head, int item_major, float softclamp,
                        int core, float* planes, size_t plane_floats, void* stream);
/* The same two cores in the bf16-product form of the tiled core (csrc/attn_tiled_bf16.hip), whatever d4_train_attn_products_set says: the
 * parameter lists, outputs, refusals and texts above, but `core` must be 1 (the whole-problem-in-LDS kernels have no bf16 form) and `planes`
 * holds the bf16 images too: their transposed copies are padded to 32 items per problem, so the size depends on the items per problem and not
 * on the rows alone.  Forms are recorded under the families "train_attn_bf16" and "train_xattn_bf16" (by the block calls too). */
size_t d4_train_attn_core_bf16_plane_floats(int groups, int items, int heads, int dim_head);
size_t d4_train_xattn_core_bf16_plane_floats(int groups, int nq, int nk, int heads, int dim_head);
int d4_train_attn_core_bf16(const float* proj, int ldp, const float* rv, const float* gamma, const float* d_o3,
                            float* o3, float* dproj, float* d_rv, float* dgamma_part,
                            int groups, int items, int heads, int dim_head, float softclamp, int num_special, int belief,
                            int g_inner, int64_t g_outer_stride, int64_t item_stride, int causal, const float* inv_freq,
                            int core, float* planes, size_t plane_floats, void* stream);
int d4_train_xattn_core_bf16(const float* projq, int ldq, const float* projk, int ldk, const float* gamma, const float* d_o3,
                             float* o3, float* dprojq, float* dprojk, float* dgamma_part,
                             int groups, int nq, int nk, int heads, int dim_head, int item_major, float softclamp,
                             int core, float* planes, size_t plane_floats, void* stream);

/* Operator-level entry points of the launches only the engine reaches otherwise (test / tooling use): one GEMM family and configuration chosen by
 * the caller, the pair launches, and the per-frame fused block tails of csrc/frame_fused.hip.  Each fills the launcher's argument struct
 * (csrc/kernels.h: GemmArgs, SmallAttnArgs, PoolMixArgs) and calls the launcher the engine calls; no kernel has a test-only branch.
 * d4_gemm_desc carries every GemmArgs field the engine sets (see csrc/kernels.h for their meaning; strides and leading dimensions in elements). */
typedef struct d4_gemm_desc {
    const float* A; int32_t lda;
    const float* W; int32_t ldw;
    float* C; int32_t ldc;
    const float* bias;
    const float* R; int32_t ldr;
    int32_t M, N, K, flags;
    float rms_eps;
    float* C2; int32_t ldc2, c2_S, c2_lo, c2_hi, c2_last;
    int32_t batch; int64_t strideA, strideW, strideC;
    const uint16_t* Ab; const uint16_t* Wb; uint16_t* Cb; uint16_t* C2b;
    int64_t wplane; const float* wscale; int64_t strideWs; const int32_t* aexp;
} d4_gemm_desc;
#define D4_GEMM_TILE 0          /* first fp32 family (csrc/gemm.hip) through the dispatcher under d4_gemm_force_config(config) */
#define D4_GEMM_V2 1            /* gemm2_launch(config) */
#define D4_GEMM_V2_KSPLIT 2     /* gemm2_ksplit_launch (config ignored) */
#define D4_GEMM_X3 3            /* gemm_x3_launch(config) */
#define D4_GEMM_X3SK 4          /* gemm_x3sk_launch (config ignored) */
#define D4_GEMM_H2 5            /* gemm_h2_launch(config) */
#define D4_GEMM_SKINNY 6        /* gemm_skinny (config ignored) */
#define D4_GEMM_BF16 7          /* gemm_bf16 under its force hook (config) */
#define D4_GEMM_BF16A 8         /* gemm_bf16a_launch(config); configuration 6 is the phased kernel of csrc/gemm_bf16p.hip */
#define D4_GEMM_FAMILIES 9
/* Number of configurations of a family (1 for the single-form targets, -1 for an unknown family). */
int d4_gemm_family_configs(int family);
/* The family the dispatcher (d4::gemm) would run `d` on, under the current d4_gemm_force_config hook and with GemmArgs::rule_M = rule_M (0: the call's own
 * row count); -1 with d4_last_error set for a call the dispatcher rejects.  Host logic only: nothing is launched and no GPU is needed. */
int d4_gemm_route(const d4_gemm_desc* d, int rule_M);
/* Runs `d` on exactly the family / configuration named.  A call the family's `*_applicable` / `*_config_valid` refuses fails with an error that
 * starts "d4_gemm_run: call not supported" and names the reason; nothing falls through to another family. */
int d4_gemm_run(const d4_gemm_desc* d, int family, int config, void* stream);
/* The same with an output row map (csrc/kernels.h: GemmArgs::rm_*): A holds frames of rm_Sc dense rows, C frames of rm_S = rm_Sc + rm_nr rows; dense row r
 * goes to row (r / rm_Sc) * rm_S + (r % rm_Sc) + ((r % rm_Sc) >= rm_lo ? rm_nr : 0) and the gap rows are not written.  D4_GEMM_X3SK and D4_GEMM_V2 (single
 * and batched) implement it for the plain epilogue (bias, row scale); every other family, and any other epilogue, fails with an error. */
int d4_gemm_run_rowmap(const d4_gemm_desc* d, int family, int config, int rm_Sc, int rm_S, int rm_lo, int rm_nr, void* stream);
/* The filled form of the persistent split-operand kernel (csrc/gemm_x3sk.hip: gemm_x3sk_fill_launch).  `main` (a D4_GEMM_X3SK call of at least one whole
 * round of 128 x 128 tiles, no row map) is walked in whole tiles, and the first `fill_tiles` 128 x 64 tiles of `fill` — an independent f32-input product of
 * the LDS-DMA family: no batch, row map, second output or epilogue other than row scale / bias; tiles in that family's block order — run on the workgroups
 * main's last partial round leaves idle.  d4_gemm_fill_capacity: how many those are on the current device (0: not persistent, or no partial round).  More
 * tiles than the capacity or than the fill problem has, an unsupported fill, or a main call the plain launcher refuses fail with an error.  Both outputs
 * carry the bits of the two plain launches.  d4_gemm_run_fill_rowmap puts an output row map (as d4_gemm_run_rowmap) on the fill, which is refused. */
int d4_gemm_fill_capacity(const d4_gemm_desc* main_call);
int d4_gemm_run_fill(const d4_gemm_desc* main_call, const d4_gemm_desc* fill, int fill_tiles, void* stream);
int d4_gemm_run_fill_rowmap(const d4_gemm_desc* main_call, const d4_gemm_desc* fill, int fill_tiles, int rm_Sc, int rm_S, int rm_lo, int rm_nr, void* stream);
#define D4_PAIR_SKINNY 0        /* gemm_skinny_pair */
#define D4_PAIR_BF16A 1         /* gemm_bf16a_pair_launch */
#define D4_PAIR_V2 2            /* gemm2_pair_launch(config) */
/* Two descriptors in ONE launch of the pair form named; refusals as d4_gemm_run ("d4_gemm_run_pair: call not supported"). */
int d4_gemm_run_pair(const d4_gemm_desc* a, const d4_gemm_desc* b, int target, int config, void* stream);
/* The per-frame fused tails.  d4_tile16_weights: W [N][ldw] -> Wt [N / 16][K / 4][16][4], the weight image the frame kernels stream.
 * d4_frame_attn_out / d4_attn_out_cols: within-frame self attention of `frames` frames of S tokens (8 heads x 64; arguments as d4_small_attn)
 * -> output projection to D columns (wo_t: the tiled image of Wo [D][512]; W: Wo itself, row-major at ldw) + resid, written to out [frames * S][ldo]
 * and, when c2 is given, the rows c2_lo <= s < c2_hi (+ the last token when c2_last) of every frame to c2 [frames * (c2_hi - c2_lo + c2_last)][ldc2].
 * d4_frame_pool: AttentionPool mix (arguments as d4_pool_mix, M = frames * S rows) -> per-head value projection (wv_t: tiled [4 * 64][D]) -> output
 * projection (wo_t: tiled [D][4 * 64]) + resid; d4_frame_pool_tail the same from the mixes u [frames * S][heads][D] of d4_pool_mix. */
int d4_tile16_weights(const float* W, int ldw, float* Wt, int N, int K, void* stream);
int d4_frame_attn_out(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                      const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                      const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                      int64_t m_item_stride, uint16_t* out_b, int frames, int heads, int S, float softclamp, int mask_special, int belief, int dh,
                      const float* wo_t, int D, const float* resid, int ldr, float* out, int ldo, float* c2, int ldc2, int c2_lo, int c2_hi, int c2_last,
                      void* stream);
int d4_attn_out_cols(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                     const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                     const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                     int64_t m_item_stride, uint16_t* out_b, int frames, int heads, int S, float softclamp, int mask_special, int belief, int dh,
                     const float* W, int ldw, int D, const float* resid, int ldr, float* out, int ldo, float* c2, int ldc2, int c2_lo, int c2_hi, int c2_last,
                     void* stream);
int d4_frame_pool(const float* q, int ldq, const float* x, int ldx, const float* gate_w, const float* k, int ldk, const float* hid, int D,
                  const float* k_gamma, int M, int L, int heads, float eps, const float* wv_t, const float* wo_t, int frames, int S, const float* resid,
                  int ldr, float* out, int ldo, float* c2, int ldc2, int c2_lo, int c2_hi, int c2_last, void* stream);
int d4_frame_pool_tail(const float* u, const float* wv_t, const float* wo_t, int frames, int S, int D, int pool_heads, const float* resid, int ldr,
                       float* out, int ldo, float* c2, int ldc2, int c2_lo, int c2_hi, int c2_last, void* stream);
/* The latent-token ends of a dynamics evaluation as one per-frame kernel each (csrc/latent_ends.hip; 8 heads x 64, n <= 32, ns <= 16, dl <= 256).
 * d4_lqap_in: latents [frames * n][ldl] -> K | V = rms-scaled latents x w_kv [2 * 512][ldw]^T (dl % 32 == 0) -> attention of the ns learned queries
 * q [ns][512] with head gates gate [ns][8] -> out [frames * ns][512]: the bits of d4_gemm(GEMM_RMS_ROWSCALE) on the LDS-DMA family, then d4_small_attn.
 * d4_lqap_out: attention of the n learned queries q [n][512] (gate [n][8]) over the ns rows kv [frames * ns][ldkv] (K | V) of each frame ->
 * pred [frames * n][ldp] = pooled x w_out [dl][ldw]^T: the bits of d4_small_attn, then d4_gemm on the LDS-DMA family. */
int d4_lqap_in(const float* latents, int ldl, const float* w_kv, int ldw, const float* q, const float* gate, const float* k_gamma, float* out, int frames,
               int heads, int n, int ns, int dl, float eps, void* stream);
int d4_lqap_out(const float* kv, int ldkv, const float* q, const float* gate, const float* k_gamma, const float* w_out, int ldw, float* pred, int ldp,
                int frames, int heads, int n, int ns, int dl, void* stream);

int d4_rmsnorm_backward(const float* x, const float* dy, const float* gamma, float* dx, float* d_gamma, float* scratch, int rows, int dim, float eps,
                        void* stream);
/* Operator-level entry points of the norm, gather, reduction and token-assembly launchers (test / tooling use).  Each fills the
 * launcher's arguments (csrc/kernels.h) and calls the launcher the engine, the learner and the blocks call; no kernel has a test-only branch.
 * Leading dimensions in floats.
 *   d4_layernorm_rows            y = LayerNorm(x) * g + b (b may be null; biased variance), then SiLU when `silu`; dim <= 4096.
 *   d4_assemble_tokens           the token rows of `B * Tq` frames from the embedding tables; d4_assemble_desc mirrors AssembleArgs field by field.
 *   d4_gather_space_double_norm  rows first .. first + ns of every frame of S tokens: RMSNorm(g0) then RMSNorm(g1), out [frames * ns][dim].
 *   d4_colsum                    out[c] = sum_r x[r][c]; scratch (may be null) of at least 16 * cols floats lets rows >= 8192 take the chunked form.
 *   d4_colsum_batch              1 .. 4 column sums in one launch, each in the order of d4_colsum without scratch.
 *   d4_rmsnorm_bwd               tg [rows][dim] = dxhat * x * rstd and, unless dx is null, dx [rows][dim].
 *   d4_euler_step_rows           d4_euler_step on B rows of n_el elements at leading dimensions ldx / ldp.
 *   d4_splitk_reduce             y [M][ldy] = act(sum_s part[s][M][N] + bias) (bias may be null; SiLU when `silu`), the slices added in order.
 *   d4_mean_tokens               out [B][d] = mean over the n tokens of x [B][n][d], added in token order.
 *   d4_hl_gauss_scalar_strided   d4_hl_gauss_scalar with row r written to out[r * out_stride].
 *   d4_unary_rows                y[i] = SiLU(x[i]) (op 0) or tanh(x[i]) (op 1), n elements.
 *   d4_copy_rows, d4_pad_cols, d4_video_patches (to_patches 1: 'b c t (h p1) (w p2) -> (b t h w) (p1 p2 c)', 0: its inverse), d4_cache_transfer (engine
 *                                cache [Lt][2][cache_batch * S][H][Tcap][dh] <-> [Lt][2][B * S][H][frames][dh]; to_ext 1 reads the cache), d4_cunembed (op 0:
 *                                prediction head 0 of U [nc][mtp][d][2] as rows [2 nc][d]; op 1: the gradient scattered back, other heads zero),
 *                                d4_coord_grid (out [nh * nw][ld]: the two linspace(-1, 1) coordinates, remaining columns zero), d4_pack_tokens (which 0: the
 *                                decoder's rows pos + img | the first n_lat of n_total latent rows, patch rows also to `compact`; which 1: the encoder's rows
 *                                img | latent tokens, latent rows also to `compact`): the index permutations and copies, arguments as the launchers'.
 *   d4_fold_rows                 out [rows][ld_out] = W [rows][K] * gamma [K] (gamma may be null: a copy).
 *   d4_swiglu_pack_rows          proj_in [2 inner][K] (value rows, then gate rows) and its bias -> [2 inner_pad][K] in groups of 32 value rows and their 32 gate
 *                                rows, gamma folded, zero rows and zero bias entries for the padding; inner_pad % 32 == 0.
 *   d4_build_latent_input        out [B][Tq][n_el]: frames t < Tq - 1 lerp(hist, ctx_noise, w) read at a frame stride of hist_t_stride (ctx_noise may be
 *                                null: hist itself), the last frame x [B][n_el].
 *   d4_prep_eval_inputs          per frame i = b * Tq + t: sig[i] = sig_val at the last frame of a batch, ctx_sig elsewhere; pact [B * Tq][na] / pcont [B * Tq][nc]
 *                                = the history row (b, frame_base + t - 1) of actions_hist / cont_hist [B][hist_stride][.], -1 / NaN at global frame 0 or
 *                                without a history (either may be null).
 *   d4_layernorm_silu_bwd        backward of a = SiLU(LayerNorm(z) * g + b) on z [rows][ldz], da [rows][dim]: tg = dy * zhat, tb = dy ([rows][dim]) and
 *                                dz [rows][ldz].
 *   d4_silu_bwd                  dz[i] = dy[i] * SiLU'(z[i]), n elements.
 *   d4_swiglu                    h [rows][2 inner_pad] (value half | gate half).  bwd 0: out [rows][inner_pad] = value * SiLU(gate); bwd 1: out
 *                                [rows][2 inner_pad] = the gradient of h given du [rows][inner_pad].  Columns inner .. inner_pad are written as zero.
 *   d4_multi_copy                up to 10 contiguous copies of n[i] floats in one launch (src[i] null: zero fill); an eleventh segment is refused.
 *   d4_zero_pad_cols             columns c0 .. c1 of x [rows][ld] set to zero.
 *   d4_cvt_pad_bf16              dst [rows][ldd] = bf16(src [rows][lds]) (round to nearest even), columns cols .. cols_pad zero; cols_pad % 8 == 0,
 *                                ldd % 8 == 0, dst 16-byte aligned, anything else is refused.
 *   d4_cvt_transpose_bf16        dst [cols][ldd], dst[c][r] = bf16(src[r][c]) for r < rows, zero for rows <= r < rows_pad. */
int d4_layernorm_rows(const float* x, int ldx, const float* g, const float* b, float* y, int ldy, int rows, int dim, float eps, int silu, void* stream);
typedef struct d4_assemble_desc {
    float* tokens;
    const float* space;
    const float* signal_embed;
    const float* step_embed;
    const float* registers;
    const float* agent_embed;
    const float* task_embed;
    const float* action_embed;
    const float* action_learned;
    const int32_t* signal_levels;
    int32_t signal_uniform;
    const int64_t* prev_actions;
    const float* prev_cont;
    const float* cont_embed;
    const int64_t* tasks;
    const int32_t* action_offsets;
    int32_t B, Tq, S, D, ns, nr, na, nc, step_log2;
    float* compact;
    int32_t has_agent;
} d4_assemble_desc;
int d4_assemble_tokens(const d4_assemble_desc* d, void* stream);
int d4_gather_space_double_norm(const float* tokens, float* out, const float* g0, const float* g1, int frames, int S, int first, int dim, int ns,
                                float eps, void* stream);
int d4_colsum(const float* x, int ld, int rows, int cols, float* out, float* scratch, size_t scratch_floats, void* stream);
int d4_colsum_batch(int n, const float* const* x, const int32_t* ld, const int32_t* rows, const int32_t* cols, float* const* out, void* stream);
int d4_rmsnorm_bwd(const float* x, const float* dxhat, const float* gamma, float* tg, float* dx, int rows, int dim, float eps, void* stream);
int d4_euler_step_rows(float* x, int ldx, const float* pred, int ldp, int B, int n_el, float one_minus_t, float dt, void* stream);
int d4_splitk_reduce(const float* part, int S, int M, int N, const float* bias, int silu, float* y, int ldy, void* stream);
int d4_mean_tokens(const float* x, float* out, int B, int n, int d, void* stream);
int d4_hl_gauss_scalar_strided(const float* logits, int ld, const float* centers, float* out, int out_stride, int rows, int bins, void* stream);
int d4_unary_rows(int op, const float* x, float* y, int64_t n, void* stream);
int d4_copy_rows(const float* src, int lds, float* dst, int ldd, int rows, int cols, void* stream);
int d4_fold_rows(const float* W, const float* gamma, float* out, int rows, int K, int ld_out, void* stream);
int d4_swiglu_pack_rows(const float* W, const float* bias, const float* gamma, float* Wp, float* bp, int inner, int inner_pad, int K, void* stream);
int d4_build_latent_input(float* out, const float* hist, const float* ctx_noise, const float* x, int B, int Tq, int n_el, int hist_t_stride, float w, void* stream);
int d4_pad_cols(const float* W, float* out, int rows, int cols, int cols_pad, void* stream);
int d4_video_patches(const float* src, float* dst, int B, int C, int T, int nh, int nw, int ps, int to_patches, void* stream);
int d4_cache_transfer(float* cache, float* ext, int Lt, int cache_batch, int B, int S, int H, int Tcap, int frames, int to_ext, int dh, void* stream);
int d4_cunembed(int op, const float* src, float* dst, int nc, int mtp, int d, void* stream);
int d4_coord_grid(float* out, int nh, int nw, int ld, void* stream);
int d4_pack_tokens(int which, float* tokens, float* compact, const float* pos, const float* img, const float* lat, int frames, int P, int n_lat, int n_total,
                   int D, void* stream);
int d4_prep_eval_inputs(int32_t* sig, int64_t* pact, const int64_t* actions_hist, int B, int Tq, int na, int frame_base, int hist_stride, int sig_val, int ctx_sig,
                        float* pcont, const float* cont_hist, int nc, void* stream);
int d4_layernorm_silu_bwd(const float* z, int ldz, const float* da, const float* g, const float* b, float* tg, float* tb, float* dz, int rows, int dim, float eps,
                          void* stream);
int d4_silu_bwd(const float* dy, const float* z, float* dz, int64_t n, void* stream);
int d4_swiglu(int bwd, const float* h, const float* du, float* out, int rows, int inner, int inner_pad, void* stream);
int d4_multi_copy(int count, float* const* dst, const float* const* src, const int64_t* n, void* stream);
int d4_zero_pad_cols(float* x, int rows, int ld, int c0, int c1, void* stream);
int d4_cvt_pad_bf16(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int rows, int cols, int cols_pad, void* stream);
int d4_cvt_transpose_bf16(const float* src, int lds, uint16_t* dst, int ldd, int rows, int cols, int rows_pad, void* stream);
int d4_hl_gauss_scalar(const float* logits, int ld, const float* centers, float* out, int rows,
                       int bins, void* stream);
/* MultiCategorical.sample + log_prob of the sample (dreamer4.py:485-497, 1374-1376, 1422-1423), stateless: Gumbel-max per action type from
 * injected uniforms [rows][ld_u] (the layout of the logits), log-softmax gather.  action_sizes: device int32 [na].  Indices are bit-exact
 * against the reference whenever the top-2 (logit / T + Gumbel) margin exceeds fp32 rounding. */
int d4_categorical_sample_logp(const float* logits, int ld, const float* uniform, int ld_u, const int32_t* action_sizes, int rows, int na,
                               float temperature, int64_t* actions, float* log_probs, void* stream);
/* The value branch's loss, stateless (dreamer4.py:6254-6295; HLGaussLoss / SymExpTwoHot targets): HL-Gauss (two_hot = 0: support = [bins + 1] bin
 * edges, sigma in value units) or two-hot (two_hot = 1: support = [bins] bin values) targets of `targets`, cross entropy against `logits`, mean
 * over the rows with mask != 0 (mask null: all rows).  loss[0] and dlogits [rows][ld] = d loss / d logits in one call.
 * scratch >= 2 * rows + 64 floats. */
int d4_hl_gauss_ce(const float* logits, int ld, const float* targets, const float* mask, const float* support, int rows, int bins, float vmin,
                   float vmax, float sigma, float eps, int two_hot, float* loss, float* dlogits, float* scratch, void* stream);
/* The policy branch's loss for discrete actions, stateless (a wrapper of d4_policy_loss below; dreamer4.py:6077-6242: log-prob of the stored actions under the MultiCategorical
 * logits, PPO clipped surrogate (objective 0, dreamer4.py:6204-6212) or SPO (1, dreamer4.py:6188-6198) against the behaviour log-probs
 * [rows][na], entropy bonus, masked mean): loss[0] and dlogits [rows][ld] in one call — the fused kernel d4_learn runs, the advantages taken as
 * given (normalise them before, dreamer4.py:5985-5999).  action_sizes: device int32 [na], `total` their sum.  scratch >= 5 * rows + 64 floats. */
int d4_ppo_policy_loss(const float* logits, int ld, const int64_t* actions, const float* old_log_probs, const float* advantages, const float* mask,
                       const int32_t* action_sizes, int rows, int na, int total, int objective, float eps_clip, float entropy_weight, float* loss,
                       float* dlogits, float* scratch, void* stream);
int d4_gae(const float* rewards, const float* values, const int64_t* lens, const uint8_t* is_truncated,
           const uint8_t* terminals, float gamma, float lam, int batch, int time, float* returns,
           void* stream);
/* d4_gae with the two further outputs the learner consumes: adv [batch][time] = returns - values (values read as 0 past `len`)
 * and mask [batch][time] = 1 on the learnable steps t < len - truncated, 0 elsewhere.  lens null: every trajectory has `time` steps;
 * is_truncated null: every trajectory is truncated; terminals null: none is terminal.  Nothing past `len` is read. */
int d4_gae_adv(const float* rewards, const float* values, const int64_t* lens, const uint8_t* is_truncated, const uint8_t* terminals, float gamma,
               float lam, int batch, int time, float* returns, float* adv, float* mask, void* stream);
/* The whole policy branch's loss, stateless (dreamer4.py:5985-6242; test / tooling use): the descriptor mirrors the learner's
 * PolicyLossArgs (csrc/learn.hip) field by field, and the call runs what d4_learn runs: the masked advantage statistics, the fused forward +
 * backward kernel, the row sums and the final division by max(sum mask, 1).
 *   discrete part (na > 0): logits [rows][ld], actions int64 [rows][na], old_log_probs [rows][na], action_sizes device int32 [na] with sum
 *     `total` <= ld, old_logits [rows][ldo] (pmpo KL; else may be null); dlogits [rows][ld], columns total .. ld written as zero.
 *   continuous part (nc > 0): cparams [rows][ldc] raw Beta parameters (2 per action), actions_cont [rows][nc] in (0, 1), old_log_probs_cont
 *     [rows][nc], old_cparams [rows][nc][2] (pmpo KL; else may be null), beta_param as d4_config.continuous_beta_param; dcparams [rows][ldc],
 *     columns 2 nc .. ldc written as zero.
 *   advantages [rows] raw; normalize != 0: z-scored over the rows with mask != 0, the variance clamped at eps.  mask [rows] or null (all rows).
 *   objective 0 ppo, 1 spo, 2 pmpo; kl_w is read under pmpo only.
 *   loss[0]; row_pl / row_ent / row_aux [rows]: the masked per-row surrogate, negative entropy and KL terms.  scratch >= rows + 64 floats.
 * Refused before any launch: a null argument of a part in use, ld < total, ldc < 2 nc, kl_w > 0 under pmpo without the old logits / parameters,
 * an objective outside 0 .. 2. */
typedef struct d4_policy_loss_desc {
    const float* logits; int32_t ld;
    const int64_t* actions;
    const float* old_log_probs;
    const float* old_logits; int32_t ldo;
    const float* advantages;
    const float* mask;
    const int32_t* action_sizes;
    int32_t rows, na, total;
    const float* cparams; int32_t ldc;
    const float* actions_cont;
    const float* old_log_probs_cont;
    const float* old_cparams;
    int32_t nc, beta_param;
    int32_t objective, normalize, use_gate, reverse_kl;
    float eps, clip, ent_w, gate_temp, pmpo_alpha, kl_w;
    float* loss;
    float* dlogits;
    float* dcparams;
    float* row_pl;
    float* row_ent;
    float* row_aux;
    float* scratch;
} d4_policy_loss_desc;
int d4_policy_loss(const d4_policy_loss_desc* d, void* stream);
/* Return statistics of keep_reward_ema_stats, stateless (dreamer4.py:5985-6015): one workgroup, no host synchronisation.
 *   x = returns[i] with mask[i] != 0 (mask null: all n); lo, hi = their q_lo / q_hi quantiles (linear interpolation, exact order statistics by a
 *   four-pass radix selection, any n); mean, var = mean and biased variance of clamp(x, lo, hi);
 *   ema[0] <- lerp(ema[0], mean, 1 - reward_ema_decay), ema[1] likewise with var (in place; untouched when no element is kept);
 *   adv[i] = (returns[i] - ema[0]) / std - (old_values[i] - ema[0]) / std for all n, std = sqrt(max(ema[1], 1e-5)), from the UPDATED pair;
 *   stats[4] = lo, hi, mean, var (zeros when no element is kept). */
int d4_return_stats(const float* returns, const float* old_values, const float* mask, int64_t n, float* ema, double reward_ema_decay, float q_lo,
                    float q_hi, float* adv, float* stats, void* stream);
/* The value branch's loss with PPO value clipping, stateless (dreamer4.py:6254-6295).  The fields are d4_hl_gauss_ce's arguments, plus
 * old_values [rows], clip_values and value_clip, plus row_loss [rows] (the masked per-row losses).  clip_values = 0: d4_hl_gauss_ce's launches and
 * bits (old_values may be null).  clip_values != 0: per row  values = sum softmax(logits) * centres (bin centres of the edges / the two-hot bin
 * values), clipped = old + clamp(values - old, +-value_clip), q = the targets' encoder applied to clipped (same range clamp),
 * loss = max(CE, -sum p log max(q, 1e-20)) and dlogits its gradient (through q and values where the clipped branch wins and no clamp is active).
 * scratch >= rows + 64 floats. */
typedef struct d4_value_loss_desc {
    const float* logits; int32_t ld;
    const float* returns;
    const float* old_values;
    const float* mask;
    const float* support;
    int32_t rows, bins;
    float vmin, vmax, sigma, eps;
    int32_t two_hot, clip_values;
    float value_clip;
    float* loss;
    float* row_loss;
    float* dlogits;
    float* scratch;
} d4_value_loss_desc;
int d4_value_loss(const d4_value_loss_desc* d, void* stream);
/* Pixel-side operators of the VideoTokenizer training forward (dreamer4.py:4239-4603; csrc/tok_train.hip).  Patch rows are
 * [(b t nh nw)][(p1 p2 c)] of a video (b c t (nh p1) (nw p2)); the patch row C * ps * ps and every `dim` must be multiples of 4, row pointers 16-byte
 * aligned.  No allocation, no host synchronisation; column sums and the loss sum go through per-block partials in the caller's `part` and one
 * fixed-order reduction (no float atomics): equal inputs give equal bits.
 *   d4_flow_noised_patches   rows = patch rows of noise.lerp(video, t[b]) (torch's lerp: t = 1 gives d4_video_patches' bits, t = 0 the noise's).
 *                            noise and t both null: the video's own patch rows, d4_video_patches' bits.
 *   d4_tok_rows_part_floats  floats of `part` the two row backward operators need for `rows` rows of `dim`.
 *   d4_layernorm_rows_bwd    backward of y = LayerNorm(x) * g (no bias, biased variance) on x [rows][ldx], dy [rows][dim]: dx [rows][ldx] and
 *                            dg [dim] = sum over rows of dy * xhat.  dim <= 1024.
 *   d4_mask_rows_fwd         y [rows][dim] = token where mask[row] != 0, x elsewhere.
 *   d4_mask_rows_bwd         dx = dy on unmasked rows, 0 on masked rows; dtoken [dim] = sum of dy over the masked rows.  dim <= 1024.
 *   d4_recon_loss_fwd_bwd    loss[0] = mean((pred - target)^2) over all B C T H W elements and d_rows = d loss / d recon_rows.  v_space 1:
 *                            pred = (recon - noise.lerp(video, t)) / (1 - t), target = video - noise (t[b] < 1); v_space 0: pred = recon,
 *                            target = video (noise and t may be null).  part: at least 1024 floats. */
int d4_flow_noised_patches(const float* video, const float* noise, const float* t, float* rows, int B, int C, int T, int nh, int nw, int ps, void* stream);
size_t d4_tok_rows_part_floats(int rows, int dim);
int d4_layernorm_rows_bwd(const float* x, int ldx, const float* dy, const float* g, float* dx, float* dg, float* part, size_t part_floats, int rows, int dim,
                          float eps, void* stream);
int d4_mask_rows_fwd(const float* x, const uint8_t* mask, const float* token, float* y, int rows, int dim, void* stream);
int d4_mask_rows_bwd(const float* dy, const uint8_t* mask, float* dx, float* dtoken, float* part, size_t part_floats, int rows, int dim, void* stream);
int d4_recon_loss_fwd_bwd(const float* recon_rows, const float* video, const float* noise, const float* t, int B, int C, int T, int nh, int nw, int ps, int v_space,
                          float* loss, float* d_rows, float* part, size_t part_floats, void* stream);
/* Latent regularisers of the VideoTokenizer training forward (dreamer4.py:728-767, 389-402; csrc/tok_reg.hip).  Each call writes the loss and
 * d loss / d x for a unit upstream gradient.  No allocation, no host synchronisation, no float atomics: equal inputs give equal bits.
 *   d4_sigreg_fwd_bwd        sigreg(x) without a mask on x [K][N][d], projs [M][d] the RAW normal draw (each row is normalised as F.normalize does, eps
 *                            1e-12): the empirical characteristic function per (k, slice, knot) as the mean over N at the knots linspace(lo, hi,
 *                            num_knots), squared distance to exp(-t^2 / 2) weighted by exp(-t^2 / 2), trapezoid over the knots, mean over (K, M).
 *                            d <= 128, 2 <= num_knots <= 64, M <= 4096, K <= 65535; anything else is an error.  Nothing of size N * M is written.
 *   d4_sigreg_part_floats    floats of `part` it needs: 2 K M num_knots per block of 64 rows of N, plus ceil(K M num_knots / 256).
 *   d4_latent_ortho_fwd_bwd  orthogonal_loss(x) on x [F][n][d]: per frame centre over n, F.normalize the rows, sum of the squared off-diagonal entries
 *                            of the n x n Gram; mean over F.  n <= 1024, d <= 128.  n = 1 gives exactly 0 and a zero gradient.
 *   d4_latent_ortho_part_floats  floats of `part` it needs (F). */
size_t d4_sigreg_part_floats(int K, int N, int M, int num_knots);
int d4_sigreg_fwd_bwd(const float* x, const float* projs, int K, int N, int d, int M, float lo, float hi, int num_knots, float* loss, float* dx, float* part,
                      size_t part_floats, void* stream);
size_t d4_latent_ortho_part_floats(int F);
int d4_latent_ortho_fwd_bwd(const float* x, int F, int n, int d, float* loss, float* dx, float* part, size_t part_floats, void* stream);
/* d4_pack_tokens that also writes the bf16 image of the token rows (the bf16 tokenizer engine's slab 0, VideoTokenizer(matmul_dtype='bf16');
 * DESIGN.md 27): tokens and compact carry d4_pack_tokens' bits, tokens_b [frames * (P + n_lat)][D] their round-to-nearest-even bf16 values, written
 * by the same pass (16-byte stores at D % 8 == 0 with 32-byte aligned fp32 buffers and a 16-byte aligned image, 8-byte stores at D % 4 == 0,
 * element stores otherwise).  compact_b (may be null): the bf16 image of `compact`, same layout, likewise.  Nothing past the rows named is written. */
int d4_pack_tokens_bf16(int which, float* tokens, uint16_t* tokens_b, float* compact, uint16_t* compact_b, const float* pos, const float* img, const float* lat,
                        int frames, int P, int n_lat, int n_total, int D, void* stream);

/* ---- MuonAdamAtan2 (csrc/muon.hip) ------------------------------------------------------------------------------------
 * A plan describes a group of 2-D fp32 matrices (rows[i] x cols[i], contiguous) and owns the device tables of its launches: per pass one
 * table of prepare / finish workgroups and two tile tables (matrix, tile row, tile col) of the grouped products.  Matrices are taken in
 * order into passes whose work buffers (X, X', A, B per matrix, every dimension padded to 128) fit `workspace_bytes`; one matrix that
 * does not fit alone is refused by name.  The caller provides the workspace (256-byte aligned, at least workspace_bytes(plan): the work
 * buffers of the largest pass plus the strip partials of the Frobenius norms).
 *   d4_muon_step        per matrix W with gradient g and momentum m (g read as g * min(1, max_grad_norm / (sqrt(*grad_norm_sq) + 1e-6))
 *                       when grad_norm_sq is given and max_grad_norm > 0):
 *                         m <- lerp(m, g, 1 - beta);  u = nesterov ? lerp(g, m, beta) : m;  X = NS(u);
 *                         W <- W (1 - lr weight_decay) - lr update_scale[i] X
 *                       params / grads / exp_avg / update_scale: HOST arrays of the plan's length (device pointers; host floats).
 *                       The device pointer table is uploaded only when a pointer or a scale changed since the last call.
 *   d4_newton_schulz    out[i] = NS(in[i]) alone, through the same launchers (in / out: host arrays of device pointers):
 *                         X = u / max(|u|_F, eps), oriented rows <= cols;  `steps` times  A = X X^T, B = b A + c A A, X <- a X + B X.
 * Launches per call: passes * (2 + 3 * steps).  Fixed-order reductions, no float atomics: equal inputs and state give equal bits, and the
 * pass partition does not change them.  Learning rates, betas and weight decay are doubles: the lerp weights 1 - beta, the decay factor
 * 1 - lr wd and the bias corrections are formed in double and rounded once (1 - 0.99f is 1e-6 off 0.01).
 *   d4_multi_table_bytes / d4_sumsq_multi / d4_adam_atan2_multi   multi-tensor kernels over a device table of n tensors (numel[i] >= 1
 *                       elements each; host arrays).  `table`: caller-owned device memory of d4_multi_table_bytes(n, numel) bytes, 16-byte
 *                       aligned; upload != 0 (re)writes it from the host pointer arrays (needed at first use and whenever a pointer
 *                       changed), upload == 0 reuses it and ignores the pointer arrays.
 *                         d4_sumsq_multi       out[0] = sum over all tensors of x^2 (per-4096-element partials, then one block).
 *                         d4_adam_atan2_multi  m <- lerp(m, g, 1 - beta1); v <- lerp(v, g^2, 1 - beta2);
 *                                              W <- W (1 - lr wd) - lr a atan2(m / (1 - beta1^step), b sqrt(v / (1 - beta2^step)))
 *                                              with g clipped as in d4_muon_step.  One launch.
 *   d4_muon_plan_create_products   the plan with its product form chosen.  products 0: exactly d4_muon_plan_create.  products 1: the
 *                       Newton-Schulz products on the bf16 matrix pipe (csrc/muon_bf16.hip): prepare and finish stay fp32 (the momentum holds the
 *                       same bits), X0 = bf16(u / max(|u|_F, eps)) is rounded once after the fp32 scaling, every product takes bf16 operands with
 *                       fp32 accumulation and rounds its fp32 epilogue once; all work buffers are bf16 and the workspace is not larger than the
 *                       fp32 plan's.  Launches per call: passes * (3 + 3 * steps).  Any other value is refused.  The mode belongs to the plan:
 *                       d4_muon_step, d4_newton_schulz, d4_muon_plan_workspace_bytes and d4_muon_plan_passes follow it.
 *   d4_muon_plan_products          the plan's product form (0 or 1). */
typedef struct d4_muon_plan d4_muon_plan;
int d4_muon_plan_create(int n, const int32_t* rows, const int32_t* cols, size_t workspace_bytes, d4_muon_plan** out);
int d4_muon_plan_create_products(int n, const int32_t* rows, const int32_t* cols, size_t workspace_bytes, int products, d4_muon_plan** out);
int d4_muon_plan_products(const d4_muon_plan* plan);
void d4_muon_plan_destroy(d4_muon_plan* plan);
size_t d4_muon_plan_workspace_bytes(const d4_muon_plan* plan);
int d4_muon_plan_passes(const d4_muon_plan* plan);
int d4_muon_step(d4_muon_plan* plan, void* const* params, const void* const* grads, void* const* exp_avg, const float* update_scale, void* workspace,
                 size_t workspace_bytes, double lr, double weight_decay, double beta, int nesterov, int steps, float a, float b, float c, float eps,
                 const float* grad_norm_sq, float max_grad_norm, void* stream);
int d4_newton_schulz(d4_muon_plan* plan, const void* const* in, void* const* out, void* workspace, size_t workspace_bytes, int steps, float a, float b,
                     float c, float eps, void* stream);
size_t d4_multi_table_bytes(int n, const int64_t* numel);
int d4_sumsq_multi(int n, const int64_t* numel, const void* const* x, void* table, size_t table_bytes, int upload, float* out, void* stream);
int d4_adam_atan2_multi(int n, const int64_t* numel, void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, void* table,
                        size_t table_bytes, int upload, int step, double lr, double beta1, double beta2, double weight_decay, double a, double b,
                        const float* grad_norm_sq, float max_grad_norm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* D4HIP_H */
