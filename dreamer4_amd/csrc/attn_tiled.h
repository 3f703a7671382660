// The attention cores of the training path: the argument blocks shared by the whole-problem-in-LDS kernels (backward.hip: attn_bwd_kernel,
// xattn_bwd_kernel, <= 64 items per group and side) and the tiled core (attn_tiled.hip, up to ATT_MAX_FRAMES items: the time layers, and
// with d4_train_wide_set(1) the within-frame and cross attentions).
#pragma once
#include "common.h"
#include "kernels.h"
#include <stdint.h>

namespace d4 {

// F groups of S items, one attention problem per (group, head), head dim DH <= 64.  Rows of proj: q @ 0, k @ hd, v @ 2hd,
// gate logit @ 3hd + head, mix logit @ 3hd + hp4 + head  (hd = heads * DH, hp4 = heads rounded up to 4).
struct AttnBwdArgs {
    const float* proj; int ldp;        // [F*S][ldp] forward projections (mix logits include their bias)
    const float* rv;                   // [F*S][hd] value residual or null
    const float* gamma;                // [heads][DH]
    const float* d_o3;                 // [F*S][hd] gradient of the gated attention output (before to_out); null: forward only
    float* o3;                         // [F*S][hd] out: gated attention output (recomputed forward)
    float* dproj;                      // [F*S][ldp] out: gradients of the projections (same columns)
    float* d_rv;                       // [F*S][hd] out (when rv)
    float* dgamma_part;                // [F][hd] out: per-frame partial of d gamma
    int F, S, heads, hp4;              // F groups of S items
    float softclamp; int num_special, belief;
    // row of item j of group g = (g / g_inner) * g_outer_stride + (g % g_inner) + j * item_stride:
    //   within-frame attention: g_inner 1, g_outer_stride S, item_stride 1;  time attention over [B][T][S] rows: g_inner S, g_outer_stride T * S, item_stride S
    int g_inner = 1; int64_t g_outer_stride = 0, item_stride = 1;
    int causal = 0;                    // item i sees items j <= i
    const float* inv_freq = nullptr;   // [DH / 2] rotary frequencies applied to q and k at position j (time attention), or null
};

// Cross attention: G groups of nq queries over nk keys, one problem per (group, head).  projq rows: q @ 0, gate logit @ hd + head; projk rows: k @ 0, v @ hd.
struct XAttnArgs {
    const float* projq; int ldq;       // [G * nq][ldq], row g * nq + i
    const float* projk; int ldk;       // key j of group g: row g * nk + j (group major) or j * G + g (item major: the stack of hiddens)
    const float* gamma;
    const float* d_o3;                 // [G * nq][hd] or null (forward only)
    float* o3;                         // [G * nq][hd]
    float* dprojq; float* dprojk;      // gradients, same layouts
    float* dgamma_part;                // [G][hd]
    int G, nq, nk, heads, item_major;
    float softclamp;
};

constexpr int ATT_MAX_FRAMES = 1024;   // cap of the tiled core, items per problem side (the per-row planes and the post-pass are sized for it)

// floats of per-row planes the tiled core needs behind the block's workspace (R rows in all; cross: Rq query rows, Rk key rows)
size_t attn_tiled_floats(int R, int heads, int dh);
size_t attn_tiled_cross_floats(int Rq, int Rk, int heads, int dh);
// the time geometry (causal, rotary) or the within-frame geometry (neither; num_special): same outputs as attn_bwd_kernel (o3; with d_o3 also dproj, d_rv, dgamma_part)
int attn_tiled_core(const AttnBwdArgs& a, int dh, float* planes, hipStream_t s);
// the cross geometry: same outputs as xattn_bwd_kernel (o3; with d_o3 also dprojq, dprojk, dgamma_part)
int attn_tiled_cross_core(const XAttnArgs& a, int dh, float* planes, hipStream_t s);

// The same two cores with their six products on the bf16 matrix pipe (attn_tiled_bf16.hip; d4_train_attn_products_set(1)): the planes above and,
// behind them, the bf16 images, which depend on the items per problem (the transposed ones are padded to 32 items per problem)
size_t attn_tiled_bf16_floats(int groups, int items, int heads, int dh);
size_t attn_tiled_bf16_cross_floats(int groups, int nq, int nk, int heads, int dh);
int attn_tiled_bf16_core(const AttnBwdArgs& a, int dh, float* planes, hipStream_t s);
int attn_tiled_bf16_cross_core(const XAttnArgs& a, int dh, float* planes, hipStream_t s);

}  // namespace d4
