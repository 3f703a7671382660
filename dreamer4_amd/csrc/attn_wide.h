// Wide-frame attention core of the inference path, the part its product forms share: the semantics of attn.hip's attn_wide_kernel
// (value-residual mix, key l2-norm * (gamma + 1) * sqrt(dh), scores * dh^-1/2, softclamp, special-token rule, softmax, . v, belief
// projection, head gate) for head dims 16 / 32 / 64, nq != nk, and up to WIDE_ATTN_MAX items per side — forward only, one launch, no
// workspace.  The two matrix products, their fragments and the LDS layout belong to a policy type Prod (fp32: attn_wide_mfma.hip's
// ProdF32, bf16: attn_wide_bf16.hip's ProdBf16); everything else is fp32 and is written here once.
//
//   grid (groups * heads, ceil(nq / 64)), 256 threads: wave w of a block owns queries 64 blockIdx.y + 16 w .. + 15.
//   The keys go in tiles of 64.  Per tile the four waves prepare the keys and values ONCE into LDS (wave w: keys 16 w .. + 15 of the
//   tile, lane = (key l & 15, feature quarter kq = l >> 4), features 16 s + 4 kq .. + 3: DH / 16 float4 per operand and lane (a misaligned
//   value residual: by floats); rows past nk are zero-filled and never addressed in global memory), then every wave scores its 16 queries
//   against the tile.  Both products run in the orientation of attn_tiled.hip's tiled_fwd_kernel: S^T tiles (accumulator rows = keys:
//   register r of lane (tok, kq) of sub-tile kt is S[query tok][key 16 kt + 4 kq + r]), so P goes from its accumulator registers straight
//   into P V as the A operand; online softmax per 64 keys (attn_mfma.h: online_softmax_step).
//
// Prod<DH> supplies: Lds (the static __shared__ storage), QFrag and load_q (the query's B fragments of Q K^T), stage (one prepared key /
// value row into LDS; called by every lane of every wave), scores (one 16-key S^T sub-tile) and pv (o += P V' over the tile, with the
// policy's own skip granularity).
//
// Barriers: every wave of a block — also one whose 16 queries are all past nq — runs the same number of tile steps (the bound is the
// maximum over the block's waves, computed from block-uniform values only), stages its keys and meets both barriers of every step; a wave
// with nothing left to score skips the products, never a barrier.  There is no early return.
//
// Deterministic: no atomics, every sum in a fixed order.  Capture-safe: no host synchronisation, no attribute call (static LDS).
#pragma once
#include "common.h"
#include "kernels.h"
#include "attn_mfma.h"
#include <float.h>

namespace d4 {

constexpr int WIDE_WT = 64;                              // keys per tile

template <int DH, class Prod>
__device__ __forceinline__ void wide_attn_body(const SmallAttnArgs& p) {
    constexpr int NS = DH / 16;
    __shared__ typename Prod::Lds lds;
    const int nq = p.nq, nk = p.nk, ms = p.mask_special;
    const int g = blockIdx.x / p.heads, h = blockIdx.x % p.heads;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, tok = lane & 15, kq = lane >> 4;
    const int b0 = blockIdx.y * 64, i0 = b0 + 16 * w;
    const int n_ord = ms > 0 ? nq - ms : 0;              // queries below n_ord are ordinary: they see the first nk - ms keys only
    const int k_ord = nk - ms;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // the engine's value-residual rows start 3 hd + 2 heads floats into a projection row: 16-byte aligned with an even number of heads only
    const bool r_al4 = ((uintptr_t)p.vres % 16) == 0 && (p.r_group_stride % 4) == 0 && (p.r_item_stride % 4) == 0;
    // the last key any of the queries i0w .. i0w + 15 sees (a wave of ordinary queries stops before the special block); -1: no query
    auto wave_last_key = [&](int i0w) { return i0w >= nq ? -1 : (i0w + 15 < n_ord ? k_ord - 1 : nk - 1); };
    const int jmax = wave_last_key(i0);
    int jmax_blk = -1;                                   // block-uniform: the tile loop's bound
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) jmax_blk = max(jmax_blk, wave_last_key(b0 + 16 * ww));

    const float scale = rsqrtf((float)DH);
    const int i = i0 + tok;
    const bool ordinary = i < n_ord;
    typename Prod::QFrag q;
    f32x4 o[NS], gk[NS];
    {
        const float ksc = sqrtf((float)DH);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            o[s] = zero;
#pragma unroll
            for (int e = 0; e < 4; ++e) gk[s][e] = (p.k_gamma[h * DH + 16 * s + 4 * kq + e] + 1.f) * ksc;
        }
    }
    Prod::load_q(q, p.q + g * p.q_group_stride + (int64_t)i * p.q_item_stride + h * DH, i < nq, kq);
    float m = -FLT_MAX, l = 0.f;

    for (int j0 = 0; j0 <= jmax_blk; j0 += WIDE_WT) {
        // ---- stage keys j0 .. j0 + 63: wave w prepares key j0 + 16 w + tok (every wave, whatever its queries)
        {
            const int jl = 16 * w + tok, j = j0 + jl;
            f32x4 k4[NS], v4[NS];
            if (j < nk) {
                const float* kr = p.k + g * p.k_group_stride + (int64_t)j * p.k_item_stride + h * DH + 4 * kq;
                const float* vr = p.v + g * p.v_group_stride + (int64_t)j * p.v_item_stride + h * DH + 4 * kq;
#pragma unroll
                for (int s = 0; s < NS; ++s) { k4[s] = *reinterpret_cast<const f32x4*>(kr + 16 * s); v4[s] = *reinterpret_cast<const f32x4*>(vr + 16 * s); }
                if (p.vres) {
                    const float* rr = p.vres + g * p.r_group_stride + (int64_t)j * p.r_item_stride + h * DH + 4 * kq;
                    const float wm = sigmoidf(p.mix[g * p.m_group_stride + (int64_t)j * p.m_item_stride + h]);
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        f32x4 r4;
                        if (r_al4) r4 = *reinterpret_cast<const f32x4*>(rr + 16 * s);
                        else { r4[0] = rr[16 * s]; r4[1] = rr[16 * s + 1]; r4[2] = rr[16 * s + 2]; r4[3] = rr[16 * s + 3]; }
#pragma unroll
                        for (int e = 0; e < 4; ++e) v4[s][e] = lerp_torch(v4[s][e], r4[e], wm);
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < NS; ++s) { k4[s] = zero; v4[s] = zero; }
            }
            float ss = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e) ss = __builtin_fmaf(k4[s][e], k4[s][e], ss);
            ss += __shfl_xor(ss, 16); ss += __shfl_xor(ss, 32);            // (the four feature quarters of a key sit on lanes tok + 16 kq)
            const float nrm = fmaxf(sqrtf(ss), 1e-12f);
            Prod::stage(lds, jl, w, tok, kq, k4, v4, nrm, gk);              // (the whole wave is here: a policy may exchange across lanes)
        }
        __syncthreads();

        if (j0 <= jmax) {                                   // (wave-uniform; no barrier inside)
            // scores of 64 keys, transposed tiles: pr[kt][r] = S[i][j0 + 16 kt + 4 kq + r]
            f32x4 pr[4];
            float mt = -FLT_MAX;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const int jb = j0 + 16 * kt;
                pr[kt] = f32x4{-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
                if (jb > jmax) continue;                    // (wave-uniform)
                const f32x4 st = Prod::scores(lds, kt, tok, kq, q);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = jb + 4 * kq + r;
                    float simc = st[r] * scale;
                    if (p.softclamp > 0.f) simc = tanhf(simc / p.softclamp) * p.softclamp;
                    const bool sees = j < nk && !(ordinary && j >= k_ord);
                    pr[kt][r] = sees ? simc : -FLT_MAX;
                    mt = fmaxf(mt, pr[kt][r]);
                }
            }
            online_softmax_step<NS>(pr, mt, m, l, o, kq);
            Prod::pv(lds, pr, o, j0, jmax, tok, kq);
        }
        __syncthreads();                                    // the tile is consumed: the next step overwrites it
    }

    // ---- epilogue: accumulator row r of lane (tok, kq) is query i0 + 4 kq + r, feature 16 s + tok
    const float linv = 1.f / l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float lr = __shfl(linv, 4 * kq + r);
        const int qi = i0 + 4 * kq + r;
        if (qi >= nq) continue;                             // (uniform over each 16-lane row group)
        float on[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) on[s] = o[s][r] * lr;
        if (p.belief) {                                     // self attention: orthogonalise against query qi's own (mixed) fp32 value row
            const float* vr = p.v + g * p.v_group_stride + (int64_t)qi * p.v_item_stride + h * DH + tok;
            float vi[NS], vsq = 0.f, dot = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) vi[s] = vr[16 * s];
            if (p.vres) {
                const float* rr = p.vres + g * p.r_group_stride + (int64_t)qi * p.r_item_stride + h * DH + tok;
                const float wm = sigmoidf(p.mix[g * p.m_group_stride + (int64_t)qi * p.m_item_stride + h]);
#pragma unroll
                for (int s = 0; s < NS; ++s) vi[s] = lerp_torch(vi[s], rr[16 * s], wm);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) vsq = __builtin_fmaf(vi[s], vi[s], vsq);
            const float vinv = 1.f / fmaxf(sqrtf(row_sum16(vsq)), 1e-12f);
#pragma unroll
            for (int s = 0; s < NS; ++s) { vi[s] *= vinv; dot = __builtin_fmaf(on[s], vi[s], dot); }
            dot = row_sum16(dot);
#pragma unroll
            for (int s = 0; s < NS; ++s) on[s] -= dot * vi[s];
        }
        const float gt = p.gate ? sigmoidf(p.gate[g * p.g_group_stride + (int64_t)qi * p.g_item_stride + h]) : 1.f;
        const int64_t ooff = g * p.o_group_stride + (int64_t)qi * p.o_item_stride + h * DH + tok;
        float* orow = p.out + ooff;
#pragma unroll
        for (int s = 0; s < NS; ++s) orow[16 * s] = on[s] * gt;
        if (p.out_b) {                                      // the bf16 image of the same rows (bf16 engine): the value just stored, rounded to nearest even
            uint16_t* brow = p.out_b + ooff;
#pragma unroll
            for (int s = 0; s < NS; ++s) brow[16 * s] = bf16_bits(on[s] * gt);
        }
    }
}

// The head-dim ladder of both forms on validated arguments: names the instantiation of the __global__ template KERNEL in *form and launches it.
#define D4_WIDE_ATTN_LAUNCH(KERNEL, p, stream, form)                                                                    \
    do {                                                                                                                \
        const dim3 grid((unsigned)((int64_t)(p).groups * (p).heads), (unsigned)cdiv((p).nq, 64)), block(256);           \
        if ((p).dh == 64) { *(form) = #KERNEL "<64>"; hipLaunchKernelGGL(KERNEL<64>, grid, block, 0, stream, p); }      \
        else if ((p).dh == 32) { *(form) = #KERNEL "<32>"; hipLaunchKernelGGL(KERNEL<32>, grid, block, 0, stream, p); } \
        else { *(form) = #KERNEL "<16>"; hipLaunchKernelGGL(KERNEL<16>, grid, block, 0, stream, p); }                   \
        D4_LAUNCH_CHECK();                                                                                              \
    } while (0)

}  // namespace d4
