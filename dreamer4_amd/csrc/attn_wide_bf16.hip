// Wide-frame attention core of the inference path with both products on the bf16 matrix pipe (opt-in: SmallAttnArgs::wide == 2): the
// semantics, arguments, refusals, grid and barrier discipline of attn_wide_mfma.hip's wide_attn_kernel<DH>, forward only, one launch, no
// workspace, static LDS.
//
// Arithmetic: k' = k / max(|k|, 1e-12) (gamma + 1) sqrt(dh) and v' = v + sigmoid(mix) (vres - v) in fp32, then rounded to bf16 (nearest
// even) on their way into LDS; q rounded to bf16 in registers; S = q^ k^'^T on v_mfma_f32_16x16x32_bf16 with fp32 accumulate; scale,
// soft clamp, special-token rule and the online softmax per 64-key tile in fp32; p = exp(s - m_running) rounded to bf16 for p^ v^' (same
// instruction), the row sum from the unrounded p; belief projection (the query's own fp32 v' row, re-read from global memory), head gate
// and output in fp32.  Head dim 16: the 32-deep contraction of Q K^T is zero-padded (the lanes of k = 16 .. 31 carry a zero q fragment).
//
//   grid (groups * heads, ceil(nq / 64)), 256 threads: wave w of a block owns queries 64 blockIdx.y + 16 w .. + 15; keys in tiles of 64.
//   Staging (every wave, once per tile): wave w prepares key 16 w + (l & 15) of the tile, lane = (key l & 15, feature quarter kq = l >> 4),
//   features 16 s + 4 kq .. + 3.  Rows past nk are zero-filled and never addressed in global memory.
//   S^T tiles (accumulator rows = keys): register r of lane (tok, kq) of sub-tile kt is S[query tok][key 16 kt + 4 kq + r], so the eight
//   registers of sub-tiles 2 u, 2 u + 1, packed to bf16, ARE the A fragment of P V' over the 32 keys of half u — in the key order
//   slot 8 kq + j <-> key 16 (j >> 2) + 4 kq + (j & 3) of the half.  V' is kept transposed in that slot order.
//
// LDS (16 KB at DH 64, static):
//   Ks [64 keys][DH] bf16, natural feature order, in 16-byte chunks (8 features); chunk c of row r sits at chunk c ^ f(r) with
//      f(r) = (r >> 1) & 7 (DH 64: 8 chunks), (-(r >> 2)) & 3 (DH 32: 4 chunks), 0 (DH 16: 2 chunks).
//   Vt [DH features][64 slots] bf16 (128-byte rows = 8 chunks of 8 slots), chunk c of row r at c ^ ((r >> 1) & 7) ^ ((r & 1) << 2).
//   Reads are one ds_read_b128 per fragment: lane (tok, kq) reads chunk 4 s + kq of row 16 kt + tok.  With the 16-lane service groups of
//   ds_read_b128 ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) and the bank (byte / 4) % 64, every group's 16 lanes cover
//   the 16 16-byte slots of the 256-byte bank row exactly once for each DH: conflict-free (computed from the bank rule, not measured).
//   Writes are ds_write_b64 (groups of 16 consecutive lanes, bank (byte / 4) % 32): in Ks two rows share a bank pair at DH 64 and 32 (2-way), four
//   at DH 16 (4-way, one store per tile); Vt's store is 2-way at every DH (computed, not measured).  The value tile is transposed in registers
//   first: the four lanes of a quad (keys 4 g .. 4 g + 3, four features each) exchange bf16 pairs by two DPP quad permutes, after which a
//   lane holds ONE feature of the quad's four keys = four consecutive slots = one 8-byte store.
//
// Barriers: as wide_attn_kernel — every wave of a block, also one whose 16 queries are all past nq, runs the same number of tile steps (a
// block-uniform bound), stages its keys and meets both barriers of every step; a wave with nothing left to score skips the products, never
// a barrier.  There is no early return.
//
// Deterministic: no atomics, every sum in a fixed order.  Capture-safe: no host synchronisation, no attribute call (static LDS).
#include "common.h"
#include "kernels.h"
#include "attn_mfma.h"
#include <float.h>

namespace d4 {

namespace {

constexpr int WT = 64;                                   // keys per tile

typedef __bf16 wb_b8 __attribute__((ext_vector_type(8)));
typedef __bf16 wb_b2 __attribute__((ext_vector_type(2)));
typedef uint32_t wb_u2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {      // (a in the low half): v_cvt_pk_bf16_f32, round to nearest even
    wb_b2 o;
    o[0] = (__bf16)a; o[1] = (__bf16)b;
    return __builtin_bit_cast(uint32_t, o);
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
template <int DH>
__device__ __forceinline__ int ks_swz(int row) {         // Ks: the chunk swizzle f(row) of the header
    return DH == 64 ? ((row >> 1) & 7) : DH == 32 ? ((-(row >> 2)) & 3) : 0;
}

__device__ __forceinline__ int vt_swz(int row) {         // Vt: the same for its 128-byte rows (bit 0 of the row spreads the 8-byte stores over all banks)
    return ((row >> 1) & 7) ^ ((row & 1) << 2);
}

template <int DH>
__global__ __launch_bounds__(256) void wide_attn_bf16_kernel(SmallAttnArgs p) {
    constexpr int NS = DH / 16;                          // float4 per operand and lane in staging; 16-feature output tiles
    constexpr int KS = DH == 64 ? 2 : 1;                 // 32-deep contraction steps of Q K^T
    __shared__ __attribute__((aligned(16))) uint16_t Ks[WT * DH];
    __shared__ __attribute__((aligned(16))) uint16_t Vt[DH * WT];
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
    // B fragments of Q K^T: q[i][32 s + 8 kq .. + 7] as bf16 (DH 16: the lanes kq >= 2 pad the contraction with zeros)
    wb_b8 qf[KS];
    f32x4 o[NS], gk[NS];
    {
        const bool qok = i < nq && (DH > 16 || kq < 2);
        const float* qrow = p.q + g * p.q_group_stride + (int64_t)i * p.q_item_stride + h * DH + (DH > 16 ? 8 * kq : 8 * (kq & 1));
        const float ksc = sqrtf((float)DH);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const f32x4 a = qok ? *reinterpret_cast<const f32x4*>(qrow + 32 * s) : zero;
            const f32x4 b = qok ? *reinterpret_cast<const f32x4*>(qrow + 32 * s + 4) : zero;
#pragma unroll
            for (int e = 0; e < 4; ++e) { qf[s][e] = (__bf16)a[e]; qf[s][4 + e] = (__bf16)b[e]; }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            o[s] = zero;
#pragma unroll
            for (int e = 0; e < 4; ++e) gk[s][e] = (p.k_gamma[h * DH + 16 * s + 4 * kq + e] + 1.f) * ksc;
        }
    }
    float m = -FLT_MAX, l = 0.f;

    for (int j0 = 0; j0 <= jmax_blk; j0 += WT) {
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
            const int c = tok & 3, tg = tok >> 2;                          // (the whole wave is here: the quad exchanges below see every lane)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                // k': features 16 s + 4 kq .. + 3 of key jl = half (kq & 1) of chunk 2 s + (kq >> 1) of row jl
                wb_u2 kn;
                kn[0] = pk_bf16(k4[s][0] / nrm * gk[s][0], k4[s][1] / nrm * gk[s][1]);
                kn[1] = pk_bf16(k4[s][2] / nrm * gk[s][2], k4[s][3] / nrm * gk[s][3]);
                *reinterpret_cast<wb_u2*>(Ks + jl * DH + 8 * ((2 * s + (kq >> 1)) ^ ks_swz<DH>(jl)) + 4 * (kq & 1)) = kn;
                // v': 4 keys x 4 features of a quad, transposed: lane c ends with feature 16 s + 4 kq + c of keys 4 tg .. 4 tg + 3
                const uint32_t d0 = pk_bf16(v4[s][0], v4[s][1]), d1 = pk_bf16(v4[s][2], v4[s][3]);
                const bool up = (c & 2) != 0, odd = (c & 1) != 0;
                const uint32_t got = dpp_u<0x4E>(up ? d0 : d1);            // quad_perm [2,3,0,1]: lane c ^ 2
                const uint32_t x0 = up ? got : d0, x1 = up ? d1 : got;      // features 2 (c >> 1), + 1 of keys (c & 1), (c & 1) + 2
                const uint32_t lo = (x0 & 0xffffu) | (x1 << 16), hi = (x0 >> 16) | (x1 & 0xffff0000u);
                const uint32_t oth = dpp_u<0xB1>(odd ? lo : hi);            // quad_perm [1,0,3,2]: lane c ^ 1
                wb_u2 vt;                                                   // feature c of keys 0, 1 | 2, 3 of the quad
                vt[0] = odd ? ((oth & 0xffffu) | (x0 & 0xffff0000u)) : ((x0 & 0xffffu) | (oth << 16));
                vt[1] = odd ? ((oth >> 16) | (x1 & 0xffff0000u)) : ((x1 & 0xffffu) | (oth & 0xffff0000u));
                // slots 32 (w >> 1) + 8 tg + 4 (w & 1) .. + 3 = half (w & 1) of chunk 4 (w >> 1) + tg of row 16 s + 4 kq + c
                const int row = 16 * s + 4 * kq + c;
                *reinterpret_cast<wb_u2*>(Vt + row * WT + 8 * ((4 * (w >> 1) + tg) ^ vt_swz(row)) + 4 * (w & 1)) = vt;
            }
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
                f32x4 st = zero;
                const int row = 16 * kt + tok;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const int ch = DH > 16 ? 4 * s + kq : (kq & 1);
                    const wb_b8 kf = *reinterpret_cast<const wb_b8*>(Ks + row * DH + 8 * (ch ^ ks_swz<DH>(row)));
                    st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], st, 0, 0, 0);
                }
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
            mt = fmaxf(mt, __shfl_xor(mt, 16)); mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float mn = fmaxf(m, mt);
            const float alpha = expf(m - mn);               // (first tile: exp(-huge) = 0 onto l = 0, o = 0)
            float ls = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { pr[kt][r] = pr[kt][r] > -FLT_MAX ? expf(pr[kt][r] - mn) : 0.f; ls += pr[kt][r]; }
            ls += __shfl_xor(ls, 16); ls += __shfl_xor(ls, 32);
            l = l * alpha + ls;                              // (the row sum takes the unrounded p)
            m = mn;
            // the accumulator's rows are queries 4 kq + r: their rescale sits on lane 4 kq + r
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ar = __shfl(alpha, 4 * kq + r);
#pragma unroll
                for (int s = 0; s < NS; ++s) o[s][r] *= ar;
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (j0 + 32 * u > jmax) continue;           // (a skipped second sub-tile of a half has p = 0)
                wb_b8 pa;                                   // A fragment: slot 8 kq + e <-> key 4 kq + e of sub-tile 2 u, slot 8 kq + 4 + e of 2 u + 1
#pragma unroll
                for (int e = 0; e < 4; ++e) { pa[e] = (__bf16)pr[2 * u][e]; pa[4 + e] = (__bf16)pr[2 * u + 1][e]; }
#pragma unroll
                for (int t = 0; t < NS; ++t) {
                    const int row = 16 * t + tok;
                    const wb_b8 vf = *reinterpret_cast<const wb_b8*>(Vt + row * WT + 8 * ((4 * u + kq) ^ vt_swz(row)));
                    o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vf, o[t], 0, 0, 0);
                }
            }
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
        float* orow = p.out + g * p.o_group_stride + (int64_t)qi * p.o_item_stride + h * DH + tok;
#pragma unroll
        for (int s = 0; s < NS; ++s) orow[16 * s] = on[s] * gt;
    }
}

}  // namespace

// Launches on arguments wide_attn (attn_wide_mfma.hip) has validated; *form names the kernel that ran.  `out_b` is left to small_attn's conversion pass.
int wide_attn_bf16_launch(const SmallAttnArgs& p, hipStream_t stream, const char** form) {
    const dim3 grid((unsigned)((int64_t)p.groups * p.heads), (unsigned)cdiv(p.nq, 64)), block(256);
    if (p.dh == 64) { *form = "wide_attn_bf16_kernel<64>"; hipLaunchKernelGGL(wide_attn_bf16_kernel<64>, grid, block, 0, stream, p); }
    else if (p.dh == 32) { *form = "wide_attn_bf16_kernel<32>"; hipLaunchKernelGGL(wide_attn_bf16_kernel<32>, grid, block, 0, stream, p); }
    else { *form = "wide_attn_bf16_kernel<16>"; hipLaunchKernelGGL(wide_attn_bf16_kernel<16>, grid, block, 0, stream, p); }
    D4_LAUNCH_CHECK();
    return 0;
}

}  // namespace d4
