// Tiled (flash-style) attention core of the training path: the semantics of backward.hip's attn_bwd_kernel (rotary on q and on the
// normalised, scaled key; key RMS-norm with (gamma + 1) sqrt(dh); value-residual mix; softclamp; mask; belief projection; head gate) and
// of its xattn_bwd_kernel, for up to ATT_MAX_FRAMES items per problem side, with memory linear in the items.  One set of kernels, three
// geometries (the template argument GEO picks the visibility rule and which per-row features exist):
//   GEO_TIME   the time layers: causal (j <= i), rotary, value residual, belief
//   GEO_FRAME  within a frame: no rotary; query i sees key j unless i is ordinary and j special (the last num_special items); value
//              residual, belief (a runtime flag)
//   GEO_CROSS  nq queries over nk keys from separate projection buffers (keys group major or item major): no mask, no value residual, no belief
//
// Six kernels over per-row planes ([group * heads + head][item][DH], so a (group, head) problem is contiguous whatever the row geometry;
// query-side planes hold nq rows per problem, key-side planes nk; the frames / keys below are the time geometry's, the other two differ
// only in the bounds sees() / last_key() / first_query() give):
//   pre    one wave per (row, head): phase A of attn_bwd_kernel written to the planes (rotated q, normalised / scaled / rotated k, unrotated
//          normalised k, mixed v, 1/|k|, 1/|v|, mix and gate sigmoids)
//   fwd    one wave per 16 queries (a block = a 64-query tile) walks the keys <= its last query, 64 at a time, with an online softmax;
//          writes the pre-belief output o, the row's log-sum-exp, and o3
//   dprep  one wave per (row, head): gate and belief backward -> dO, the direct value gradient, the gate logit's gradient, dO . o
//   dq     one wave per 16 queries walks the keys <= its own: P recomputed from the log-sum-exp, dS, dQ = dS K
//   dkv    one wave per 16 keys walks the queries >= its own: dV = P^T dO, dK = dS^T Q
//   post   one block per (group, head): phase C of attn_bwd_kernel (transposed rotary, key-norm backward, value-mix backward, d gamma partial)
//
// All six products run on v_mfma_f32_16x16x4_f32.  Register r of lane l of a 16x16 accumulator holds row 4 (l >> 4) + r, column l & 15, and
// an A operand wants row l & 15, contraction index l >> 4.  So a product is always computed with the index the NEXT product contracts over on
// the accumulator's ROW side: fwd / dq compute S^T-tiles (rows = keys) and feed P / dS as the A operand of P V / dS K; dkv computes S-tiles
// (rows = queries) and feeds P / dS as the A operand of P^T dO / dS^T Q.  The contraction then runs in the order 4 (l >> 4) + e on both
// operands (a fixed permutation), and no score ever goes through LDS.  The kernels use no LDS and no barrier: a wave is independent.
//
// Deterministic: no atomics, every sum in a fixed order.  Rows past `frames` of the last tile are never addressed (loads give zero, stores skip).
//
// The geometries, the argument block, the planes and the three per-row kernels (pre, dprep, post) live in attn_tiled_rows.h, which this file shares
// with attn_tiled_bf16.hip (the same core with its six products on the bf16 matrix pipe, an opt-in); this file instantiates them in their fp32 form.
#define D4_ATTN_TILED_FORM_FILE
#include "attn_tiled_rows.h"

namespace d4 {

int g_time_attn_tiled = 0;
int g_space_attn_tiled = 0;
int g_cross_attn_tiled = 0;

namespace {

// operand row `row` of a [T][DH] plane as DH / 16 float4s: features 16 s + 4 kq .. + 3 (zero past the last row)
template <int NS>
__device__ __forceinline__ void load_rows(f32x4 (&dst)[NS], const float* plane, int row, int T, int kq) {
    constexpr int DH = 16 * NS;
#pragma unroll
    for (int s = 0; s < NS; ++s)
        dst[s] = row < T ? *reinterpret_cast<const f32x4*>(plane + (int64_t)row * DH + 16 * s + 4 * kq) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// C[m][n] = sum_feature A[m][.] B[n][.]: both operands as load_rows gives them (A rows on l & 15, B rows on l & 15)
template <int NS>
__device__ __forceinline__ f32x4 dot_tile(const f32x4 (&a)[NS], const f32x4 (&b)[NS]) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][e], b[s][e], c, 0, 0, 0);
    return c;
}

// acc[t] += A B with A[m = l & 15][k -> row r0 + 4 kq + e] = a[e] and B rows r0 + 4 kq + e of a [T][DH] plane (columns 16 t + (l & 15))
template <int NS>
__device__ __forceinline__ void acc_rows(f32x4 (&acc)[NS], const f32x4& a, const float* plane, int r0, int T, int kq, int tok) {
    constexpr int DH = 16 * NS;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int row = r0 + 4 * kq + e;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const float b = row < T ? plane[(int64_t)row * DH + 16 * t + tok] : 0.f;
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b, acc[t], 0, 0, 0);
        }
    }
}

// ---- forward: grid (G * heads, ceil(nq / 64)); wave w of a block owns queries 64 blockIdx.y + 16 w .. + 15
// Every query sees key 0 in all three geometries (an ordinary key unless every item is special, and then every query is special), so the
// running maximum is finite after the first 64 keys; a later tile that is all masked for a row leaves that row's m, l and o as they are
// (its scores are -FLT_MAX, which the exponential step turns into exact zeros).
template <int DH, int GEO>
__global__ __launch_bounds__(256) void tiled_fwd_kernel(TiledArgs p, TiledPlanes t) {
    constexpr int NS = DH / 16;
    const int nq = p.nq, nk = p.nk, hd = p.heads * DH, fs = nk - p.num_special;
    const int gh = blockIdx.x, f = gh / p.heads, h = gh % p.heads;
    const int lane = threadIdx.x & 63, tok = lane & 15, kq = lane >> 4;
    const int i0 = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (i0 >= nq) return;
    const int64_t pbq = (int64_t)gh * nq * DH, sbq = (int64_t)gh * nq, pbk = (int64_t)gh * nk * DH, sbk = (int64_t)gh * nk;
    const float *Q = t.qr + pbq, *K = t.kn + pbk, *V = t.vm + pbk;
    const float scale = rsqrtf((float)DH);
    const int i = i0 + tok;
    const int jmax = last_key<GEO>(i0, nk, fs);                       // the last key any query of this wave sees
    f32x4 q4[NS], o[NS];
    load_rows<NS>(q4, Q, i, nq, kq);
#pragma unroll
    for (int s = 0; s < NS; ++s) o[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -FLT_MAX, l = 0.f;
    for (int j0 = 0; j0 <= jmax; j0 += 64) {
        // scores of 64 keys, transposed tiles: pr[kt][r] = S[i][j0 + 16 kt + 4 kq + r]
        f32x4 pr[4];
        float mt = -FLT_MAX;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int jb = j0 + 16 * kt;
            pr[kt] = f32x4{-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
            if (jb > jmax) continue;                                   // (wave-uniform)
            f32x4 k4[NS];
            load_rows<NS>(k4, K, jb + tok, nk, kq);
            const f32x4 st = dot_tile<NS>(k4, q4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = jb + 4 * kq + r;
                float simc = st[r] * scale;
                if (p.softclamp > 0.f) simc = tanhf(simc / p.softclamp) * p.softclamp;
                pr[kt][r] = sees<GEO>(i, j, nk, fs) ? simc : -FLT_MAX;
                mt = fmaxf(mt, pr[kt][r]);
            }
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16)); mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);
        const float alpha = expf(m - mn);                              // (first tile: exp(-huge) = 0 onto l = 0, o = 0)
        float ls = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { pr[kt][r] = pr[kt][r] > -FLT_MAX ? expf(pr[kt][r] - mn) : 0.f; ls += pr[kt][r]; }
        ls += __shfl_xor(ls, 16); ls += __shfl_xor(ls, 32);
        l = l * alpha + ls;
        m = mn;
        // the accumulator's rows are queries 4 kq + r: their rescale sits on lane 4 kq + r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ar = __shfl(alpha, 4 * kq + r);
#pragma unroll
            for (int s = 0; s < NS; ++s) o[s][r] *= ar;
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int jb = j0 + 16 * kt;
            if (jb > jmax) continue;
            acc_rows<NS>(o, pr[kt], V, jb, nk, kq, tok);
        }
    }
    const float lse = m + logf(l), linv = 1.f / l;
    float lse_r[4], linv_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { lse_r[r] = __shfl(lse, 4 * kq + r); linv_r[r] = __shfl(linv, 4 * kq + r); }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = i0 + 4 * kq + r;
        if (qi >= nq) continue;                                        // (uniform over each 16-lane row group)
        float on_[NS], vn[NS], dot = 0.f;
        const float vinv = GEO == GEO_CROSS ? 0.f : t.vinv[sbk + qi];   // (belief: the query's own value row; the cross geometry has neither)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            on_[s] = o[s][r] * linv_r[r];
            t.o[pbq + (int64_t)qi * DH + 16 * s + tok] = on_[s];
            vn[s] = GEO == GEO_CROSS ? 0.f : V[(int64_t)qi * DH + 16 * s + tok] * vinv;
            dot = __builtin_fmaf(on_[s], vn[s], dot);
        }
        dot = (GEO != GEO_CROSS && p.belief) ? row_sum16(dot) : 0.f;
        if (tok == 0) t.lse[sbq + qi] = lse_r[r];
        const float gt = t.gt[sbq + qi];
        float* orow = p.o3 + row_of(p.qm, f, qi) * hd + h * DH;
#pragma unroll
        for (int s = 0; s < NS; ++s) orow[16 * s + tok] = (on_[s] - dot * vn[s]) * gt;
    }
}

// ---- dQ: grid (G * heads, ceil(nq / 64)); wave w owns queries 64 blockIdx.y + 16 w .. + 15 and walks the key tiles up to the last it sees
template <int DH, int GEO>
__global__ __launch_bounds__(256) void tiled_dq_kernel(TiledArgs p, TiledPlanes t) {
    constexpr int NS = DH / 16;
    const int nq = p.nq, nk = p.nk, fs = nk - p.num_special;
    const int gh = blockIdx.x;
    const int lane = threadIdx.x & 63, tok = lane & 15, kq = lane >> 4;
    const int i0 = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (i0 >= nq) return;
    const int64_t pbq = (int64_t)gh * nq * DH, sbq = (int64_t)gh * nq, pbk = (int64_t)gh * nk * DH;
    const float *Q = t.qr + pbq, *K = t.kn + pbk, *V = t.vm + pbk, *DO = t.dO + pbq;
    const float scale = rsqrtf((float)DH);
    const int i = i0 + tok;
    const int jmax = last_key<GEO>(i0, nk, fs);
    f32x4 q4[NS], do4[NS], dq[NS];
    load_rows<NS>(q4, Q, i, nq, kq);
    load_rows<NS>(do4, DO, i, nq, kq);
#pragma unroll
    for (int s = 0; s < NS; ++s) dq[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float lse = i < nq ? t.lse[sbq + i] : 0.f, delta = i < nq ? t.delta[sbq + i] : 0.f;
    for (int jb = 0; jb <= jmax; jb += 16) {
        f32x4 k4[NS], v4[NS];
        load_rows<NS>(k4, K, jb + tok, nk, kq);
        load_rows<NS>(v4, V, jb + tok, nk, kq);
        const f32x4 st = dot_tile<NS>(k4, q4);                         // st[r] = q_i . k_j, j = jb + 4 kq + r
        const f32x4 dpt = dot_tile<NS>(v4, do4);                       // dO_i . v_j
        f32x4 ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = jb + 4 * kq + r;
            float pij, d;
            p_and_ds(st[r], dpt[r], lse, delta, sees<GEO>(i, j, nk, fs) && i < nq, scale, p.softclamp, pij, d);
            ds[r] = d;
        }
        acc_rows<NS>(dq, ds, K, jb, nk, kq, tok);                      // dq_i += sum_j dS_ij k_j
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = i0 + 4 * kq + r;
        if (qi >= nq) continue;
#pragma unroll
        for (int s = 0; s < NS; ++s) t.dq[pbq + (int64_t)qi * DH + 16 * s + tok] = dq[s][r];
    }
}

// ---- dK / dV: grid (G * heads, ceil(nk / 64)); wave w owns keys 64 blockIdx.y + 16 w .. + 15 and walks the query tiles from the first that sees one
template <int DH, int GEO>
__global__ __launch_bounds__(256) void tiled_dkv_kernel(TiledArgs p, TiledPlanes t) {
    constexpr int NS = DH / 16;
    const int nq = p.nq, nk = p.nk, fs = nk - p.num_special;
    const int gh = blockIdx.x;
    const int lane = threadIdx.x & 63, tok = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (j0 >= nk) return;
    const int64_t pbq = (int64_t)gh * nq * DH, sbq = (int64_t)gh * nq, pbk = (int64_t)gh * nk * DH;
    const float *Q = t.qr + pbq, *K = t.kn + pbk, *V = t.vm + pbk, *DO = t.dO + pbq;
    const float scale = rsqrtf((float)DH);
    const int j = j0 + tok;
    f32x4 k4[NS], v4[NS], dk[NS], dv[NS];
    load_rows<NS>(k4, K, j, nk, kq);
    load_rows<NS>(v4, V, j, nk, kq);
#pragma unroll
    for (int s = 0; s < NS; ++s) { dk[s] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[s] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int ib = first_query<GEO>(j0, fs); ib < nq; ib += 16) {
        f32x4 q4[NS], do4[NS];
        load_rows<NS>(q4, Q, ib + tok, nq, kq);
        load_rows<NS>(do4, DO, ib + tok, nq, kq);
        const f32x4 st = dot_tile<NS>(q4, k4);                         // st[r] = q_i . k_j, i = ib + 4 kq + r
        const f32x4 dpt = dot_tile<NS>(do4, v4);
        f32x4 pt, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ib + 4 * kq + r;
            const bool in = i < nq;
            const float lse = in ? t.lse[sbq + i] : 0.f, delta = in ? t.delta[sbq + i] : 0.f;
            float pij, d;
            p_and_ds(st[r], dpt[r], lse, delta, in && sees<GEO>(i, j, nk, fs), scale, p.softclamp, pij, d);
            pt[r] = pij; ds[r] = d;
        }
        acc_rows<NS>(dv, pt, DO, ib, nq, kq, tok);                     // dv_j += sum_i P_ij dO_i
        acc_rows<NS>(dk, ds, Q, ib, nq, kq, tok);                      // dk_j += sum_i dS_ij q_i
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int kj = j0 + 4 * kq + r;
        if (kj >= nk) continue;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            t.dkn[pbk + (int64_t)kj * DH + 16 * s + tok] = dk[s][r];
            t.dv[pbk + (int64_t)kj * DH + 16 * s + tok] = dv[s][r];
        }
    }
}

template <int DH, int GEO>
int launch_tiled(const TiledArgs& a, const TiledPlanes& t, hipStream_t s) {
    const int nmax = a.nq > a.nk ? a.nq : a.nk, gh = a.G * a.heads;
    const dim3 block(256), rows(gh, (nmax + 3) / 4), qrows(gh, (a.nq + 3) / 4), qtiles(gh, (a.nq + 63) / 64), ktiles(gh, (a.nk + 63) / 64);
    hipLaunchKernelGGL((tiled_pre_kernel<DH, GEO, false>), rows, block, 0, s, a, t);
    hipLaunchKernelGGL((tiled_fwd_kernel<DH, GEO>), qtiles, block, 0, s, a, t);
    D4_LAUNCH_CHECK();
    if (!a.d_o3) return 0;
    hipLaunchKernelGGL((tiled_dprep_kernel<DH, GEO, false>), qrows, block, 0, s, a, t);
    hipLaunchKernelGGL((tiled_dq_kernel<DH, GEO>), qtiles, block, 0, s, a, t);
    hipLaunchKernelGGL((tiled_dkv_kernel<DH, GEO>), ktiles, block, 0, s, a, t);
    hipLaunchKernelGGL((tiled_post_kernel<DH, GEO>), dim3(gh), block, 0, s, a, t);
    D4_LAUNCH_CHECK();
    return 0;
}

template <int GEO>
int launch_dh(const TiledArgs& a, int dh, float* planes, hipStream_t s) {
    if (int rc = check_tiled(a, dh, planes)) return rc;
    if (a.G * a.heads == 0) return 0;
    TiledPlanes t{};
    carve(t, planes, (size_t)a.G * a.nq, (size_t)a.G * a.nk, a.heads, dh, GEO == GEO_CROSS);
#define D4_TILED_FORM(DH_) (GEO == GEO_TIME ? "tiled<time," #DH_ ">" : GEO == GEO_FRAME ? "tiled<frame," #DH_ ">" : "tiled<cross," #DH_ ">")
    if (dh == 64) { note_train_form(GEO == GEO_CROSS, D4_TILED_FORM(64)); return launch_tiled<64, GEO>(a, t, s); }
    if (dh == 32) { note_train_form(GEO == GEO_CROSS, D4_TILED_FORM(32)); return launch_tiled<32, GEO>(a, t, s); }
    note_train_form(GEO == GEO_CROSS, D4_TILED_FORM(16));
#undef D4_TILED_FORM
    return launch_tiled<16, GEO>(a, t, s);
}

}  // namespace

size_t attn_tiled_floats(int R, int heads, int dh) { TiledPlanes t{}; return carve(t, nullptr, R, R, heads, dh, false); }
size_t attn_tiled_cross_floats(int Rq, int Rk, int heads, int dh) { TiledPlanes t{}; return carve(t, nullptr, Rq, Rk, heads, dh, true); }

int attn_tiled_core(const AttnBwdArgs& a, int dh, float* planes, hipStream_t s) {
    const bool time = a.causal && a.inv_freq;
    if (int rc = check_self_geometry(a)) return rc;
    const TiledArgs p = tiled_args(a, dh);
    return time ? launch_dh<GEO_TIME>(p, dh, planes, s) : launch_dh<GEO_FRAME>(p, dh, planes, s);
}

int attn_tiled_cross_core(const XAttnArgs& a, int dh, float* planes, hipStream_t s) {
    return launch_dh<GEO_CROSS>(tiled_args(a, dh), dh, planes, s);
}

}  // namespace d4
