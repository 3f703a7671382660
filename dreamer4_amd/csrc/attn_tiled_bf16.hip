// Tiled attention core of the training path with its six products on the bf16 matrix pipe (opt-in: d4_train_attn_products_set(1)):
// the structure, geometries, grids and outputs of attn_tiled.hip (pre, fwd, dprep, dq, dkv, post; one wave per 16 rows, no LDS, no atomics,
// every sum in a fixed order), with v_mfma_f32_16x16x32_bf16 in place of v_mfma_f32_16x16x4_f32.
//
// Arithmetic.  pre, dprep and post are attn_tiled_rows.h's fp32 kernels; pre and dprep also write bf16 images (round to nearest even) of the
// rotated q, of k', of the mixed v and of dO.  S = q^ k^'^T and dP = dO^ v^^T take the row-major images with fp32 accumulate; scale, soft clamp,
// visibility, the online softmax per 64 keys, lse, P = exp(s - lse) and dS = P (dP - delta) (1 - tanh^2) scale are fp32; p (forward), P and dS
// (backward) are rounded to bf16 as the A operands of p^ v^, P^^T dO^, dS^ k^' and dS^^T q^ (fp32 accumulate), whose B operands come from the
// transposed images.  The forward's row sum takes the unrounded p; the belief projection the query's own fp32 v row; delta = dO^ . o.
//
// Orientation.  The C / D layout of the 16x16x32 bf16 MFMA is the f32 form's (register r of lane l: row 4 (l >> 4) + r, column l & 15), and
// its A / B operands hold contraction index 8 (l >> 4) + j in element j of lane l (row / column l & 15).  So, as in attn_tiled.hip, every score
// tile is computed with the index the next product contracts over on the accumulator's row side, and the eight registers of two adjacent
// 16-row sub-tiles of a lane, packed pairwise, ARE the A fragment of that product over 32 items, in the slot order
//     slot 8 kq + j  <->  item 16 (j >> 2) + 4 kq + (j & 3)            (kq = l >> 4)
// The B operand presents the same order from a transposed image [feature][item]: two aligned 8-byte loads per lane, items r0 + 4 kq .. + 3 and
// r0 + 16 + 4 kq .. + 3 of feature 16 t + (l & 15).  fwd keeps its 64-key step (two such halves); dq and dkv walk 32 items per step.  A
// sub-tile beyond the last key (dq) contributes exact zeros; dkv starts its walk at a multiple of 32 so that a step never leaves the padded
// image (the queries it adds below first_query see none of the wave's keys: exact zeros).  Head dim 16 zero-pads the 32-deep contraction of
// the score products: the lanes kq >= 2 carry zero fragments on both sides.
//
// Every element of every image is written before it is read: rows < items by pre / dprep, the pad columns of the transposed images as zeros
// by the same kernels; rows past the last item of the row-major images are never loaded (the fragment is zero).
#define D4_ATTN_TILED_FORM_FILE
#include "attn_tiled_rows.h"

namespace d4 {

namespace {

typedef __bf16 tb_b8 __attribute__((ext_vector_type(8)));

// bf16 elements of the images behind the carve-up (each image rounded up to 128 elements = 256 bytes); base null: the size only
size_t carve_images(TiledPlanes& t, uint16_t* base, size_t G, int nq, int nk, int heads, int dh) {
    size_t off = 0;
    auto take = [&](size_t n) { uint16_t* p = base ? base + off : nullptr; off += (n + 127) / 128 * 128; return p; };
    t.nqp = (nq + 31) / 32 * 32; t.nkp = (nk + 31) / 32 * 32;
    const size_t gh = G * heads;
    t.qb = take(gh * nq * dh); t.dob = take(gh * nq * dh); t.kb = take(gh * nk * dh); t.vb = take(gh * nk * dh);
    t.qt = take(gh * dh * t.nqp); t.dot = take(gh * dh * t.nqp); t.kt = take(gh * dh * t.nkp); t.vt = take(gh * dh * t.nkp);
    return off;
}

// score-type fragments of row `row` of a row-major image [n][DH]: features 32 s + 8 kq .. + 7 (zero past the last row; DH 16: zero for kq >= 2)
template <int DH>
struct RowFrag { tb_b8 f[DH == 64 ? 2 : 1]; };
template <int DH>
__device__ __forceinline__ void load_frag(RowFrag<DH>& d, const uint16_t* img, int row, int n, int kq) {
    constexpr int KS = DH == 64 ? 2 : 1;
    const bool ok = row < n && (DH > 16 || kq < 2);
    const uint16_t* src = img + (int64_t)row * DH + (DH > 16 ? 8 * kq : 8 * (kq & 1));
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const f32x4 raw = ok ? *reinterpret_cast<const f32x4*>(src + 32 * s) : f32x4{0.f, 0.f, 0.f, 0.f};
        d.f[s] = __builtin_bit_cast(tb_b8, raw);
    }
}
// C[m][n] = sum_feature A[m][.] B[n][.]
template <int DH>
__device__ __forceinline__ f32x4 dot_frag(const RowFrag<DH>& a, const RowFrag<DH>& b) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < (DH == 64 ? 2 : 1); ++s) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.f[s], b.f[s], c, 0, 0, 0);
    return c;
}
// the A fragment of two adjacent accumulator sub-tiles (see "Orientation")
__device__ __forceinline__ tb_b8 pack_pair(const f32x4& lo, const f32x4& hi) {
    tb_b8 a;
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] = (__bf16)lo[e]; a[4 + e] = (__bf16)hi[e]; }
    return a;
}
// acc[t] += A B over the items r0 .. r0 + 31 of a transposed image [DH][np] (r0 a multiple of 16 with r0 + 32 <= np): column 16 t + tok
template <int NS>
__device__ __forceinline__ void acc_items(f32x4 (&acc)[NS], const tb_b8& a, const uint16_t* timg, int np, int r0, int kq, int tok) {
    typedef float tb_f2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const uint16_t* src = timg + (int64_t)(16 * t + tok) * np + r0 + 4 * kq;
        const tb_f2 lo = *reinterpret_cast<const tb_f2*>(src), hi = *reinterpret_cast<const tb_f2*>(src + 16);
        const f32x4 raw = {lo[0], lo[1], hi[0], hi[1]};
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(tb_b8, raw), acc[t], 0, 0, 0);
    }
}

// ---- forward: grid (G * heads, ceil(nq / 64)); wave w of a block owns queries 64 blockIdx.y + 16 w .. + 15  (attn_tiled.hip's tiled_fwd_kernel)
template <int DH, int GEO>
__global__ __launch_bounds__(256) void tiled_bf16_fwd_kernel(TiledArgs p, TiledPlanes t) {
    constexpr int NS = DH / 16;
    const int nq = p.nq, nk = p.nk, hd = p.heads * DH, fs = nk - p.num_special;
    const int gh = blockIdx.x, f = gh / p.heads, h = gh % p.heads;
    const int lane = threadIdx.x & 63, tok = lane & 15, kq = lane >> 4;
    const int i0 = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (i0 >= nq) return;
    const int64_t pbq = (int64_t)gh * nq * DH, sbq = (int64_t)gh * nq, pbk = (int64_t)gh * nk * DH, sbk = (int64_t)gh * nk;
    const uint16_t *Q = t.qb + pbq, *K = t.kb + pbk, *VT = t.vt + (int64_t)gh * DH * t.nkp;
    const float* V = t.vm + pbk;
    const float scale = rsqrtf((float)DH);
    const int i = i0 + tok;
    const int jmax = last_key<GEO>(i0, nk, fs);
    RowFrag<DH> qf;
    load_frag<DH>(qf, Q, i, nq, kq);
    f32x4 o[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) o[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -FLT_MAX, l = 0.f;
    for (int j0 = 0; j0 <= jmax; j0 += 64) {
        f32x4 pr[4];
        float mt = -FLT_MAX;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int jb = j0 + 16 * kt;
            pr[kt] = f32x4{-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
            if (jb > jmax) continue;                                   // (wave-uniform)
            RowFrag<DH> kf;
            load_frag<DH>(kf, K, jb + tok, nk, kq);
            const f32x4 st = dot_frag<DH>(kf, qf);
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
        const float alpha = expf(m - mn);
        float ls = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { pr[kt][r] = pr[kt][r] > -FLT_MAX ? expf(pr[kt][r] - mn) : 0.f; ls += pr[kt][r]; }
        ls += __shfl_xor(ls, 16); ls += __shfl_xor(ls, 32);
        l = l * alpha + ls;
        m = mn;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ar = __shfl(alpha, 4 * kq + r);
#pragma unroll
            for (int s = 0; s < NS; ++s) o[s][r] *= ar;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (j0 + 32 * u > jmax) continue;                          // (a skipped second sub-tile of a half has p = 0)
            acc_items<NS>(o, pack_pair(pr[2 * u], pr[2 * u + 1]), VT, t.nkp, j0 + 32 * u, kq, tok);
        }
    }
    const float lse = m + logf(l), linv = 1.f / l;
    float lse_r[4], linv_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { lse_r[r] = __shfl(lse, 4 * kq + r); linv_r[r] = __shfl(linv, 4 * kq + r); }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = i0 + 4 * kq + r;
        if (qi >= nq) continue;
        float on_[NS], vn[NS], dot = 0.f;
        const float vinv = GEO == GEO_CROSS ? 0.f : t.vinv[sbk + qi];
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

// ---- dQ: grid (G * heads, ceil(nq / 64)); a wave owns 16 queries and walks the keys up to the last it sees, 32 at a time
template <int DH, int GEO>
__global__ __launch_bounds__(256) void tiled_bf16_dq_kernel(TiledArgs p, TiledPlanes t) {
    constexpr int NS = DH / 16;
    const int nq = p.nq, nk = p.nk, fs = nk - p.num_special;
    const int gh = blockIdx.x;
    const int lane = threadIdx.x & 63, tok = lane & 15, kq = lane >> 4;
    const int i0 = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (i0 >= nq) return;
    const int64_t pbq = (int64_t)gh * nq * DH, sbq = (int64_t)gh * nq, pbk = (int64_t)gh * nk * DH;
    const uint16_t *Q = t.qb + pbq, *DO = t.dob + pbq, *K = t.kb + pbk, *V = t.vb + pbk, *KT = t.kt + (int64_t)gh * DH * t.nkp;
    const float scale = rsqrtf((float)DH);
    const int i = i0 + tok;
    const int jmax = last_key<GEO>(i0, nk, fs);
    RowFrag<DH> qf, dof;
    load_frag<DH>(qf, Q, i, nq, kq);
    load_frag<DH>(dof, DO, i, nq, kq);
    f32x4 dq[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) dq[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float lse = i < nq ? t.lse[sbq + i] : 0.f, delta = i < nq ? t.delta[sbq + i] : 0.f;
    for (int jb = 0; jb <= jmax; jb += 32) {
        f32x4 ds[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            ds[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (jb + 16 * u > jmax) continue;                          // (wave-uniform)
            RowFrag<DH> kf, vf;
            load_frag<DH>(kf, K, jb + 16 * u + tok, nk, kq);
            load_frag<DH>(vf, V, jb + 16 * u + tok, nk, kq);
            const f32x4 st = dot_frag<DH>(kf, qf);                     // st[r] = q_i . k_j, j = jb + 16 u + 4 kq + r
            const f32x4 dpt = dot_frag<DH>(vf, dof);                   // dO_i . v_j
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = jb + 16 * u + 4 * kq + r;
                float pij, d;
                p_and_ds(st[r], dpt[r], lse, delta, sees<GEO>(i, j, nk, fs) && i < nq, scale, p.softclamp, pij, d);
                ds[u][r] = d;
            }
        }
        acc_items<NS>(dq, pack_pair(ds[0], ds[1]), KT, t.nkp, jb, kq, tok);    // dq_i += sum_j dS_ij k_j
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = i0 + 4 * kq + r;
        if (qi >= nq) continue;
#pragma unroll
        for (int s = 0; s < NS; ++s) t.dq[pbq + (int64_t)qi * DH + 16 * s + tok] = dq[s][r];
    }
}

// ---- dK / dV: grid (G * heads, ceil(nk / 64)); a wave owns 16 keys and walks the queries from the first that sees one (rounded down to 32), 32 at a time
template <int DH, int GEO>
__global__ __launch_bounds__(256) void tiled_bf16_dkv_kernel(TiledArgs p, TiledPlanes t) {
    constexpr int NS = DH / 16;
    const int nq = p.nq, nk = p.nk, fs = nk - p.num_special;
    const int gh = blockIdx.x;
    const int lane = threadIdx.x & 63, tok = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (j0 >= nk) return;
    const int64_t pbq = (int64_t)gh * nq * DH, sbq = (int64_t)gh * nq, pbk = (int64_t)gh * nk * DH, tbq = (int64_t)gh * DH * t.nqp;
    const uint16_t *Q = t.qb + pbq, *DO = t.dob + pbq, *K = t.kb + pbk, *V = t.vb + pbk, *QT = t.qt + tbq, *DOT = t.dot + tbq;
    const float scale = rsqrtf((float)DH);
    const int j = j0 + tok;
    RowFrag<DH> kf, vf;
    load_frag<DH>(kf, K, j, nk, kq);
    load_frag<DH>(vf, V, j, nk, kq);
    f32x4 dk[NS], dv[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) { dk[s] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[s] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int ib = first_query<GEO>(j0, fs) & ~31; ib < nq; ib += 32) {
        f32x4 pt[2], ds[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            pt[u] = f32x4{0.f, 0.f, 0.f, 0.f}; ds[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ib + 16 * u >= nq) continue;                           // (wave-uniform)
            RowFrag<DH> qf, dof;
            load_frag<DH>(qf, Q, ib + 16 * u + tok, nq, kq);
            load_frag<DH>(dof, DO, ib + 16 * u + tok, nq, kq);
            const f32x4 st = dot_frag<DH>(qf, kf);                     // st[r] = q_i . k_j, i = ib + 16 u + 4 kq + r
            const f32x4 dpt = dot_frag<DH>(dof, vf);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ib + 16 * u + 4 * kq + r;
                const bool in = i < nq;
                const float lse = in ? t.lse[sbq + i] : 0.f, delta = in ? t.delta[sbq + i] : 0.f;
                float pij, d;
                p_and_ds(st[r], dpt[r], lse, delta, in && sees<GEO>(i, j, nk, fs), scale, p.softclamp, pij, d);
                pt[u][r] = pij; ds[u][r] = d;
            }
        }
        acc_items<NS>(dv, pack_pair(pt[0], pt[1]), DOT, t.nqp, ib, kq, tok);   // dv_j += sum_i P_ij dO_i
        acc_items<NS>(dk, pack_pair(ds[0], ds[1]), QT, t.nqp, ib, kq, tok);    // dk_j += sum_i dS_ij q_i
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
int launch_tiled_bf16(const TiledArgs& a, const TiledPlanes& t, hipStream_t s) {
    const int npmax = t.nqp > t.nkp ? t.nqp : t.nkp, gh = a.G * a.heads;
    const dim3 block(256), rows(gh, npmax / 4), qrows(gh, t.nqp / 4), qtiles(gh, (a.nq + 63) / 64), ktiles(gh, (a.nk + 63) / 64);
    hipLaunchKernelGGL((tiled_pre_kernel<DH, GEO, true>), rows, block, 0, s, a, t);
    hipLaunchKernelGGL((tiled_bf16_fwd_kernel<DH, GEO>), qtiles, block, 0, s, a, t);
    D4_LAUNCH_CHECK();
    if (!a.d_o3) return 0;
    hipLaunchKernelGGL((tiled_dprep_kernel<DH, GEO, true>), qrows, block, 0, s, a, t);
    hipLaunchKernelGGL((tiled_bf16_dq_kernel<DH, GEO>), qtiles, block, 0, s, a, t);
    hipLaunchKernelGGL((tiled_bf16_dkv_kernel<DH, GEO>), ktiles, block, 0, s, a, t);
    hipLaunchKernelGGL((tiled_post_kernel<DH, GEO>), dim3(gh), block, 0, s, a, t);
    D4_LAUNCH_CHECK();
    return 0;
}

template <int GEO>
int launch_dh_bf16(const TiledArgs& a, int dh, float* planes, hipStream_t s) {
    if (int rc = check_tiled(a, dh, planes)) return rc;
    if (a.G * a.heads == 0) return 0;
    TiledPlanes t{};
    const size_t off = carve(t, planes, (size_t)a.G * a.nq, (size_t)a.G * a.nk, a.heads, dh, GEO == GEO_CROSS);
    carve_images(t, reinterpret_cast<uint16_t*>(planes + off), a.G, a.nq, a.nk, a.heads, dh);
#define D4_TILED_FORM(DH_) (GEO == GEO_TIME ? "tiled_bf16<time," #DH_ ">" : GEO == GEO_FRAME ? "tiled_bf16<frame," #DH_ ">" : "tiled_bf16<cross," #DH_ ">")
    if (dh == 64) { note_train_bf16_form(GEO == GEO_CROSS, D4_TILED_FORM(64)); return launch_tiled_bf16<64, GEO>(a, t, s); }
    if (dh == 32) { note_train_bf16_form(GEO == GEO_CROSS, D4_TILED_FORM(32)); return launch_tiled_bf16<32, GEO>(a, t, s); }
    note_train_bf16_form(GEO == GEO_CROSS, D4_TILED_FORM(16));
#undef D4_TILED_FORM
    return launch_tiled_bf16<16, GEO>(a, t, s);
}

size_t total_floats(size_t G, int nq, int nk, int heads, int dh, bool cross) {
    TiledPlanes t{};
    return carve(t, nullptr, G * nq, G * nk, heads, dh, cross) + (carve_images(t, nullptr, G, nq, nk, heads, dh) + 1) / 2;
}

}  // namespace

size_t attn_tiled_bf16_floats(int groups, int items, int heads, int dh) { return total_floats(groups, items, items, heads, dh, false); }
size_t attn_tiled_bf16_cross_floats(int groups, int nq, int nk, int heads, int dh) { return total_floats(groups, nq, nk, heads, dh, true); }

int attn_tiled_bf16_core(const AttnBwdArgs& a, int dh, float* planes, hipStream_t s) {
    const bool time = a.causal && a.inv_freq;
    if (int rc = check_self_geometry(a)) return rc;
    const TiledArgs p = tiled_args(a, dh);
    return time ? launch_dh_bf16<GEO_TIME>(p, dh, planes, s) : launch_dh_bf16<GEO_FRAME>(p, dh, planes, s);
}

int attn_tiled_bf16_cross_core(const XAttnArgs& a, int dh, float* planes, hipStream_t s) { return launch_dh_bf16<GEO_CROSS>(tiled_args(a, dh), dh, planes, s); }

}  // namespace d4
