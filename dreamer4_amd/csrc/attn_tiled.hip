// Tiled (flash-style) causal attention core of the training time layers: the semantics of backward.hip's attn_bwd_kernel (rotary on q and on
// the normalised, scaled key; key RMS-norm with (gamma + 1) sqrt(dh); value-residual mix; softclamp; causal mask; belief projection; head
// gate) for up to ATT_MAX_FRAMES frames per trajectory, with memory linear in the frames.
//
// Six kernels over per-row planes ([group * heads + head][frame][DH], so a (group, head) problem is contiguous whatever the row geometry):
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
#include "attn_tiled.h"
#include "kernels.h"
#include <float.h>

namespace d4 {

int g_time_attn_tiled = 0;

namespace {

__device__ __forceinline__ float sigm_t(float x) { return 1.f / (1.f + expf(-x)); }

struct TiledPlanes {
    float *qr, *kn, *kh, *vm, *o, *dO, *dvd, *dq, *dkn, *dv;      // [F * heads][T][DH]
    float *kinv, *vinv, *mx, *gt, *lse, *delta;                    // [F * heads][T]
};

constexpr int TL_PLANES = 10, TL_SCALARS = 6;

TiledPlanes carve(float* base, int R, int heads, int dh) {
    TiledPlanes t{};
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base + off; off += (n + 63) / 64 * 64; return p; };
    const size_t big = (size_t)R * heads * dh, small = (size_t)R * heads;
    t.qr = take(big); t.kn = take(big); t.kh = take(big); t.vm = take(big); t.o = take(big); t.dO = take(big); t.dvd = take(big);
    t.dq = take(big); t.dkn = take(big); t.dv = take(big);
    t.kinv = take(small); t.vinv = take(small); t.mx = take(small); t.gt = take(small); t.lse = take(small); t.delta = take(small);
    return t;
}

// rotary as in attn_bwd_kernel: lane = feature, the partner feature is lane ^ (DH / 2)
template <int DH>
__device__ __forceinline__ float rot_fwd(float t, int pos, float freq, int lane, bool on) {
    float sn, cs;
    sincosf(freq * (float)pos, &sn, &cs);
    const float partner = __shfl(t, lane ^ (DH / 2));
    return on ? t * cs + (lane < DH / 2 ? -partner : partner) * sn : 0.f;
}
template <int DH>
__device__ __forceinline__ float rot_bwd(float y, int pos, float freq, int lane, bool on) {
    float sn, cs;
    sincosf(freq * (float)pos, &sn, &cs);
    const float partner = __shfl(y * sn, lane ^ (DH / 2));
    return on ? y * cs + (lane < DH / 2 ? partner : -partner) : 0.f;
}

__device__ __forceinline__ int64_t group_row0(const AttnBwdArgs& p, int f) { return (int64_t)(f / p.g_inner) * p.g_outer_stride + (f % p.g_inner); }

// ---- pre-pass: grid (F * heads, ceil(T / 4)), one wave per row
template <int DH>
__global__ __launch_bounds__(256) void tiled_pre_kernel(AttnBwdArgs p, TiledPlanes t) {
    const int T = p.S, hd = p.heads * DH;
    const int gh = blockIdx.x, f = gh / p.heads, h = gh % p.heads;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (j >= T) return;
    const bool on = lane < DH;
    const int64_t row = group_row0(p, f) + j * p.item_stride;
    const float sc = on ? (p.gamma[h * DH + lane] + 1.f) * sqrtf((float)DH) : 0.f;
    const float freq = on ? p.inv_freq[lane & (DH / 2 - 1)] : 0.f;
    const float* pr = p.proj + row * p.ldp;
    const float qv = on ? pr[h * DH + lane] : 0.f, kv = on ? pr[hd + h * DH + lane] : 0.f;
    float vv = on ? pr[2 * hd + h * DH + lane] : 0.f;
    float mx = 0.f;
    if (p.rv) {
        mx = sigm_t(pr[3 * hd + p.hp4 + h]);
        const float r = on ? p.rv[row * hd + h * DH + lane] : 0.f;
        vv = vv + mx * (r - vv);
    }
    const float ki = 1.f / fmaxf(sqrtf(wave_sum(kv * kv)), 1e-12f);
    const float vi = 1.f / fmaxf(sqrtf(wave_sum(vv * vv)), 1e-12f);
    const float qrot = rot_fwd<DH>(qv, j, freq, lane, on), krot = rot_fwd<DH>(kv * ki * sc, j, freq, lane, on);
    const int64_t sj = (int64_t)gh * T + j;
    if (on) {
        t.qr[sj * DH + lane] = qrot; t.kh[sj * DH + lane] = kv * ki; t.kn[sj * DH + lane] = krot; t.vm[sj * DH + lane] = vv;
    }
    if (lane == 0) { t.kinv[sj] = ki; t.vinv[sj] = vi; t.mx[sj] = mx; t.gt[sj] = sigm_t(pr[3 * hd + h]); }
}

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

// ---- forward: grid (F * heads, ceil(T / 64)); wave w of a block owns queries 64 blockIdx.y + 16 w .. + 15
template <int DH>
__global__ __launch_bounds__(256) void tiled_fwd_kernel(AttnBwdArgs p, TiledPlanes t) {
    constexpr int NS = DH / 16;
    const int T = p.S, hd = p.heads * DH;
    const int gh = blockIdx.x, f = gh / p.heads, h = gh % p.heads;
    const int lane = threadIdx.x & 63, tok = lane & 15, kq = lane >> 4;
    const int i0 = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (i0 >= T) return;
    const int64_t pb = (int64_t)gh * T * DH, sb = (int64_t)gh * T;
    const float *Q = t.qr + pb, *K = t.kn + pb, *V = t.vm + pb;
    const float scale = rsqrtf((float)DH);
    const int i = i0 + tok;
    const int jmax = (i0 + 15 < T - 1) ? i0 + 15 : T - 1;           // the last key any query of this wave sees
    f32x4 q4[NS], o[NS];
    load_rows<NS>(q4, Q, i, T, kq);
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
            load_rows<NS>(k4, K, jb + tok, T, kq);
            const f32x4 st = dot_tile<NS>(k4, q4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = jb + 4 * kq + r;
                float simc = st[r] * scale;
                if (p.softclamp > 0.f) simc = tanhf(simc / p.softclamp) * p.softclamp;
                pr[kt][r] = (j <= i && j < T) ? simc : -FLT_MAX;
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
            acc_rows<NS>(o, pr[kt], V, jb, T, kq, tok);
        }
    }
    const float lse = m + logf(l), linv = 1.f / l;
    float lse_r[4], linv_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { lse_r[r] = __shfl(lse, 4 * kq + r); linv_r[r] = __shfl(linv, 4 * kq + r); }
    const int64_t row0 = group_row0(p, f);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = i0 + 4 * kq + r;
        if (qi >= T) continue;                                         // (uniform over each 16-lane row group)
        float on_[NS], vn[NS], dot = 0.f;
        const float vinv = t.vinv[sb + qi];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            on_[s] = o[s][r] * linv_r[r];
            t.o[pb + (int64_t)qi * DH + 16 * s + tok] = on_[s];
            vn[s] = V[(int64_t)qi * DH + 16 * s + tok] * vinv;
            dot = __builtin_fmaf(on_[s], vn[s], dot);
        }
        dot = p.belief ? row_sum16(dot) : 0.f;
        if (tok == 0) t.lse[sb + qi] = lse_r[r];
        const float gt = t.gt[sb + qi];
        float* orow = p.o3 + (row0 + qi * p.item_stride) * hd + h * DH;
#pragma unroll
        for (int s = 0; s < NS; ++s) orow[16 * s + tok] = (on_[s] - dot * vn[s]) * gt;
    }
}

// ---- gate and belief backward per row: grid (F * heads, ceil(T / 4)), one wave per row, lane = feature
template <int DH>
__global__ __launch_bounds__(256) void tiled_dprep_kernel(AttnBwdArgs p, TiledPlanes t) {
    const int T = p.S, hd = p.heads * DH;
    const int gh = blockIdx.x, f = gh / p.heads, h = gh % p.heads;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= T) return;
    const bool on = lane < DH;
    const int64_t row = group_row0(p, f) + i * p.item_stride;
    const int64_t si = (int64_t)gh * T + i;
    const float o = on ? t.o[si * DH + lane] : 0.f;
    const float vinv = t.vinv[si], gt = t.gt[si];
    const float vni = (on ? t.vm[si * DH + lane] : 0.f) * vinv;
    const float sdot = p.belief ? wave_sum(o * vni) : 0.f;
    const float o2 = o - sdot * vni;
    const float d3 = on ? p.d_o3[row * hd + h * DH + lane] : 0.f;
    const float dgl = wave_sum(d3 * o2) * gt * (1.f - gt);
    if (lane == 0) p.dproj[row * p.ldp + 3 * hd + h] = dgl;
    const float d2 = d3 * gt;
    float dOi = d2, dvdir = 0.f;
    if (p.belief) {
        const float c2 = wave_sum(d2 * vni);
        dOi = d2 - c2 * vni;
        const float dvn = -(sdot * d2 + c2 * o);
        dvdir = (dvn - wave_sum(dvn * vni) * vni) * vinv;
    }
    const float delta = wave_sum(dOi * o);                             // the softmax backward's row term: sum_j P_ij (dO_i . v_j) = dO_i . o_i
    if (on) { t.dO[si * DH + lane] = dOi; t.dvd[si * DH + lane] = dvdir; }
    if (lane == 0) t.delta[si] = delta;
}

// P and dS of one score element: sim = q . k (the key carries its scale), lse the query row's log-sum-exp, delta its dO . o
__device__ __forceinline__ void p_and_ds(float dotqk, float dp, float lse, float delta, bool valid, float scale, float softclamp, float& pij, float& ds) {
    const float sim = dotqk * scale;
    float th = 0.f, simc = sim;
    if (softclamp > 0.f) { th = tanhf(sim / softclamp); simc = th * softclamp; }
    pij = valid ? expf(simc - lse) : 0.f;
    ds = pij * (dp - delta);
    if (softclamp > 0.f) ds *= 1.f - th * th;
    ds *= scale;
}

// ---- dQ: grid (F * heads, ceil(T / 64)); wave w owns queries 64 blockIdx.y + 16 w .. + 15 and walks the key tiles <= its own
template <int DH>
__global__ __launch_bounds__(256) void tiled_dq_kernel(AttnBwdArgs p, TiledPlanes t) {
    constexpr int NS = DH / 16;
    const int T = p.S;
    const int gh = blockIdx.x;
    const int lane = threadIdx.x & 63, tok = lane & 15, kq = lane >> 4;
    const int i0 = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (i0 >= T) return;
    const int64_t pb = (int64_t)gh * T * DH, sb = (int64_t)gh * T;
    const float *Q = t.qr + pb, *K = t.kn + pb, *V = t.vm + pb, *DO = t.dO + pb;
    const float scale = rsqrtf((float)DH);
    const int i = i0 + tok;
    const int jmax = (i0 + 15 < T - 1) ? i0 + 15 : T - 1;
    f32x4 q4[NS], do4[NS], dq[NS];
    load_rows<NS>(q4, Q, i, T, kq);
    load_rows<NS>(do4, DO, i, T, kq);
#pragma unroll
    for (int s = 0; s < NS; ++s) dq[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float lse = i < T ? t.lse[sb + i] : 0.f, delta = i < T ? t.delta[sb + i] : 0.f;
    for (int jb = 0; jb <= jmax; jb += 16) {
        f32x4 k4[NS], v4[NS];
        load_rows<NS>(k4, K, jb + tok, T, kq);
        load_rows<NS>(v4, V, jb + tok, T, kq);
        const f32x4 st = dot_tile<NS>(k4, q4);                         // st[r] = q_i . k_j, j = jb + 4 kq + r
        const f32x4 dpt = dot_tile<NS>(v4, do4);                       // dO_i . v_j
        f32x4 ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = jb + 4 * kq + r;
            float pij, d;
            p_and_ds(st[r], dpt[r], lse, delta, j <= i && j < T && i < T, scale, p.softclamp, pij, d);
            ds[r] = d;
        }
        acc_rows<NS>(dq, ds, K, jb, T, kq, tok);                       // dq_i += sum_j dS_ij k_j
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = i0 + 4 * kq + r;
        if (qi >= T) continue;
#pragma unroll
        for (int s = 0; s < NS; ++s) t.dq[pb + (int64_t)qi * DH + 16 * s + tok] = dq[s][r];
    }
}

// ---- dK / dV: grid (F * heads, ceil(T / 64)); wave w owns keys 64 blockIdx.y + 16 w .. + 15 and walks the query tiles >= its own
template <int DH>
__global__ __launch_bounds__(256) void tiled_dkv_kernel(AttnBwdArgs p, TiledPlanes t) {
    constexpr int NS = DH / 16;
    const int T = p.S;
    const int gh = blockIdx.x;
    const int lane = threadIdx.x & 63, tok = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (j0 >= T) return;
    const int64_t pb = (int64_t)gh * T * DH, sb = (int64_t)gh * T;
    const float *Q = t.qr + pb, *K = t.kn + pb, *V = t.vm + pb, *DO = t.dO + pb;
    const float scale = rsqrtf((float)DH);
    const int j = j0 + tok;
    f32x4 k4[NS], v4[NS], dk[NS], dv[NS];
    load_rows<NS>(k4, K, j, T, kq);
    load_rows<NS>(v4, V, j, T, kq);
#pragma unroll
    for (int s = 0; s < NS; ++s) { dk[s] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[s] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int ib = j0; ib < T; ib += 16) {
        f32x4 q4[NS], do4[NS];
        load_rows<NS>(q4, Q, ib + tok, T, kq);
        load_rows<NS>(do4, DO, ib + tok, T, kq);
        const f32x4 st = dot_tile<NS>(q4, k4);                         // st[r] = q_i . k_j, i = ib + 4 kq + r
        const f32x4 dpt = dot_tile<NS>(do4, v4);
        f32x4 pt, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = ib + 4 * kq + r;
            const bool in = i < T;
            const float lse = in ? t.lse[sb + i] : 0.f, delta = in ? t.delta[sb + i] : 0.f;
            float pij, d;
            p_and_ds(st[r], dpt[r], lse, delta, in && j <= i && j < T, scale, p.softclamp, pij, d);
            pt[r] = pij; ds[r] = d;
        }
        acc_rows<NS>(dv, pt, DO, ib, T, kq, tok);                      // dv_j += sum_i P_ij dO_i
        acc_rows<NS>(dk, ds, Q, ib, T, kq, tok);                       // dk_j += sum_i dS_ij q_i
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int kj = j0 + 4 * kq + r;
        if (kj >= T) continue;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            t.dkn[pb + (int64_t)kj * DH + 16 * s + tok] = dk[s][r];
            t.dv[pb + (int64_t)kj * DH + 16 * s + tok] = dv[s][r];
        }
    }
}

// ---- post-pass: one block per (group, head), wave w takes rows w, w + 4, ...; lane = feature
template <int DH>
__global__ __launch_bounds__(256) void tiled_post_kernel(AttnBwdArgs p, TiledPlanes t) {
    __shared__ float gpart[4][64];
    const int T = p.S, hd = p.heads * DH;
    const int gh = blockIdx.x, f = gh / p.heads, h = gh % p.heads;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool on = lane < DH;
    const int64_t row0 = group_row0(p, f);
    const float sc = on ? (p.gamma[h * DH + lane] + 1.f) * sqrtf((float)DH) : 0.f;
    const float freq = on ? p.inv_freq[lane & (DH / 2 - 1)] : 0.f;
    float gacc = 0.f;
    for (int j = w; j < T; j += 4) {
        const int64_t sj = (int64_t)gh * T + j, row = row0 + j * p.item_stride;
        float* dr = p.dproj + row * p.ldp;
        const float dq = rot_bwd<DH>(on ? t.dq[sj * DH + lane] : 0.f, j, freq, lane, on);
        if (on) dr[h * DH + lane] = dq;
        const float dkn = rot_bwd<DH>(on ? t.dkn[sj * DH + lane] : 0.f, j, freq, lane, on);
        const float dv = on ? t.dvd[sj * DH + lane] + t.dv[sj * DH + lane] : 0.f;
        const float khj = on ? t.kh[sj * DH + lane] : 0.f;
        gacc += dkn * khj;
        const float dkh = dkn * sc;
        const float dk = (dkh - wave_sum(dkh * khj) * khj) * t.kinv[sj];
        if (on) dr[hd + h * DH + lane] = dk;
        if (p.rv) {
            const float mx = t.mx[sj];
            const float* pr = p.proj + row * p.ldp;
            const float vraw = on ? pr[2 * hd + h * DH + lane] : 0.f;
            const float r = on ? p.rv[row * hd + h * DH + lane] : 0.f;
            const float dmx = wave_sum(dv * (r - vraw));
            if (on) { dr[2 * hd + h * DH + lane] = dv * (1.f - mx); p.d_rv[row * hd + h * DH + lane] = dv * mx; }
            if (lane == 0) dr[3 * hd + p.hp4 + h] = dmx * mx * (1.f - mx);
        } else {
            if (on) dr[2 * hd + h * DH + lane] = dv;
            if (lane == 0) dr[3 * hd + p.hp4 + h] = 0.f;
        }
    }
    gpart[w][lane] = gacc;
    __syncthreads();
    if (w == 0 && on) p.dgamma_part[(int64_t)f * hd + h * DH + lane] = (((gpart[0][lane] + gpart[1][lane]) + gpart[2][lane]) + gpart[3][lane]) * sqrtf((float)DH);
}

template <int DH>
int launch_tiled(const AttnBwdArgs& a, const TiledPlanes& t, hipStream_t s) {
    const int T = a.S;
    const dim3 block(256), rows(a.F * a.heads, (T + 3) / 4), tiles(a.F * a.heads, (T + 63) / 64);
    hipLaunchKernelGGL(tiled_pre_kernel<DH>, rows, block, 0, s, a, t);
    hipLaunchKernelGGL(tiled_fwd_kernel<DH>, tiles, block, 0, s, a, t);
    D4_LAUNCH_CHECK();
    if (!a.d_o3) return 0;
    hipLaunchKernelGGL(tiled_dprep_kernel<DH>, rows, block, 0, s, a, t);
    hipLaunchKernelGGL(tiled_dq_kernel<DH>, tiles, block, 0, s, a, t);
    hipLaunchKernelGGL(tiled_dkv_kernel<DH>, tiles, block, 0, s, a, t);
    hipLaunchKernelGGL(tiled_post_kernel<DH>, dim3(a.F * a.heads), block, 0, s, a, t);
    D4_LAUNCH_CHECK();
    return 0;
}

}  // namespace

size_t attn_tiled_floats(int R, int heads, int dh) {
    const size_t big = ((size_t)R * heads * dh + 63) / 64 * 64, small = ((size_t)R * heads + 63) / 64 * 64;
    return TL_PLANES * big + TL_SCALARS * small;
}

int attn_tiled_core(const AttnBwdArgs& a, int dh, float* planes, hipStream_t s) {
    D4_REQUIRE(a.causal && a.inv_freq && planes, "tiled attention core: time geometry (causal, rotary) and its planes only");
    D4_REQUIRE(a.S >= 1 && a.S <= ATT_MAX_FRAMES, "tiled attention core: %d frames (max %d)", a.S, ATT_MAX_FRAMES);
    D4_REQUIRE(a.num_special == 0, "tiled attention core: no special-token mask in the time geometry");
    D4_REQUIRE((int64_t)a.F * a.heads <= 0x7fffffff, "tiled attention core: grid too large");
    if (a.F * a.heads == 0) return 0;
    const TiledPlanes t = carve(planes, a.F * a.S, a.heads, dh);
    if (dh == 64) return launch_tiled<64>(a, t, s);
    if (dh == 32) return launch_tiled<32>(a, t, s);
    D4_REQUIRE(dh == 16, "tiled attention core: head dim %d (16, 32 or 64)", dh);
    return launch_tiled<16>(a, t, s);
}

}  // namespace d4
