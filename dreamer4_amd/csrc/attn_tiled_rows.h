// What the two product forms of the tiled attention core of the training path share (attn_tiled.hip: every product on the f32-input MFMA;
// attn_tiled_bf16.hip: on the bf16 matrix pipe): the geometries and their visibility rule, the argument block, the per-row planes
// and their carve-up, the launchers' argument checks, the rotary helpers, P and dS of a score element, and the three per-row kernels pre / dprep / post.  All of it sits in an unnamed namespace: each of
// the two files instantiates its own copies.
//
// IMG (pre, dprep) = false is the fp32 form.  IMG = true is the bf16 form: the same fp32 arithmetic, then bf16 images (round to nearest even)
// of the rotated q, of k' and of the mixed v (pre) and of dO (dprep), each of them twice: row major [problem][item][DH] for the products that
// contract over features, and transposed [problem][DH][items rounded up to 32] for the products that contract over items.  The kernel that
// owns a transposed image writes its pad columns as zero (its grid covers the padded items).  The fp32 planes no kernel of that form reads
// (qr, kn, dO) are not written, and dprep forms the row term delta from the ROUNDED dO.
#pragma once
#ifndef D4_ATTN_TILED_FORM_FILE
#error "attn_tiled_rows.h defines kernels in an unnamed namespace: it is for attn_tiled.hip and attn_tiled_bf16.hip alone (declarations for everyone else: attn_tiled.h)"
#endif
#include "attn_tiled.h"
#include "kernels.h"
#include <float.h>

namespace d4 {

namespace {

enum { GEO_TIME = 0, GEO_FRAME = 1, GEO_CROSS = 2 };

// row of item j of group g = (g / g_inner) * outer + g % g_inner + j * item   (AttnBwdArgs' rule; item-major keys: g_inner G, outer 0, item G)
struct RowMap { int g_inner; int64_t outer, item; };
__device__ __forceinline__ int64_t row_of(const RowMap& m, int g, int j) { return (int64_t)(g / m.g_inner) * m.outer + (g % m.g_inner) + j * m.item; }

// what the kernels see of either argument block (AttnBwdArgs: one buffer, both sides; XAttnArgs: two)
struct TiledArgs {
    const float* projq; int ldq;       // q @ 0, gate logit @ gcol + head
    const float* projk; int ldk;       // k @ kcol, v @ vcol, mix logit @ mcol + head (self geometries)
    int kcol, vcol, gcol, mcol;
    const float *rv, *gamma, *d_o3, *inv_freq;
    float *o3, *dprojq, *dprojk, *d_rv, *dgamma_part;
    int G, nq, nk, heads;
    float softclamp; int num_special, belief;
    RowMap qm, km;
};

inline TiledArgs tiled_args(const AttnBwdArgs& a, int dh) {
    const int hd = a.heads * dh;
    const RowMap rm{a.g_inner, a.g_outer_stride, a.item_stride};
    return TiledArgs{a.proj, a.ldp, a.proj, a.ldp, hd, 2 * hd, 3 * hd, 3 * hd + a.hp4, a.rv, a.gamma, a.d_o3, a.inv_freq,
                     a.o3, a.dproj, a.dproj, a.d_rv, a.dgamma_part, a.F, a.S, a.S, a.heads, a.softclamp, a.num_special, a.belief, rm, rm};
}
inline TiledArgs tiled_args(const XAttnArgs& a, int dh) {
    const int hd = a.heads * dh;
    const RowMap qm{1, a.nq, 1}, km = a.item_major ? RowMap{a.G > 0 ? a.G : 1, 0, a.G} : RowMap{1, a.nk, 1};
    return TiledArgs{a.projq, a.ldq, a.projk, a.ldk, 0, hd, hd, 0, nullptr, a.gamma, a.d_o3, nullptr,
                     a.o3, a.dprojq, a.dprojk, nullptr, a.dgamma_part, a.G, a.nq, a.nk, a.heads, a.softclamp, 0, 0, qm, km};
}

// what either form's launcher checks before it carves the planes (the cross geometry has no more to check)
inline int check_tiled(const TiledArgs& a, int dh, const float* planes) {
    D4_REQUIRE(planes, "tiled attention core: no planes");
    D4_REQUIRE(a.nq >= 1 && a.nq <= ATT_MAX_FRAMES && a.nk >= 1 && a.nk <= ATT_MAX_FRAMES, "tiled attention core: %d queries / %d keys per problem (max %d)",
               a.nq, a.nk, ATT_MAX_FRAMES);
    D4_REQUIRE((int64_t)a.G * a.heads <= 0x7fffffff, "tiled attention core: grid too large");
    D4_REQUIRE(dh == 64 || dh == 32 || dh == 16, "tiled attention core: head dim %d (16, 32 or 64)", dh);
    return 0;
}
inline int check_self_geometry(const AttnBwdArgs& a) {
    const bool time = a.causal && a.inv_freq;
    D4_REQUIRE(time || (!a.causal && !a.inv_freq), "tiled attention core: the time geometry (causal, rotary) or the within-frame geometry (neither)");
    D4_REQUIRE(a.S >= 1 && a.S <= ATT_MAX_FRAMES, "tiled attention core: %d items per group (max %d)", a.S, ATT_MAX_FRAMES);
    D4_REQUIRE(time ? a.num_special == 0 : (a.num_special >= 0 && a.num_special <= a.S), "tiled attention core: %d special items of %d", a.num_special, a.S);
    return 0;
}

// query i sees key j
template <int GEO>
__device__ __forceinline__ bool sees(int i, int j, int nk, int fs) {
    if (GEO == GEO_TIME) return j <= i && j < nk;
    if (GEO == GEO_FRAME) return j < nk && !(i < fs && j >= fs);
    return j < nk;
}
// the last key any of the queries i0 .. i0 + 15 sees (a wave of ordinary queries stops before the special block)
template <int GEO>
__device__ __forceinline__ int last_key(int i0, int nk, int fs) {
    if (GEO == GEO_TIME) return (i0 + 15 < nk - 1) ? i0 + 15 : nk - 1;
    if (GEO == GEO_FRAME) return (i0 + 15 < fs) ? fs - 1 : nk - 1;
    return nk - 1;
}
// the first query tile (a multiple of 16) with a query that sees any of the keys j0 .. j0 + 15 (an all-special key tile: the special queries only)
template <int GEO>
__device__ __forceinline__ int first_query(int j0, int fs) {
    if (GEO == GEO_TIME) return j0;
    if (GEO == GEO_FRAME) return j0 >= fs ? (fs & ~15) : 0;
    return 0;
}

__device__ __forceinline__ float sigm_t(float x) { return 1.f / (1.f + expf(-x)); }

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

struct TiledPlanes {
    float *qr, *o, *dO, *dq;                                       // [G * heads][nq][DH]
    float *kn, *kh, *vm, *dvd, *dkn, *dv;                          // [G * heads][nk][DH]  (dvd, like vinv and mx: the self geometries only)
    float *gt, *lse, *delta;                                       // [G * heads][nq]
    float *kinv, *vinv, *mx;                                       // [G * heads][nk]
    // the bf16 form only, behind the carve-up (null otherwise): row-major images [G * heads][items][DH], transposed images
    // [G * heads][DH][nqp | nkp] with nqp / nkp = nq / nk rounded up to 32 and zeros in the pad columns
    uint16_t *qb, *dob, *kb, *vb, *qt, *dot, *kt, *vt;
    int nqp, nkp;
};

__device__ __forceinline__ uint16_t bf16_bits(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }      // round to nearest even
__device__ __forceinline__ float bf16_round(float x) { return (float)(__bf16)x; }

// Rq query rows and Rk key rows in all (the self geometries: Rq = Rk); base null: the size only
inline size_t carve(TiledPlanes& t, float* base, size_t Rq, size_t Rk, int heads, int dh, bool cross) {
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 63) / 64 * 64; return p; };
    const size_t bq = Rq * heads * dh, bk = Rk * heads * dh, sq = Rq * heads, sk = Rk * heads;
    t.qr = take(bq); t.kn = take(bk); t.kh = take(bk); t.vm = take(bk); t.o = take(bq); t.dO = take(bq);
    t.dvd = cross ? nullptr : take(bk);
    t.dq = take(bq); t.dkn = take(bk); t.dv = take(bk);
    t.kinv = take(sk);
    t.vinv = cross ? nullptr : take(sk); t.mx = cross ? nullptr : take(sk);
    t.gt = take(sq); t.lse = take(sq); t.delta = take(sq);
    return off;
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

// ---- pre-pass: grid (G * heads, ceil(max(nq, nk) / 4)), one wave per row
// (IMG: grid (G * heads, ceil(max(nqp, nkp) / 4)); the waves of items n .. np - 1 write the pad columns of the transposed images)
template <int DH, int GEO, bool IMG>
__global__ __launch_bounds__(256) void tiled_pre_kernel(TiledArgs p, TiledPlanes t) {
    const int hd = p.heads * DH;
    const int gh = blockIdx.x, f = gh / p.heads, h = gh % p.heads;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool on = lane < DH;
    const float sc = on ? (p.gamma[h * DH + lane] + 1.f) * sqrtf((float)DH) : 0.f;
    if (GEO == GEO_CROSS) {                                            // the two sides are different rows of different buffers
        if (j < p.nk) {
            const float* pr = p.projk + row_of(p.km, f, j) * p.ldk;
            const float kv = on ? pr[p.kcol + h * DH + lane] : 0.f, vv = on ? pr[p.vcol + h * DH + lane] : 0.f;
            const float ki = 1.f / fmaxf(sqrtf(wave_sum(kv * kv)), 1e-12f);
            const int64_t sj = (int64_t)gh * p.nk + j;
            if (!IMG) {
                if (on) { t.kh[sj * DH + lane] = kv * ki; t.kn[sj * DH + lane] = kv * ki * sc; t.vm[sj * DH + lane] = vv; }
            } else if (on) {
                const uint16_t kb = bf16_bits(kv * ki * sc), vb = bf16_bits(vv);
                t.kh[sj * DH + lane] = kv * ki; t.vm[sj * DH + lane] = vv;
                t.kb[sj * DH + lane] = kb; t.vb[sj * DH + lane] = vb;
                t.kt[((int64_t)gh * DH + lane) * t.nkp + j] = kb; t.vt[((int64_t)gh * DH + lane) * t.nkp + j] = vb;
            }
            if (lane == 0) t.kinv[sj] = ki;
        } else if (IMG && j < t.nkp && on) {
            t.kt[((int64_t)gh * DH + lane) * t.nkp + j] = 0; t.vt[((int64_t)gh * DH + lane) * t.nkp + j] = 0;
        }
        if (j < p.nq) {
            const float* pr = p.projq + row_of(p.qm, f, j) * p.ldq;
            const int64_t si = (int64_t)gh * p.nq + j;
            if (!IMG) {
                if (on) t.qr[si * DH + lane] = pr[h * DH + lane];
            } else if (on) {
                const uint16_t qb = bf16_bits(pr[h * DH + lane]);
                t.qb[si * DH + lane] = qb; t.qt[((int64_t)gh * DH + lane) * t.nqp + j] = qb;
            }
            if (lane == 0) t.gt[si] = sigm_t(pr[p.gcol + h]);
        } else if (IMG && j < t.nqp && on) t.qt[((int64_t)gh * DH + lane) * t.nqp + j] = 0;
        return;
    }
    const int T = p.nk;
    if (j >= T) {
        if (IMG && j < t.nkp && on) {
            const int64_t tj = ((int64_t)gh * DH + lane) * t.nkp + j;
            t.qt[tj] = 0; t.kt[tj] = 0; t.vt[tj] = 0;
        }
        return;
    }
    const int64_t row = row_of(p.km, f, j);
    const float freq = (GEO == GEO_TIME && on) ? p.inv_freq[lane & (DH / 2 - 1)] : 0.f;
    const float* pr = p.projk + row * p.ldk;
    const float qv = on ? pr[h * DH + lane] : 0.f, kv = on ? pr[hd + h * DH + lane] : 0.f;
    float vv = on ? pr[2 * hd + h * DH + lane] : 0.f;
    float mx = 0.f;
    if (p.rv) {
        mx = sigm_t(pr[p.mcol + h]);
        const float r = on ? p.rv[row * hd + h * DH + lane] : 0.f;
        vv = vv + mx * (r - vv);
    }
    const float ki = 1.f / fmaxf(sqrtf(wave_sum(kv * kv)), 1e-12f);
    const float vi = 1.f / fmaxf(sqrtf(wave_sum(vv * vv)), 1e-12f);
    const float qrot = GEO == GEO_TIME ? rot_fwd<DH>(qv, j, freq, lane, on) : qv;
    const float krot = GEO == GEO_TIME ? rot_fwd<DH>(kv * ki * sc, j, freq, lane, on) : kv * ki * sc;
    const int64_t sj = (int64_t)gh * T + j;
    if (!IMG) {
        if (on) {
            t.qr[sj * DH + lane] = qrot; t.kh[sj * DH + lane] = kv * ki; t.kn[sj * DH + lane] = krot; t.vm[sj * DH + lane] = vv;
        }
    } else if (on) {
        const uint16_t qb = bf16_bits(qrot), kb = bf16_bits(krot), vb = bf16_bits(vv);
        const int64_t tj = ((int64_t)gh * DH + lane) * t.nkp + j;
        t.kh[sj * DH + lane] = kv * ki; t.vm[sj * DH + lane] = vv;
        t.qb[sj * DH + lane] = qb; t.kb[sj * DH + lane] = kb; t.vb[sj * DH + lane] = vb;
        t.qt[tj] = qb; t.kt[tj] = kb; t.vt[tj] = vb;
    }
    if (lane == 0) { t.kinv[sj] = ki; t.vinv[sj] = vi; t.mx[sj] = mx; t.gt[sj] = sigm_t(pr[p.gcol + h]); }
}

// ---- gate and belief backward per query row: grid (G * heads, ceil(nq / 4)), one wave per row, lane = feature
// (IMG: grid (G * heads, ceil(nqp / 4)); the waves of queries nq .. nqp - 1 write the pad columns of the transposed image of dO)
template <int DH, int GEO, bool IMG>
__global__ __launch_bounds__(256) void tiled_dprep_kernel(TiledArgs p, TiledPlanes t) {
    const int nq = p.nq, hd = p.heads * DH;
    const int gh = blockIdx.x, f = gh / p.heads, h = gh % p.heads;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool on = lane < DH;
    if (i >= nq) {
        if (IMG && i < t.nqp && on) t.dot[((int64_t)gh * DH + lane) * t.nqp + i] = 0;
        return;
    }
    const bool belief = GEO != GEO_CROSS && p.belief;
    const int64_t row = row_of(p.qm, f, i);
    const int64_t si = (int64_t)gh * nq + i;
    const float o = on ? t.o[si * DH + lane] : 0.f;
    const float vinv = GEO == GEO_CROSS ? 0.f : t.vinv[si], gt = t.gt[si];
    const float vni = (GEO != GEO_CROSS && on ? t.vm[si * DH + lane] : 0.f) * vinv;
    const float sdot = belief ? wave_sum(o * vni) : 0.f;
    const float o2 = o - sdot * vni;
    const float d3 = on ? p.d_o3[row * hd + h * DH + lane] : 0.f;
    const float dgl = wave_sum(d3 * o2) * gt * (1.f - gt);
    if (lane == 0) p.dprojq[row * p.ldq + p.gcol + h] = dgl;
    const float d2 = d3 * gt;
    float dOi = d2, dvdir = 0.f;
    if (belief) {
        const float c2 = wave_sum(d2 * vni);
        dOi = d2 - c2 * vni;
        const float dvn = -(sdot * d2 + c2 * o);
        dvdir = (dvn - wave_sum(dvn * vni) * vni) * vinv;
    }
    // the softmax backward's row term: sum_j P_ij (dO_i . v_j) = dO_i . o_i  (IMG: of the rounded dO the product dP = dO^ v^T takes, so that dP - delta cancels)
    const float delta = wave_sum((IMG ? bf16_round(dOi) : dOi) * o);
    if (!IMG) {
        if (on) { t.dO[si * DH + lane] = dOi; if (GEO != GEO_CROSS) t.dvd[si * DH + lane] = dvdir; }
    } else if (on) {
        t.dob[si * DH + lane] = bf16_bits(dOi); t.dot[((int64_t)gh * DH + lane) * t.nqp + i] = bf16_bits(dOi);
        if (GEO != GEO_CROSS) t.dvd[si * DH + lane] = dvdir;
    }
    if (lane == 0) t.delta[si] = delta;
}

// ---- post-pass: one block per (group, head), wave w takes rows w, w + 4, ...; lane = feature
template <int DH, int GEO>
__global__ __launch_bounds__(256) void tiled_post_kernel(TiledArgs p, TiledPlanes t) {
    __shared__ float gpart[4][64];
    const int nq = p.nq, nk = p.nk, hd = p.heads * DH;
    const int gh = blockIdx.x, f = gh / p.heads, h = gh % p.heads;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool on = lane < DH;
    const float sc = on ? (p.gamma[h * DH + lane] + 1.f) * sqrtf((float)DH) : 0.f;
    const float freq = (GEO == GEO_TIME && on) ? p.inv_freq[lane & (DH / 2 - 1)] : 0.f;
    float gacc = 0.f;
    for (int j = w; j < nk; j += 4) {
        const int64_t sj = (int64_t)gh * nk + j, row = row_of(p.km, f, j);
        float* dr = p.dprojk + row * p.ldk;
        if (GEO != GEO_CROSS) {                                        // (query j is the same row)
            const float dqp = on ? t.dq[sj * DH + lane] : 0.f;
            const float dq = GEO == GEO_TIME ? rot_bwd<DH>(dqp, j, freq, lane, on) : dqp;
            if (on) dr[h * DH + lane] = dq;
        }
        const float dknp = on ? t.dkn[sj * DH + lane] : 0.f;
        const float dkn = GEO == GEO_TIME ? rot_bwd<DH>(dknp, j, freq, lane, on) : dknp;
        const float khj = on ? t.kh[sj * DH + lane] : 0.f;
        gacc += dkn * khj;
        const float dkh = dkn * sc;
        const float dk = (dkh - wave_sum(dkh * khj) * khj) * t.kinv[sj];
        if (on) dr[p.kcol + h * DH + lane] = dk;
        if (GEO == GEO_CROSS) {
            if (on) dr[p.vcol + h * DH + lane] = t.dv[sj * DH + lane];
            continue;
        }
        const float dv = on ? t.dvd[sj * DH + lane] + t.dv[sj * DH + lane] : 0.f;
        if (p.rv) {
            const float mx = t.mx[sj];
            const float* pr = p.projk + row * p.ldk;
            const float vraw = on ? pr[2 * hd + h * DH + lane] : 0.f;
            const float r = on ? p.rv[row * hd + h * DH + lane] : 0.f;
            const float dmx = wave_sum(dv * (r - vraw));
            if (on) { dr[2 * hd + h * DH + lane] = dv * (1.f - mx); p.d_rv[row * hd + h * DH + lane] = dv * mx; }
            if (lane == 0) dr[p.mcol + h] = dmx * mx * (1.f - mx);
        } else {
            if (on) dr[2 * hd + h * DH + lane] = dv;
            if (lane == 0) dr[p.mcol + h] = 0.f;
        }
    }
    if (GEO == GEO_CROSS)
        for (int i = w; i < nq; i += 4)
            if (on) p.dprojq[row_of(p.qm, f, i) * p.ldq + h * DH + lane] = t.dq[((int64_t)gh * nq + i) * DH + lane];
    gpart[w][lane] = gacc;
    __syncthreads();
    if (w == 0 && on) p.dgamma_part[(int64_t)f * hd + h * DH + lane] = (((gpart[0][lane] + gpart[1][lane]) + gpart[2][lane]) + gpart[3][lane]) * sqrtf((float)DH);
}

}  // namespace

}  // namespace d4
