// MuonAdamAtan2: the optimiser step of both whole-model trainings.
//
//   Muon group      one step of ALL 2-D trunk weights is  prepare, 3 grouped products per Newton-Schulz iteration, finish  per pass:
//                     prepare   m <- lerp(m, g, 1 - beta), u = nesterov ? lerp(g, m, beta) : m  (g scaled by the clip), u written into the work buffer
//                               X oriented rows <= cols with both dimensions zero-padded to the 128-tile, and per 32-row strip one partial of sum u^2
//                     gram      A  = X X^T                   (upper tiles, mirrored; iteration 0 scales X by 1 / max(|u|_F, eps) as it loads it)
//                     poly      B  = b A + c A A             (upper tiles, mirrored; A A computed as A A^T, the same bits for a symmetric A)
//                     apply     X' = a X + B X
//                     finish    W <- W (1 - lr wd) - lr s X  transposed back
//                   The three products are ONE kernel (template on the second operand's layout) on v_mfma_f32_32x32x2_f32 from LDS tiles: a workgroup of
//                   4 waves owns a 128 x 128 output tile (2 x 2 MFMA tiles per wave), k-tiles of 16 staged global -> registers -> LDS one tile ahead.
//                   A device tile table built at plan time maps blockIdx.x to (matrix, tile row, tile col): matrices of every shape share a launch.
//                   Every dimension the products see is a multiple of 128, so they carry no bounds logic at all: the ragged edges live in prepare/finish.
//   Adam-atan2      multi-tensor kernel over a device pointer table, one launch for the group.
//   gradient norm   multi-tensor partial sums (one per 4096-element chunk) and a one-block final sum: fixed order, no float atomics.
// Equal inputs and state give equal bits, whatever the pass partition: a matrix's arithmetic never depends on its neighbours in a launch.
// A plan created with products = 1 keeps prepare and this file's launch sequence and takes normalise, the products and finish from csrc/muon_bf16.hip
// (DESIGN.md 30); the description of a matrix, the plan and its table builder are in muon_plan.h for both.
#include <math.h>
#include <string.h>
#include <vector>

#include "../../include/d4hip.h"
#include "common.h"
#include "muon_plan.h"                // MuonMat, the plan and its table builder: shared with the bf16 form (csrc/muon_bf16.hip)

namespace d4 {

constexpr int MU_BK = 16;             // k-tile
constexpr int MU_LD = MU_T + 4;       // LDS row stride (floats): 16-byte aligned rows, transposing writes spread over all banks
constexpr int MT_CHUNK = 4096;        // elements per workgroup of the multi-tensor kernels

__device__ __forceinline__ float lerp_t(float s, float e, float w) {          // torch.lerp's two-sided form
    return w < 0.5f ? s + w * (e - s) : e - (e - s) * (1.f - w);
}

__device__ __forceinline__ float block_sum256(float v, float* sh) {           // fixed-order tree over 256 threads
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}

__device__ __forceinline__ float clip_coef(const float* gnorm_sq, float max_norm) {
    if (!gnorm_sq || max_norm <= 0.f) return 1.f;
    const float c = max_norm / (sqrtf(*gnorm_sq) + 1e-6f);                    // torch.nn.utils.clip_grad_norm_
    return c < 1.f ? c : 1.f;
}

// ---------------------------------------------------------------------------------------------- prepare
// blocks: int2 (matrix, strip).  A strip is MU_STRIP rows of the PADDED original matrix; the workgroup walks its 32 x 32 tiles.
__global__ __launch_bounds__(256) void muon_prepare_kernel(const MuonMat* mats, const int2* blocks, float* ws, float* partials, const float* gnorm_sq,
                                                           float max_norm, float beta, float one_minus_beta, int nesterov) {
    __shared__ float tile[32][33];
    __shared__ float red[256];
    const int2 bk = blocks[blockIdx.x];
    const MuonMat d = mats[bk.x];
    const float clip = clip_coef(gnorm_sq, max_norm);
    float* X = ws + d.x0;
    const int i0 = bk.y * MU_STRIP;
    const int cp_o = d.transposed ? d.Rp : d.Cp;                              // padded columns of the original orientation
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    float ss = 0.f;
    for (int j0 = 0; j0 < cp_o; j0 += 32) {
        float u[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + ty + 8 * q, j = j0 + tx;
            float v = 0.f;
            if (i < d.r && j < d.c) {
                const int64_t at = (int64_t)i * d.c + j;
                const float g = d.g[at] * clip;
                if (d.m) {
                    const float m = lerp_t(d.m[at], g, one_minus_beta);
                    d.m[at] = m;
                    v = nesterov ? lerp_t(g, m, beta) : m;
                } else {
                    v = g;
                }
            }
            u[q] = v;
            ss += v * v;
        }
        if (!d.transposed) {
#pragma unroll
            for (int q = 0; q < 4; ++q) X[(int64_t)(i0 + ty + 8 * q) * d.Cp + j0 + tx] = u[q];
        } else {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) tile[ty + 8 * q][tx] = u[q];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) X[(int64_t)(j0 + ty + 8 * q) * d.Cp + i0 + tx] = tile[tx][ty + 8 * q];
        }
    }
    const float tot = block_sum256(ss, red);
    if (threadIdx.x == 0) partials[d.part0 + bk.y] = tot;
}

// ---------------------------------------------------------------------------------------------- the three products
// tiles: int4 (matrix, tile row, tile col, 0).  stage 0: A = X X^T; 1: B = alpha A + beta A A^T; 2: X' = alpha X + B X.
// NN: the second operand is [k][n] (stage 2); otherwise both operands are [row][k].
template <bool NN>
__global__ __launch_bounds__(256) void muon_gemm_kernel(const MuonMat* mats, const int4* tiles, float* ws, const float* partials, int stage, int cur,
                                                        float alpha, float beta, int first, float eps) {
    __shared__ float sP[MU_BK][MU_LD];
    __shared__ float sQ[MU_BK][MU_LD];
    __shared__ float s_scale;
    const int4 t = tiles[blockIdx.x];
    const MuonMat d = mats[t.x];
    const float *P, *Q, *E;
    float* D;
    int ldp, ldq, ldd, K;
    float* Xc = ws + (cur ? d.x1 : d.x0);
    if (stage == 0) { P = Xc; Q = Xc; E = nullptr; D = ws + d.a; ldp = ldq = d.Cp; ldd = d.Rp; K = d.Cp; }
    else if (stage == 1) { P = ws + d.a; Q = P; E = P; D = ws + d.b; ldp = ldq = ldd = d.Rp; K = d.Rp; }
    else { P = ws + d.b; Q = Xc; E = Xc; D = ws + (cur ? d.x0 : d.x1); ldp = d.Rp; ldq = ldd = d.Cp; K = d.Rp; }
    const int m0 = t.y * MU_T, n0 = t.z * MU_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // iteration 0 reads the unnormalised u: 1 / max(|u|_F, eps) from the strip partials, summed in fixed order by wave 0
    float sc = 1.f;
    if (first) {
        if (wave == 0) {
            float s = 0.f;
            for (int i = lane; i < d.nparts; i += 64) s += partials[d.part0 + i];
            s = wave_sum(s);
            if (lane == 0) s_scale = 1.f / fmaxf(sqrtf(s), eps);
        }
        __syncthreads();
        sc = s_scale;
    }
    const float scP = (first && stage == 0) ? sc : 1.f;
    const float scQ = (first && stage != 1) ? sc : 1.f;

    f32x4 pv[2], qv[2];
    const int prow = tid >> 2, pk = (tid & 3) * 4;               // [row][k] operand: 64 rows x 4 quads per pass
    const int qk = tid >> 5, qn = (tid & 31) * 4;                // [k][n] operand: 8 k x 32 quads per pass
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            pv[h] = *reinterpret_cast<const f32x4*>(P + (int64_t)(m0 + prow + 64 * h) * ldp + k0 + pk);
            if constexpr (NN) qv[h] = *reinterpret_cast<const f32x4*>(Q + (int64_t)(k0 + qk + 8 * h) * ldq + n0 + qn);
            else qv[h] = *reinterpret_cast<const f32x4*>(Q + (int64_t)(n0 + prow + 64 * h) * ldq + k0 + pk);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sP[pk + i][prow + 64 * h] = pv[h][i] * scP;
            if constexpr (NN) {
                *reinterpret_cast<f32x4*>(&sQ[qk + 8 * h][qn]) = qv[h] * scQ;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) sQ[pk + i][prow + 64 * h] = qv[h][i] * scQ;
            }
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int l31 = lane & 31, lh = lane >> 5;

    fetch(0);
    for (int k0 = 0; k0 < K; k0 += MU_BK) {
        __syncthreads();
        stash();
        __syncthreads();
        if (k0 + MU_BK < K) fetch(k0 + MU_BK);
#pragma unroll
        for (int kk = 0; kk < MU_BK; kk += 2) {
            const float a0 = sP[kk + lh][wm + l31], a1 = sP[kk + lh][wm + 32 + l31];
            const float b0 = sQ[kk + lh][wn + l31], b1 = sQ[kk + lh][wn + 32 + l31];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }

    // epilogue: D = alpha * E + beta * acc; the symmetric stages also write the mirrored tile (4 consecutive rows of a lane = one 16-byte store)
    const bool mirror = stage != 2 && t.y != t.z;
    const float scE = (first && stage == 2) ? sc : 1.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn + 32 * j + l31;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = m0 + wm + 32 * i + 8 * g + 4 * lh;
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = beta * acc[i][j][4 * g + r];
                    if (E) v += alpha * (E[(int64_t)(row + r) * ldd + col] * scE);
                    o[r] = v;
                    D[(int64_t)(row + r) * ldd + col] = v;
                }
                if (mirror) *reinterpret_cast<f32x4*>(D + (int64_t)col * ldd + row) = o;
            }
        }
}

// ---------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(256) void muon_finish_kernel(const MuonMat* mats, const int2* blocks, const float* ws, int cur, float decay) {
    __shared__ float tile[32][33];
    const int2 bk = blocks[blockIdx.x];
    const MuonMat d = mats[bk.x];
    const int i0 = bk.y * MU_STRIP;
    if (i0 >= d.r) return;                                                    // a strip of padding only (uniform for the workgroup)
    const float* X = ws + (cur ? d.x1 : d.x0);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j0 = 0; j0 < d.c; j0 += 32) {
        float x[4];
        if (!d.transposed) {
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = X[(int64_t)(i0 + ty + 8 * q) * d.Cp + j0 + tx];
        } else {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) tile[ty + 8 * q][tx] = X[(int64_t)(j0 + ty + 8 * q) * d.Cp + i0 + tx];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = tile[tx][ty + 8 * q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + ty + 8 * q, j = j0 + tx;
            if (i < d.r && j < d.c) {
                const int64_t at = (int64_t)i * d.c + j;
                d.out[at] = d.w ? d.w[at] * decay + d.coef * x[q] : d.coef * x[q];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- multi-tensor kernels
struct MtTensor {                     // device table entry
    float* p; const float* g; float* m; float* v;
    int64_t n;
    int64_t block0;                   // first workgroup of this tensor
};

__device__ __forceinline__ int mt_find(const int32_t* owner) { return owner[blockIdx.x]; }

__global__ __launch_bounds__(256) void mt_sumsq_kernel(const MtTensor* tab, const int32_t* owner, float* partials) {
    __shared__ float red[256];
    const MtTensor t = tab[mt_find(owner)];
    const int64_t lo = ((int64_t)blockIdx.x - t.block0) * MT_CHUNK;
    const int64_t hi = lo + MT_CHUNK < t.n ? lo + MT_CHUNK : t.n;
    float s = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) s += t.g[i] * t.g[i];
    const float tot = block_sum256(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void mt_sumsq_final_kernel(const float* partials, int np, float* out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) s += partials[i];
    const float tot = block_sum256(s, red);
    if (threadIdx.x == 0) out[0] = tot;
}

__global__ __launch_bounds__(256) void mt_adam_atan2_kernel(const MtTensor* tab, const int32_t* owner, const float* gnorm_sq, float max_norm, float w1, float w2,
                                                            float decay, float lr_a, float b, float inv_bc1, float inv_bc2) {
    const MtTensor t = tab[mt_find(owner)];
    const float clip = clip_coef(gnorm_sq, max_norm);
    const int64_t lo = ((int64_t)blockIdx.x - t.block0) * MT_CHUNK;
    const int64_t hi = lo + MT_CHUNK < t.n ? lo + MT_CHUNK : t.n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const float g = t.g[i] * clip;
        const float m = lerp_t(t.m[i], g, w1);
        const float v = lerp_t(t.v[i], g * g, w2);
        t.m[i] = m; t.v[i] = v;
        t.p[i] = t.p[i] * decay - lr_a * atan2f(m * inv_bc1, b * sqrtf(v * inv_bc2));
    }
}

// host: layout of a multi-tensor table  [MtTensor x n][owner int32 x nblocks (padded to 16 bytes)][partials float x nblocks]
struct MtLayout { int64_t nblocks; size_t owner_off, part_off, bytes; };
static MtLayout mt_layout(int n, const int64_t* numel) {
    MtLayout L{};
    for (int i = 0; i < n; ++i) L.nblocks += (numel[i] + MT_CHUNK - 1) / MT_CHUNK;
    L.owner_off = sizeof(MtTensor) * (size_t)n;
    L.part_off = L.owner_off + (((size_t)L.nblocks * 4 + 15) & ~(size_t)15);
    L.bytes = L.part_off + (size_t)L.nblocks * 4;
    return L;
}

static int mt_upload(const char* who, int n, const int64_t* numel, void* const* p, const void* const* g, void* const* m, void* const* v, void* table,
                     const MtLayout& L, hipStream_t s) {
    std::vector<char> host(L.part_off);
    MtTensor* tab = reinterpret_cast<MtTensor*>(host.data());
    int32_t* owner = reinterpret_cast<int32_t*>(host.data() + L.owner_off);
    int64_t blk = 0;
    for (int i = 0; i < n; ++i) {
        D4_REQUIRE(g && g[i], "%s: grads[%d] is null", who, i);
        if (p) D4_REQUIRE(p[i] && m && m[i] && v && v[i], "%s: params / exp_avg / exp_avg_sq [%d] is null", who, i);
        tab[i] = MtTensor{p ? (float*)p[i] : nullptr, (const float*)g[i], m ? (float*)m[i] : nullptr, v ? (float*)v[i] : nullptr, numel[i], blk};
        const int64_t nb = (numel[i] + MT_CHUNK - 1) / MT_CHUNK;
        for (int64_t k = 0; k < nb; ++k) owner[blk + k] = i;
        blk += nb;
    }
    D4_HIP(hipMemcpyAsync(table, host.data(), L.part_off, hipMemcpyHostToDevice, s));
    D4_HIP(hipStreamSynchronize(s));          // `host` is pageable and dies with this frame
    return 0;
}

static int mt_check(const char* who, int n, const int64_t* numel, const void* table, size_t table_bytes, MtLayout* L) {
    D4_REQUIRE(n >= 1 && numel, "%s: n >= 1 and numel", who);
    for (int i = 0; i < n; ++i) D4_REQUIRE(numel[i] >= 1, "%s: numel[%d] = %lld < 1", who, i, (long long)numel[i]);
    *L = mt_layout(n, numel);
    D4_REQUIRE(L->nblocks < ((int64_t)1 << 31), "%s: too many elements", who);
    D4_REQUIRE(table && table_bytes >= L->bytes, "%s: table of %zu bytes, %zu needed (d4_multi_table_bytes)", who, table_bytes, L->bytes);
    D4_REQUIRE(((uintptr_t)table & 15) == 0, "%s: table must be 16-byte aligned", who);
    return 0;
}

}  // namespace d4

// ================================================================================================ plan (muon_plan.h)
namespace d4 {

static int muon_upload(d4_muon_plan* pl, hipStream_t s) {
    D4_HIP(hipMemcpyAsync(pl->tables, pl->mats.data(), sizeof(MuonMat) * pl->mats.size(), hipMemcpyHostToDevice, s));
    D4_HIP(hipStreamSynchronize(s));
    pl->uploaded = true;
    return 0;
}

// the fixed launch sequence of one call: per pass  prepare, [bf16 products: normalise,] steps x (gram, poly, apply), finish
static int muon_run(d4_muon_plan* pl, float* ws, const float* gnorm_sq, float max_norm, double beta, int nesterov, int steps, float a, float b, float c,
                    float eps, float decay, hipStream_t s) {
    const MuonMat* mats = reinterpret_cast<const MuonMat*>(pl->tables);
    float* partials = ws;
    float* work = ws + ((pl->part_floats + 63) & ~(size_t)63);
    for (const auto& ps : pl->passes) {
        const int2* prep = reinterpret_cast<const int2*>(pl->tables + ps.prep_off);
        const int4* sym = reinterpret_cast<const int4*>(pl->tables + ps.sym_off);
        const int4* full = reinterpret_cast<const int4*>(pl->tables + ps.full_off);
        hipLaunchKernelGGL(muon_prepare_kernel, dim3(ps.n_prep), dim3(256), 0, s, mats, prep, work, partials, gnorm_sq, max_norm, (float)beta, (float)(1. - beta), nesterov);
        D4_LAUNCH_CHECK();
        int cur = 0;
        if (pl->products == 1) {          // bf16 products: prepare wrote the fp32 u, normalise rounds X0 once, every buffer after it is bf16
            if (int rc = muon_bf16_normalise(mats, prep, ps.n_prep, work, partials, eps, s)) return rc;
            for (int it = 0; it < steps; ++it) {
                if (int rc = muon_bf16_product(mats, sym, ps.n_sym, work, 0, cur, 0.f, 1.f, s)) return rc;
                if (int rc = muon_bf16_product(mats, sym, ps.n_sym, work, 1, cur, b, c, s)) return rc;
                if (int rc = muon_bf16_product(mats, full, ps.n_full, work, 2, cur, a, 1.f, s)) return rc;
                cur ^= 1;
            }
            if (int rc = muon_bf16_finish(mats, prep, ps.n_prep, work, cur, decay, s)) return rc;
            continue;
        }
        for (int it = 0; it < steps; ++it) {
            const int first = it == 0;
            hipLaunchKernelGGL(muon_gemm_kernel<false>, dim3(ps.n_sym), dim3(256), 0, s, mats, sym, work, partials, 0, cur, 0.f, 1.f, first, eps);
            D4_LAUNCH_CHECK();
            hipLaunchKernelGGL(muon_gemm_kernel<false>, dim3(ps.n_sym), dim3(256), 0, s, mats, sym, work, partials, 1, cur, b, c, 0, eps);
            D4_LAUNCH_CHECK();
            hipLaunchKernelGGL(muon_gemm_kernel<true>, dim3(ps.n_full), dim3(256), 0, s, mats, full, work, partials, 2, cur, a, 1.f, first, eps);
            D4_LAUNCH_CHECK();
            cur ^= 1;
        }
        hipLaunchKernelGGL(muon_finish_kernel, dim3(ps.n_prep), dim3(256), 0, s, mats, prep, work, cur, decay);
        D4_LAUNCH_CHECK();
    }
    return 0;
}

static int muon_bind(d4_muon_plan* pl, const char* who, void* const* w, const void* const* g, void* const* m, void* const* out, const float* coef,
                     hipStream_t s) {
    const int n = (int)pl->mats.size();
    bool changed = !pl->uploaded;
    for (int i = 0; i < n; ++i) {
        D4_REQUIRE(g && g[i], "%s: input / gradient pointer %d is null", who, i);
        D4_REQUIRE(out && out[i], "%s: output / parameter pointer %d is null", who, i);
        if (m) D4_REQUIRE(m[i], "%s: exp_avg pointer %d is null", who, i);
        const void* now[4] = {w ? w[i] : nullptr, g[i], m ? m[i] : nullptr, out[i]};
        const float cf = coef ? coef[i] : 1.f;
        if (memcmp(now, &pl->last[4 * i], sizeof(now)) != 0 || cf != pl->last_coef[i]) changed = true;
        memcpy(&pl->last[4 * i], now, sizeof(now));
        pl->last_coef[i] = cf;
        MuonMat& d = pl->mats[i];
        d.w = (float*)now[0]; d.g = (const float*)now[1]; d.m = (float*)now[2]; d.out = (float*)now[3]; d.coef = cf;
    }
    return changed ? muon_upload(pl, s) : 0;
}

}  // namespace d4

extern "C" {

int d4_muon_plan_create(int n, const int32_t* rows, const int32_t* cols, size_t workspace_bytes, d4_muon_plan** out) {
    return d4::muon_plan_build("d4_muon_plan_create", n, rows, cols, workspace_bytes, 0, out);
}

int d4_muon_plan_create_products(int n, const int32_t* rows, const int32_t* cols, size_t workspace_bytes, int products, d4_muon_plan** out) {
    return d4::muon_plan_build("d4_muon_plan_create_products", n, rows, cols, workspace_bytes, products, out);
}

int d4_muon_plan_products(const d4_muon_plan* plan) { return plan ? plan->products : 0; }

void d4_muon_plan_destroy(d4_muon_plan* plan) {
    if (!plan) return;
    if (plan->tables) (void)hipFree(plan->tables);
    delete plan;
}

size_t d4_muon_plan_workspace_bytes(const d4_muon_plan* plan) {
    if (!plan) return 0;
    return ((plan->part_floats + 63) & ~(size_t)63) * 4 + plan->work_bytes;
}

int d4_muon_plan_passes(const d4_muon_plan* plan) { return plan ? (int)plan->passes.size() : 0; }

int d4_muon_step(d4_muon_plan* plan, void* const* params, const void* const* grads, void* const* exp_avg, const float* update_scale, void* workspace,
                 size_t workspace_bytes, double lr, double weight_decay, double beta, int nesterov, int steps, float a, float b, float c, float eps,
                 const float* grad_norm_sq, float max_grad_norm, void* stream) {
    using namespace d4;
    D4_REQUIRE(plan, "d4_muon_step: plan is null");
    D4_REQUIRE(params && grads && exp_avg && update_scale, "d4_muon_step: params, grads, exp_avg and update_scale");
    D4_REQUIRE(steps >= 1 && steps <= 64, "d4_muon_step: steps = %d outside 1 .. 64", steps);
    D4_REQUIRE(beta >= 0. && beta < 1., "d4_muon_step: beta = %g outside [0, 1)", beta);
    D4_REQUIRE(eps > 0.f, "d4_muon_step: eps must be positive");
    D4_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "d4_muon_step: workspace must be 256-byte aligned");
    D4_REQUIRE(workspace_bytes >= d4_muon_plan_workspace_bytes(plan), "d4_muon_step: workspace of %zu bytes, %zu needed", workspace_bytes,
               d4_muon_plan_workspace_bytes(plan));
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<float> coef(plan->mats.size());
    for (size_t i = 0; i < coef.size(); ++i) coef[i] = (float)(-lr * (double)update_scale[i]);
    if (int rc = muon_bind(plan, "d4_muon_step", params, grads, exp_avg, params, coef.data(), s)) return rc;
    return muon_run(plan, (float*)workspace, grad_norm_sq, max_grad_norm, beta, nesterov, steps, a, b, c, eps, (float)(1. - lr * weight_decay), s);
}

int d4_newton_schulz(d4_muon_plan* plan, const void* const* in, void* const* out, void* workspace, size_t workspace_bytes, int steps, float a, float b,
                     float c, float eps, void* stream) {
    using namespace d4;
    D4_REQUIRE(plan, "d4_newton_schulz: plan is null");
    D4_REQUIRE(in && out, "d4_newton_schulz: in and out");
    D4_REQUIRE(steps >= 1 && steps <= 64, "d4_newton_schulz: steps = %d outside 1 .. 64", steps);
    D4_REQUIRE(eps > 0.f, "d4_newton_schulz: eps must be positive");
    D4_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "d4_newton_schulz: workspace must be 256-byte aligned");
    D4_REQUIRE(workspace_bytes >= d4_muon_plan_workspace_bytes(plan), "d4_newton_schulz: workspace of %zu bytes, %zu needed", workspace_bytes,
               d4_muon_plan_workspace_bytes(plan));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = muon_bind(plan, "d4_newton_schulz", nullptr, in, nullptr, out, nullptr, s)) return rc;
    return muon_run(plan, (float*)workspace, nullptr, 0.f, 0., 0, steps, a, b, c, eps, 0.f, s);
}

size_t d4_multi_table_bytes(int n, const int64_t* numel) {
    if (n < 1 || !numel) return 0;
    return d4::mt_layout(n, numel).bytes;
}

int d4_sumsq_multi(int n, const int64_t* numel, const void* const* x, void* table, size_t table_bytes, int upload, float* out, void* stream) {
    using namespace d4;
    MtLayout L;
    if (int rc = mt_check("d4_sumsq_multi", n, numel, table, table_bytes, &L)) return rc;
    D4_REQUIRE(out, "d4_sumsq_multi: out is null");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (upload) {
        D4_REQUIRE(x, "d4_sumsq_multi: x is null");
        if (int rc = mt_upload("d4_sumsq_multi", n, numel, nullptr, x, nullptr, nullptr, table, L, s)) return rc;
    }
    const MtTensor* tab = reinterpret_cast<const MtTensor*>(table);
    const int32_t* owner = reinterpret_cast<const int32_t*>((char*)table + L.owner_off);
    float* partials = reinterpret_cast<float*>((char*)table + L.part_off);
    hipLaunchKernelGGL(mt_sumsq_kernel, dim3((unsigned)L.nblocks), dim3(256), 0, s, tab, owner, partials);
    D4_LAUNCH_CHECK();
    hipLaunchKernelGGL(mt_sumsq_final_kernel, dim3(1), dim3(256), 0, s, partials, (int)L.nblocks, out);
    D4_LAUNCH_CHECK();
    return 0;
}

int d4_adam_atan2_multi(int n, const int64_t* numel, void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, void* table,
                        size_t table_bytes, int upload, int step, double lr, double beta1, double beta2, double weight_decay, double a, double b,
                        const float* grad_norm_sq, float max_grad_norm, void* stream) {
    using namespace d4;
    MtLayout L;
    if (int rc = mt_check("d4_adam_atan2_multi", n, numel, table, table_bytes, &L)) return rc;
    D4_REQUIRE(step >= 1, "d4_adam_atan2_multi: step = %d (counts from 1)", step);
    D4_REQUIRE(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1., "d4_adam_atan2_multi: betas outside [0, 1)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (upload) {
        D4_REQUIRE(params && grads && exp_avg && exp_avg_sq, "d4_adam_atan2_multi: params, grads, exp_avg and exp_avg_sq");
        if (int rc = mt_upload("d4_adam_atan2_multi", n, numel, params, grads, exp_avg, exp_avg_sq, table, L, s)) return rc;
    }
    const MtTensor* tab = reinterpret_cast<const MtTensor*>(table);
    const int32_t* owner = reinterpret_cast<const int32_t*>((char*)table + L.owner_off);
    const float inv_bc1 = (float)(1. / (1. - pow(beta1, step))), inv_bc2 = (float)(1. / (1. - pow(beta2, step)));
    hipLaunchKernelGGL(mt_adam_atan2_kernel, dim3((unsigned)L.nblocks), dim3(256), 0, s, tab, owner, grad_norm_sq, max_grad_norm, (float)(1. - beta1),
                       (float)(1. - beta2), (float)(1. - lr * weight_decay), (float)(lr * a), (float)b, inv_bc1, inv_bc2);
    D4_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
