// MuonAdamAtan2, Newton-Schulz on the bf16 matrix pipe (opt-in per plan: d4_muon_plan_create_products(..., 1, ...)).
//
//   prepare     the fp32 form's own kernel (csrc/muon.hip), unchanged: momentum, Nesterov u, strip partials of sum u^2, u in fp32 into the region at x0
//   normalise   X0 = bf16(u * 1 / max(|u|_F, eps)): scaled in fp32, rounded once; written as X [Rp][Cp] AND its transposed image X^T [Cp][Rp]
//   gram        A  = bf16(X X^T)                   (upper tiles, mirrored)
//   poly        B  = bf16(b A + c A A^T)           (upper tiles, mirrored; A is symmetric bit for bit)
//   apply       X' = bf16(a X + B X)               computed as B (X^T)^T: X' and X'^T both written
//   finish      W <- W (1 - lr wd) - lr s X        fp32, from the bf16 X (from X^T for a transposed matrix: no transpose left to do)
// Because every X carries its transposed image, all three products are  D[m][n] = sum_k P[m][k] Q[n][k]  on [row][k] operands: ONE kernel, no layout
// template.  A workgroup of 4 waves owns a 128 x 128 tile (2 x 2 v_mfma_f32_32x32x16_bf16 tiles per wave), k-tiles of 64 staged global -> registers
// -> LDS one tile ahead; the operands are bf16 in memory, so the k-loop converts nothing and a lane's 8 consecutive k are one 16-byte LDS read.
// The epilogue is alpha * E + beta * acc in fp32 on the widened bf16 E, rounded once (v_cvt_pk_bf16_f32, nearest even) on the store.  E is read, and
// the mirrored / transposed tile written, as 4 consecutive rows of a lane = one packed 8-byte access of the transposed image.
// Every dimension is a multiple of 128 with zero pads that stay zero, so the products carry no bounds logic.  No atomics, fixed k order.
#include <math.h>

#include "../../include/d4hip.h"
#include "common.h"
#include "muon_plan.h"

namespace d4 {

namespace {

constexpr int MB_BK = 64;             // k-tile (bf16 elements)
constexpr int MB_LD = MB_BK + 8;      // LDS row stride: 144 bytes, so the 16-byte fragment reads of 16 consecutive rows cover all 64 banks once

typedef __bf16 mb_b8 __attribute__((ext_vector_type(8)));
typedef __bf16 mb_b4 __attribute__((ext_vector_type(4)));

// the bf16 X of region `cur` (0: at x1, 1: at x0); its transposed image follows it
__device__ __forceinline__ __bf16* mb_x(const MuonMat& d, float* ws, int cur) { return reinterpret_cast<__bf16*>(ws + (cur ? d.x0 : d.x1)); }
__device__ __forceinline__ const __bf16* mb_x(const MuonMat& d, const float* ws, int cur) { return reinterpret_cast<const __bf16*>(ws + (cur ? d.x0 : d.x1)); }

// ---------------------------------------------------------------------------------------------- normalise
// blocks: prepare's int2 (matrix, strip).  The strip is 32 rows of the padded ORIGINAL matrix: 32 rows of the oriented image, or 32 of its columns
// for a transposed matrix.  Reads the fp32 u (region at x0), writes X and X^T of region 0 (at x1), pads included.
__global__ __launch_bounds__(256) void muon_bf16_normalise_kernel(const MuonMat* mats, const int2* blocks, float* ws, const float* partials, float eps) {
    __shared__ __bf16 tile[32][34];
    __shared__ float s_scale;
    const int2 bk = blocks[blockIdx.x];
    const MuonMat d = mats[bk.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {                                                          // the fp32 form's scale: strip partials in fixed order
        float s = 0.f;
        for (int i = lane; i < d.nparts; i += 64) s += partials[d.part0 + i];
        s = wave_sum(s);
        if (lane == 0) s_scale = 1.f / fmaxf(sqrtf(s), eps);
    }
    __syncthreads();
    const float sc = s_scale;
    const float* U = ws + d.x0;
    __bf16* X = mb_x(d, ws, 0);
    __bf16* XT = X + (int64_t)d.Rp * d.Cp;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int walk = d.transposed ? d.Rp : d.Cp;
    for (int j0 = 0; j0 < walk; j0 += 32) {
        const int ri = d.transposed ? j0 : bk.y * MU_STRIP, cj = d.transposed ? bk.y * MU_STRIP : j0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t at = (int64_t)(ri + ty + 8 * q) * d.Cp + cj + tx;
            const __bf16 h = (__bf16)(U[at] * sc);
            X[at] = h;
            tile[ty + 8 * q][tx] = h;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) XT[(int64_t)(cj + ty + 8 * q) * d.Rp + ri + tx] = tile[tx][ty + 8 * q];
    }
}

// ---------------------------------------------------------------------------------------------- the three products
// tiles: int4 (matrix, tile row, tile col, 0).  stage 0: A = X X^T; 1: B = alpha A + beta A A^T; 2: X' = alpha X + beta B X (and X'^T).
__global__ __launch_bounds__(256) void muon_bf16_gemm_kernel(const MuonMat* mats, const int4* tiles, float* ws, int stage, int cur, float alpha, float beta) {
    __shared__ __attribute__((aligned(16))) __bf16 sP[MU_T * MB_LD];
    __shared__ __attribute__((aligned(16))) __bf16 sQ[MU_T * MB_LD];
    const int4 t = tiles[blockIdx.x];
    const MuonMat d = mats[t.x];
    __bf16* Xc = mb_x(d, ws, cur);
    __bf16* Xn = mb_x(d, ws, cur ^ 1);
    const int64_t xsz = (int64_t)d.Rp * d.Cp;
    __bf16* A = reinterpret_cast<__bf16*>(ws + d.a);
    __bf16* B = reinterpret_cast<__bf16*>(ws + d.b);
    const __bf16 *P, *Q, *ET;                    // ET: the epilogue's E through its transposed image, E[row][col] = ET[col * Rp + row]
    __bf16 *D, *DT;                              // DT: the transposed image of D, leading dimension Rp in every stage
    int ldp, ldq, ldd, K;
    if (stage == 0) { P = Xc; Q = Xc; ET = nullptr; D = A; DT = A; ldp = ldq = d.Cp; ldd = d.Rp; K = d.Cp; }
    else if (stage == 1) { P = A; Q = A; ET = A; D = B; DT = B; ldp = ldq = ldd = d.Rp; K = d.Rp; }
    else { P = B; Q = Xc + xsz; ET = Xc + xsz; D = Xn; DT = Xn + xsz; ldp = ldq = d.Rp; ldd = d.Cp; K = d.Rp; }
    const int ldt = d.Rp;
    const int m0 = t.y * MU_T, n0 = t.z * MU_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    mb_b8 pv[4], qv[4];
    const int frow = tid >> 3, fk = (tid & 7) * 8;               // 32 rows x 8 chunks of 8 k per round, 4 rounds per operand
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            pv[h] = *reinterpret_cast<const mb_b8*>(P + (int64_t)(m0 + frow + 32 * h) * ldp + k0 + fk);
            qv[h] = *reinterpret_cast<const mb_b8*>(Q + (int64_t)(n0 + frow + 32 * h) * ldq + k0 + fk);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            *reinterpret_cast<mb_b8*>(sP + (frow + 32 * h) * MB_LD + fk) = pv[h];
            *reinterpret_cast<mb_b8*>(sQ + (frow + 32 * h) * MB_LD + fk) = qv[h];
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
    const __bf16* fa = sP + (wm + l31) * MB_LD + 8 * lh;         // lane l holds row l & 31, k = 8 (l >> 5) .. + 7 of a 16-deep step
    const __bf16* fb = sQ + (wn + l31) * MB_LD + 8 * lh;

    fetch(0);
    for (int k0 = 0; k0 < K; k0 += MB_BK) {
        __syncthreads();
        stash();
        __syncthreads();
        if (k0 + MB_BK < K) fetch(k0 + MB_BK);
#pragma unroll
        for (int kk = 0; kk < MB_BK; kk += 16) {
            const mb_b8 a0 = *reinterpret_cast<const mb_b8*>(fa + kk), a1 = *reinterpret_cast<const mb_b8*>(fa + 32 * MB_LD + kk);
            const mb_b8 b0 = *reinterpret_cast<const mb_b8*>(fb + kk), b1 = *reinterpret_cast<const mb_b8*>(fb + 32 * MB_LD + kk);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        }
    }

    // epilogue: D = alpha * E + beta * acc, rounded once.  Registers 4g .. 4g + 3 of a lane are 4 consecutive rows of one column: one packed 8-byte
    // access of the transposed image, for E (stage 1: A is symmetric; stage 2: X^T) and for the mirrored tile / X'^T.
    const bool tr = stage == 2 || t.y != t.z;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn + 32 * j + l31;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = m0 + wm + 32 * i + 8 * g + 4 * lh;
                mb_b4 e, o;
                if (ET) e = *reinterpret_cast<const mb_b4*>(ET + (int64_t)col * ldt + row);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = beta * acc[i][j][4 * g + r];
                    if (ET) v += alpha * (float)e[r];
                    o[r] = (__bf16)v;
                    D[(int64_t)(row + r) * ldd + col] = o[r];
                }
                if (tr) *reinterpret_cast<mb_b4*>(DT + (int64_t)col * ldt + row) = o;
            }
        }
}

// ---------------------------------------------------------------------------------------------- finish
// blocks: prepare's int2 (matrix, strip of 32 original rows).  A transposed matrix reads X^T, which is its own orientation.
__global__ __launch_bounds__(256) void muon_bf16_finish_kernel(const MuonMat* mats, const int2* blocks, const float* ws, int cur, float decay) {
    const int2 bk = blocks[blockIdx.x];
    const MuonMat d = mats[bk.x];
    const int i0 = bk.y * MU_STRIP;
    if (i0 >= d.r) return;                                                    // a strip of padding only (uniform for the workgroup)
    const __bf16* X = mb_x(d, ws, cur) + (d.transposed ? (int64_t)d.Rp * d.Cp : 0);
    const int ld = d.transposed ? d.Rp : d.Cp;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j0 = 0; j0 < d.c; j0 += 32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + ty + 8 * q, j = j0 + tx;
            if (i < d.r && j < d.c) {
                const float x = (float)X[(int64_t)i * ld + j];
                const int64_t at = (int64_t)i * d.c + j;
                d.out[at] = d.w ? d.w[at] * decay + d.coef * x : d.coef * x;
            }
        }
    }
}

}  // namespace

int muon_bf16_normalise(const MuonMat* mats, const int2* blocks, int nblocks, float* work, const float* partials, float eps, hipStream_t s) {
    hipLaunchKernelGGL(muon_bf16_normalise_kernel, dim3(nblocks), dim3(256), 0, s, mats, blocks, work, partials, eps);
    D4_LAUNCH_CHECK();
    return 0;
}

int muon_bf16_product(const MuonMat* mats, const int4* tiles, int ntiles, float* work, int stage, int cur, float alpha, float beta, hipStream_t s) {
    hipLaunchKernelGGL(muon_bf16_gemm_kernel, dim3(ntiles), dim3(256), 0, s, mats, tiles, work, stage, cur, alpha, beta);
    D4_LAUNCH_CHECK();
    return 0;
}

int muon_bf16_finish(const MuonMat* mats, const int2* blocks, int nblocks, const float* work, int cur, float decay, hipStream_t s) {
    hipLaunchKernelGGL(muon_bf16_finish_kernel, dim3(nblocks), dim3(256), 0, s, mats, blocks, work, cur, decay);
    D4_LAUNCH_CHECK();
    return 0;
}

}  // namespace d4
