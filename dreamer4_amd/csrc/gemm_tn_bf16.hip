// Weight-gradient GEMM of the bf16 training arithmetic:  C[M][N] (fp32) = sum_k A[k][M] * B[k][N]
// with A = bf16(dY) [rows][lda] and B = bf16(X) [rows][ldb] row-major bf16 images: the contraction index k (token rows) is the SLOW index
// of both operands, while v_mfma_f32_16x16x32_bf16 wants every lane to hold 8 consecutive k of ONE output row / column.  gemm_tn.hip's trick
// (a float4 along the fast index feeds four different MFMAs) does not carry over, so here the transpose is done by the LDS read:
//
//   global --16-byte row loads--> VGPR --ds_write_b128--> LDS tile [32 k rows][128 columns] as it lies in memory (256-byte rows, chunks XOR-swizzled)
//   LDS --ds_read_b64_tr_b16--> MFMA operand: a group of 16 lanes reads a 4 (k) x 16 (column) block and every lane receives ONE column's 4 k values,
//   two such reads (k rows 8g .. 8g+3 and 8g+4 .. 8g+7 for lane group g) are the 8 k values of the lane's column.
//
// Both operands are read the same way, so the order of the 32 k rows inside one MFMA is the same permutation for A and B (a sum over k does
// not care).  No transposed copy of dY or X exists in HBM and no VALU instruction moves data between lanes.
//
// LDS image (per stage and operand: 32 rows x 256 B = 8 KB; 2 stages x 2 operands = 32 KB): byte offset of 16-byte chunk ch of row r
//   off(r, ch) = 256 r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))).
// Bank conflicts (bank = (byte / 4) % 64 for ds_read_b64_tr_b16, counted per 32-lane half): lane 4q + p of group g addresses row 8g + 4h + q,
// chunk c0 + (p >> 1) (c0 even), half-chunk p & 1.  A row is exactly 64 banks, so the bank is 4 pos + 2 (p & 1) + {0, 1} with
// pos = (c0 + (p >> 1)) ^ ((q << 2) | ((2g + h) & 3)): bit 0 = (p >> 1) ^ h, bit 1 = c0's ^ (g & 1), bits 2-3 = c0's ^ q; h is fixed per
// instruction.  Over the 32 lanes of a half (g & 1, q, p) that is 16 different chunks x 2 half-chunks = all 64 banks once: conflict-free
// (without the XOR all 8 rows of a half would share 8 banks, 8-way).  (Computed from the bank rule; no SQ_LDS_BANK_CONFLICT run is recorded.)
// The ds_write_b128 of a wave covers 4 whole rows; the XOR moves aligned 64-byte quarters inside a row, so every 8 consecutive lanes still write one aligned 128-byte run = all 32 write banks once.
//
// Every lane of every wave issues every transposed read with an in-bounds address (the tile is always whole in LDS; rows past the k slice and
// columns past the matrix are ZERO-FILLED on the way in, never masked at the read): EXEC is all ones as the instruction requires.
//
// Work split: a workgroup of 4 waves (2 x 2) owns a 128 x 128 output tile, a wave 64 x 64 = 4 x 4 MFMA tiles (64 accumulator registers).
// k is split over the grid's y dimension into slices by a rule on the shape; the slices' partial tiles are added in slice order by
// splitk_reduce, so the result is reproducible bit for bit.
#include "common.h"
#include "kernels.h"
#include "../../include/d4hip.h"

namespace d4 {

struct TnbArgs {
    const uint16_t* A; int lda;    // [K][lda] bf16, M columns used
    const uint16_t* B; int ldb;    // [K][ldb] bf16, N columns used
    float* C; int ldc;             // slice z writes C + z * strideC
    int64_t strideC;
    int M, N, K, kslice;           // slice z covers rows [z * kslice, min(K, (z + 1) * kslice)); kslice % 32 == 0
};

typedef uint32_t tnb_u4 __attribute__((ext_vector_type(4)));
typedef short tnb_s4 __attribute__((ext_vector_type(4)));
typedef short tnb_s8 __attribute__((ext_vector_type(8)));
typedef __bf16 tnb_b8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) tnb_s4* tnb_lds_s4;

constexpr int TNB_T = 128, TNB_BK = 32, TNB_OP = TNB_BK * 256;       // output tile edge; k rows per stage; bytes per operand tile

__device__ __forceinline__ int tnb_off(int r, int ch) { return 256 * r + 16 * (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))); }

__global__ __launch_bounds__(256) void gemm_tn_bf16_kernel(TnbArgs p) {
    __shared__ __attribute__((aligned(16))) char tile[2 * 2 * TNB_OP];       // [stage][A | B][32][256 B]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_n = (p.N + TNB_T - 1) / TNB_T;
    const int m0 = (blockIdx.x / tiles_n) * TNB_T, n0 = (blockIdx.x % tiles_n) * TNB_T;
    const int kbeg = blockIdx.y * p.kslice, kend = min(p.K, kbeg + p.kslice);
    const int nk = (kend - kbeg + TNB_BK - 1) / TNB_BK;

    // global -> LDS: 512 chunks of 16 bytes per operand tile, two per thread (chunk c: row c >> 4, 8 columns at 8 (c & 15))
    const int lrow = tid >> 4, lch = tid & 15;                                // rows lrow and lrow + 16
    const bool oka = m0 + 8 * lch < ((p.M + 7) & ~7), okb = n0 + 8 * lch < ((p.N + 7) & ~7);      // (lda, ldb >= the rounded widths: host check)
    const uint16_t* ga = p.A + (int64_t)(kbeg + lrow) * p.lda + (oka ? m0 + 8 * lch : 0);
    const uint16_t* gb = p.B + (int64_t)(kbeg + lrow) * p.ldb + (okb ? n0 + 8 * lch : 0);
    const int st0 = tnb_off(lrow, lch), st1 = tnb_off(lrow + 16, lch);
    tnb_u4 ra[2], rb[2];
    // raw loads from an address that is always valid (rows past the slice read row kbeg, columns past the matrix column 0); what must be zero is
    // zeroed where the registers are written to LDS, so that a load never waits on a branch
    auto gload = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t ro = kbeg + kt * TNB_BK + lrow + 16 * i < kend ? (int64_t)(kt * TNB_BK + 16 * i) : (int64_t)-lrow;
            ra[i] = *reinterpret_cast<const tnb_u4*>(ga + ro * p.lda);
            rb[i] = *reinterpret_cast<const tnb_u4*>(gb + ro * p.ldb);
        }
    };
    auto lstore = [&](int buf, int kt) {
        char* st = tile + buf * 2 * TNB_OP;
        const tnb_u4 zero4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool rok = kbeg + kt * TNB_BK + lrow + 16 * i < kend;
            *reinterpret_cast<tnb_u4*>(st + (i ? st1 : st0)) = (rok && oka) ? ra[i] : zero4;
            *reinterpret_cast<tnb_u4*>(st + TNB_OP + (i ? st1 : st0)) = (rok && okb) ? rb[i] : zero4;
        }
    };

    // transposed-read addresses: lane 4q + pp of group g supplies row 8g + 4h + q, columns 16 i + 4 pp .. + 3 of the wave's 64-column strip
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    int adr_a[4][2], adr_b[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = 8 * g + 4 * h + q;
            adr_a[i][h] = tnb_off(r, wm * 8 + 2 * i + (pp >> 1)) + 8 * (pp & 1);
            adr_b[i][h] = TNB_OP + tnb_off(r, wn * 8 + 2 * i + (pp >> 1)) + 8 * (pp & 1);
        }

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto frag = [&](const char* st, int adr0, int adr1) {
        const tnb_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tnb_lds_s4)(st + adr0));
        const tnb_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tnb_lds_s4)(st + adr1));
        const tnb_s8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(tnb_b8, v);
    };

    gload(0);
    lstore(0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;                      // (uniform over the workgroup: the transposed reads below run with every lane on)
        if (more) gload(kt + 1);
        const char* st = tile + (kt & 1) * 2 * TNB_OP;
        tnb_b8 fa[4], fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { fa[i] = frag(st, adr_a[i][0], adr_a[i][1]); fb[i] = frag(st, adr_b[i][0], adr_b[i][1]); }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        if (more) lstore((kt + 1) & 1, kt + 1);
        __syncthreads();
    }

    // D[r'][c']: r' (first operand = B column n) = 4 (lane >> 4) + reg, c' (second operand = A column m) = lane & 15: four consecutive n per lane
    float* C = p.C + blockIdx.y * p.strideC;
    const bool vec = (p.ldc % 4) == 0 && (reinterpret_cast<uintptr_t>(C) % 16) == 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = m0 + wm * 64 + 16 * i + (lane & 15);
        if (row >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + wn * 64 + 16 * j + 4 * g;
            if (col >= p.N) continue;
            float* cp = C + (int64_t)row * p.ldc + col;
            if (vec && col + 3 < p.N) *reinterpret_cast<f32x4*>(cp) = acc[i][j];
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (col + e < p.N) cp[e] = acc[i][j][e];
            }
        }
    }
}

bool gemm_tn_bf16_applicable(const uint16_t* A, int lda, const uint16_t* B, int ldb, const float* C, int ldc, int M, int N, int K) {
    return A && B && C && M >= 1 && N >= 1 && K >= 1 && lda % 8 == 0 && ldb % 8 == 0 && lda >= ((M + 7) & ~7) && ldb >= ((N + 7) & ~7) && ldc >= N &&
           (reinterpret_cast<uintptr_t>(A) & 15) == 0 && (reinterpret_cast<uintptr_t>(B) & 15) == 0 && (reinterpret_cast<uintptr_t>(C) & 3) == 0;
}

// Slice count: a rule on the shape only.  tiles x slices of about 512 workgroups (two per CU), at most 16 slices, every slice at least 256
// contraction rows (below that the partial tiles' traffic outweighs the k loop), partial products within `part`.
int gemm_tn_bf16_slices(int M, int N, int K, size_t part_floats) {
    const int64_t tiles = (int64_t)cdiv(M, TNB_T) * cdiv(N, TNB_T);
    int64_t S = (512 + tiles / 2) / tiles;
    if (S > 16) S = 16;
    if (S > K / 256) S = K / 256;
    if (S > 1 && (size_t)S * M * N > part_floats) S = (int64_t)(part_floats / ((size_t)M * N));
    return S < 1 ? 1 : (int)S;
}

int gemm_tn_bf16(const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc, int M, int N, int K, float* part, size_t part_floats, hipStream_t s,
                 int forced_slices) {
    D4_REQUIRE(gemm_tn_bf16_applicable(A, lda, B, ldb, C, ldc, M, N, K),
               "gemm_tn_bf16: leading dimensions of the bf16 images must be multiples of 8 covering M / N rounded up to 8, the images 16-byte aligned");
    int S = forced_slices > 0 ? forced_slices : gemm_tn_bf16_slices(M, N, K, part ? part_floats : 0);
    D4_REQUIRE(S == 1 || (part && (size_t)S * M * N <= part_floats), "gemm_tn_bf16: %d slices need %zu floats of scratch", S, (size_t)S * M * N);
    const int ks = cdiv(cdiv(K, S), TNB_BK) * TNB_BK;
    S = cdiv(K, ks);
    TnbArgs p{A, lda, B, ldb, S > 1 ? part : C, S > 1 ? N : ldc, S > 1 ? (int64_t)M * N : 0, M, N, K, ks};
    hipLaunchKernelGGL(gemm_tn_bf16_kernel, dim3(cdiv(M, TNB_T) * cdiv(N, TNB_T), S), dim3(256), 0, s, p);
    D4_LAUNCH_CHECK();
    if (S > 1) return splitk_reduce(part, S, M, N, nullptr, 0, C, ldc, s);
    return 0;
}

// ---- bf16 operand images of the training arithmetic: fp32 -> bf16 (round to nearest even) with the columns [cols, cols_pad) written as zeros
__global__ __launch_bounds__(256) void cvt_pad_bf16_kernel(const float* __restrict__ src, int64_t lds_, uint16_t* __restrict__ dst, int64_t ldd, int rows, int cols,
                                                           int cols_pad) {
    const int per = cols_pad / 8;
    const int64_t tot = (int64_t)rows * per;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per;
        const int c = (int)(i % per) * 8;
        const float* sp = src + r * lds_ + c;
        uint32_t o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lo = c + 2 * e < cols ? sp[2 * e] : 0.f, hi = c + 2 * e + 1 < cols ? sp[2 * e + 1] : 0.f;
            o[e] = (uint32_t)bf16_bits(lo) | ((uint32_t)bf16_bits(hi) << 16);
        }
        *reinterpret_cast<uint4*>(dst + r * ldd + c) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}
int cvt_pad_bf16(const float* src, int64_t lds_, uint16_t* dst, int64_t ldd, int rows, int cols, int cols_pad, hipStream_t s) {
    D4_REQUIRE(src && dst && cols_pad % 8 == 0 && cols_pad >= cols && ldd % 8 == 0 && ldd >= cols_pad && (reinterpret_cast<uintptr_t>(dst) & 15) == 0,
               "cvt_pad_bf16: bad arguments");
    if (rows == 0 || cols_pad == 0) return 0;
    const int64_t tot = (int64_t)rows * (cols_pad / 8);
    hipLaunchKernelGGL(cvt_pad_bf16_kernel, dim3((unsigned)((tot + 255) / 256 < 8192 ? (tot + 255) / 256 : 8192)), dim3(256), 0, s, src, lds_, dst, ldd, rows, cols, cols_pad);
    D4_LAUNCH_CHECK();
    return 0;
}

// dst[c][r] = bf16(src[r][c]) for r < rows_pad (zeros for r >= rows), c < cols: the transposed weight image of the input-gradient product
__global__ __launch_bounds__(256) void cvt_transpose_bf16_kernel(const float* __restrict__ src, int lds_, uint16_t* __restrict__ dst, int ldd, int rows, int cols,
                                                                 int rows_pad) {
    __shared__ float t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        t[ty + 8 * i][tx] = (r < rows && c < cols) ? src[(int64_t)r * lds_ + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (c < cols && r < rows_pad) dst[(int64_t)c * ldd + r] = bf16_bits(t[tx][ty + 8 * i]);
    }
}
int cvt_transpose_bf16(const float* src, int lds_, uint16_t* dst, int ldd, int rows, int cols, int rows_pad, hipStream_t s) {
    D4_REQUIRE(src && dst && rows_pad >= rows && ldd >= rows_pad, "cvt_transpose_bf16: bad arguments");
    if (rows_pad == 0 || cols == 0) return 0;
    hipLaunchKernelGGL(cvt_transpose_bf16_kernel, dim3((cols + 31) / 32, (rows_pad + 31) / 32), dim3(256), 0, s, src, lds_, dst, ldd, rows, cols, rows_pad);
    D4_LAUNCH_CHECK();
    return 0;
}

}  // namespace d4

extern "C" int d4_gemm_tn_bf16(const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc, int M, int N, int K, float* part, int64_t part_floats,
                               int slices, void* stream) {
    return d4::gemm_tn_bf16(A, lda, B, ldb, C, ldc, M, N, K, part, part ? (size_t)part_floats : 0, static_cast<hipStream_t>(stream), slices);
}

// Operator-level test entry points of the bf16 image builders above: the launchers check their own arguments.
extern "C" int d4_cvt_pad_bf16(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int rows, int cols, int cols_pad, void* stream) {
    D4_REQUIRE(rows >= 0 && cols >= 0 && lds >= cols, "d4_cvt_pad_bf16: bad arguments");
    return d4::cvt_pad_bf16(src, lds, dst, ldd, rows, cols, cols_pad, static_cast<hipStream_t>(stream));
}
extern "C" int d4_cvt_transpose_bf16(const float* src, int lds, uint16_t* dst, int ldd, int rows, int cols, int rows_pad, void* stream) {
    D4_REQUIRE(rows >= 0 && cols >= 0 && lds >= cols, "d4_cvt_transpose_bf16: bad arguments");
    return d4::cvt_transpose_bf16(src, lds, dst, ldd, rows, cols, rows_pad, static_cast<hipStream_t>(stream));
}
