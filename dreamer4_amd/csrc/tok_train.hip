// Pixel-side operators of the VideoTokenizer training forward (dreamer4.py:4239-4603): the passes that read or write
// B T H W C floats and that torch would run as five or six elementwise kernels per step.
//
//   flow_noised_patches   patch rows of noise.lerp(video, t[b]) (no noise: of the video)   D4:4457 + 3896   one read of each, one write
//   layernorm_rows_bwd    backward of LayerNorm without bias: dx per row, d gamma       D4:3842 / 3898
//   mask_rows_fwd / _bwd  rows replaced by the mask token (MAE masking) and its backward D4:4344
//   recon_loss_fwd_bwd    mean squared error of the decoder's patch rows against the video read through the patch permutation (v-space or
//                         x-space), and d loss / d patch rows in the same pass            D4:4469-4474, 4516
//
// Every column sum and the loss sum run as per-block partials in a caller-provided scratch, then ONE reduction in a fixed order (no float
// atomics): the same inputs give the same bits.  Plain HIP C++; rows are read and written as float4 (dim % 4 == 0, patch row % 4 == 0).
#include "common.h"
#include "kernels.h"

namespace d4 {

// torch's lerp (ATen/native/Lerp.h): the form that is exact at both ends, so t = 1 gives the video's own bits and t = 0 the noise's
__device__ __forceinline__ float lerp_t(float a, float b, float w) {
    const float d = b - a;
    return w < 0.5f ? a + w * d : b - d * (1.f - w);
}

// float4 i of the patch row layout [(b t h w)][(p1 p2 c)] -> the video indices (b c t (h p1) (w p2)) of its four elements.  32-bit index arithmetic
// (the entry points refuse more than 2^31 float4s): six divisions per float4, the elements inside it by carrying (c, p2, p1).
struct PatchGeom {
    int C, T, nh, nw, ps, dp4;
    __device__ __forceinline__ void video_indices(uint32_t i, int64_t (&v)[4], int& b) const {
        uint32_t r = i / (uint32_t)dp4;
        const uint32_t e = (i - r * (uint32_t)dp4) * 4u;
        uint32_t q = e / (uint32_t)C;
        int c = (int)(e - q * (uint32_t)C);
        int p1 = (int)(q / (uint32_t)ps), p2 = (int)(q - (uint32_t)p1 * (uint32_t)ps);
        const int w = (int)(r % (uint32_t)nw); r /= (uint32_t)nw;
        const int h = (int)(r % (uint32_t)nh); r /= (uint32_t)nh;
        const int t = (int)(r % (uint32_t)T);
        b = (int)(r / (uint32_t)T);
        const int64_t W = (int64_t)nw * ps, plane = (int64_t)T * nh * ps * W;              // one channel of one clip
        const int64_t base = (((int64_t)b * C * T + t) * (nh * ps) + (int64_t)h * ps) * W + (int64_t)w * ps;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = base + c * plane + p1 * W + p2;
            if (++c == C) { c = 0; if (++p2 == ps) { p2 = 0; ++p1; } }
        }
    }
};

static inline dim3 grid4(int64_t n4, int cap) {
    int64_t g = (n4 + 255) / 256;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return dim3((unsigned)g);
}

// ------------------------------------------------------------------------------------ noised patch rows
// NOISED false: the video's own patch rows (what video_to_patches writes, on this kernel's index arithmetic)
template <bool NOISED>
__global__ __launch_bounds__(256) void flow_noised_patches_kernel(const float* video, const float* noise, const float* t, float* rows, PatchGeom g, int64_t n4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 o;
        int64_t v[4];
        int b;
        g.video_indices((uint32_t)i, v, b);
        const float tb = NOISED ? t[b] : 1.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = NOISED ? lerp_t(noise[v[u]], video[v[u]], tb) : video[v[u]];
        *reinterpret_cast<f32x4*>(rows + i * 4) = o;
    }
}

int flow_noised_patches(const float* video, const float* noise, const float* t, float* rows, int B, int C, int T, int nh, int nw, int ps, hipStream_t s) {
    const int64_t n = (int64_t)B * C * T * nh * ps * nw * ps;
    if (n == 0) return 0;
    const PatchGeom g{C, T, nh, nw, ps, C * ps * ps / 4};
    if (noise) hipLaunchKernelGGL(flow_noised_patches_kernel<true>, grid4(n / 4, 4096), dim3(256), 0, s, video, noise, t, rows, g, n / 4);
    else hipLaunchKernelGGL(flow_noised_patches_kernel<false>, grid4(n / 4, 4096), dim3(256), 0, s, video, noise, t, rows, g, n / 4);
    D4_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------ row tiles with a column-sum partial
// A block owns TOK_ROW_TILE consecutive rows (few: the rows of a wave are a chain of dependent reductions, so parallelism comes from blocks), one wave
// every fourth of them; lane l holds columns 4 l + 256 j (j < TOK_NJ) of a row as float4.
// The four waves' column partials meet in LDS and are added in wave order into part[block][dim].
static constexpr int TOK_NJ = 4;                       // dim <= 1024

__device__ __forceinline__ void block_colsum_store(const f32x4 (&acc)[TOK_NJ], float* part_row, int dim) {
    __shared__ f32x4 sh[4][TOK_NJ * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < TOK_NJ; ++j) sh[wave][j * 64 + lane] = acc[j];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int j = 0; j < TOK_NJ; ++j) {
            const int c = 4 * lane + 256 * j;
            if (c < dim) {
                const f32x4 v = ((sh[0][j * 64 + lane] + sh[1][j * 64 + lane]) + sh[2][j * 64 + lane]) + sh[3][j * 64 + lane];
                *reinterpret_cast<f32x4*>(part_row + c) = v;
            }
        }
    }
}

// y = xhat * g, xhat = (x - mean) * rstd:  d g = sum_r dy xhat;  dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat))
__global__ __launch_bounds__(256) void layernorm_rows_bwd_kernel(const float* x, int ldx, const float* dy, const float* g, float* dx, float* part, int rows,
                                                                 int dim, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * TOK_ROW_TILE, r1 = min(rows, r0 + TOK_ROW_TILE);
    f32x4 acc[TOK_NJ], gv[TOK_NJ];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < TOK_NJ; ++j) {
        const int c = 4 * lane + 256 * j;
        acc[j] = zero;
        gv[j] = c < dim ? *reinterpret_cast<const f32x4*>(g + c) : zero;
    }
    const float inv_d = 1.f / (float)dim;
    for (int r = r0 + wave; r < r1; r += 4) {
        f32x4 xv[TOK_NJ], dv[TOK_NJ];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < TOK_NJ; ++j) {
            const int c = 4 * lane + 256 * j;
            xv[j] = c < dim ? *reinterpret_cast<const f32x4*>(x + (int64_t)r * ldx + c) : zero;
            dv[j] = c < dim ? *reinterpret_cast<const f32x4*>(dy + (int64_t)r * dim + c) : zero;
            sum += (xv[j][0] + xv[j][1]) + (xv[j][2] + xv[j][3]);
        }
        const float mean = wave_sum(sum) * inv_d;
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < TOK_NJ; ++j) {
            const int c = 4 * lane + 256 * j;
            if (c < dim) {
                xv[j] -= mean;
                ss += (xv[j][0] * xv[j][0] + xv[j][1] * xv[j][1]) + (xv[j][2] * xv[j][2] + xv[j][3] * xv[j][3]);
            }
        }
        const float rstd = rsqrtf(wave_sum(ss) * inv_d + eps);
        float m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int j = 0; j < TOK_NJ; ++j) {
            xv[j] *= rstd;                              // xhat (zero in the columns past dim)
            acc[j] += dv[j] * xv[j];
            dv[j] *= gv[j];                             // g dy
            m1 += (dv[j][0] + dv[j][1]) + (dv[j][2] + dv[j][3]);
            const f32x4 q = dv[j] * xv[j];
            m2 += (q[0] + q[1]) + (q[2] + q[3]);
        }
        m1 = wave_sum(m1) * inv_d; m2 = wave_sum(m2) * inv_d;
#pragma unroll
        for (int j = 0; j < TOK_NJ; ++j) {
            const int c = 4 * lane + 256 * j;
            if (c < dim) *reinterpret_cast<f32x4*>(dx + (int64_t)r * ldx + c) = (dv[j] - m1 - xv[j] * m2) * rstd;
        }
    }
    block_colsum_store(acc, part + (int64_t)blockIdx.x * dim, dim);
}

size_t tok_rows_part_floats(int rows, int dim) { return (size_t)cdiv(rows, TOK_ROW_TILE) * dim; }

int layernorm_rows_bwd(const float* x, int ldx, const float* dy, const float* g, float* dx, float* dg, float* part, int rows, int dim, float eps,
                       hipStream_t s) {
    const int nb = cdiv(rows, TOK_ROW_TILE);
    hipLaunchKernelGGL(layernorm_rows_bwd_kernel, dim3(nb), dim3(256), 0, s, x, ldx, dy, g, dx, part, rows, dim, eps);
    D4_LAUNCH_CHECK();
    return colsum(part, dim, nb, dim, dg, s);
}

// ------------------------------------------------------------------------------------ MAE mask rows
__global__ __launch_bounds__(256) void mask_rows_fwd_kernel(const float* x, const uint8_t* mask, const float* token, float* y, int64_t n4, int dim4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / dim4;
        const int c4 = (int)(i - r * dim4);
        const f32x4 v = mask[r] ? *reinterpret_cast<const f32x4*>(token + 4 * c4) : *reinterpret_cast<const f32x4*>(x + i * 4);
        *reinterpret_cast<f32x4*>(y + i * 4) = v;
    }
}

int mask_rows_fwd(const float* x, const uint8_t* mask, const float* token, float* y, int rows, int dim, hipStream_t s) {
    const int64_t n4 = (int64_t)rows * (dim / 4);
    if (n4 == 0) return 0;
    hipLaunchKernelGGL(mask_rows_fwd_kernel, grid4(n4, 4096), dim3(256), 0, s, x, mask, token, y, n4, dim / 4);
    D4_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void mask_rows_bwd_kernel(const float* dy, const uint8_t* mask, float* dx, float* part, int rows, int dim) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * TOK_ROW_TILE, r1 = min(rows, r0 + TOK_ROW_TILE);
    f32x4 acc[TOK_NJ];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < TOK_NJ; ++j) acc[j] = zero;
    for (int r = r0 + wave; r < r1; r += 4) {
        const bool m = mask[r] != 0;
#pragma unroll
        for (int j = 0; j < TOK_NJ; ++j) {
            const int c = 4 * lane + 256 * j;
            if (c < dim) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(dy + (int64_t)r * dim + c);
                if (m) acc[j] += v;
                *reinterpret_cast<f32x4*>(dx + (int64_t)r * dim + c) = m ? zero : v;
            }
        }
    }
    block_colsum_store(acc, part + (int64_t)blockIdx.x * dim, dim);
}

int mask_rows_bwd(const float* dy, const uint8_t* mask, float* dx, float* dtoken, float* part, int rows, int dim, hipStream_t s) {
    const int nb = cdiv(rows, TOK_ROW_TILE);
    hipLaunchKernelGGL(mask_rows_bwd_kernel, dim3(nb), dim3(256), 0, s, dy, mask, dx, part, rows, dim);
    D4_LAUNCH_CHECK();
    return colsum(part, dim, nb, dim, dtoken, s);
}

// ------------------------------------------------------------------------------------ reconstruction loss, forward + backward
// stage 1: every thread adds its squared errors in index order, the block in a fixed tree -> part[block]; stage 2: one block adds the partials
template <bool VSPACE>
__global__ __launch_bounds__(256) void recon_loss_kernel(const float* recon, const float* video, const float* noise, const float* t, PatchGeom g, int64_t n4,
                                                         float two_over_n, float* d_rows, float* part) {
    __shared__ float sh[256];
    float acc = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 rc = *reinterpret_cast<const f32x4*>(recon + i * 4);
        f32x4 d;
        int64_t vi[4];
        int b;
        g.video_indices((uint32_t)i, vi, b);
        const float tb = VSPACE ? t[b] : 0.f;
        const float inv = 1.f / (1.f - tb);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t v = vi[u];
            const float vid = video[v];
            if (VSPACE) {
                const float nz = noise[v];
                const float diff = (rc[u] - lerp_t(nz, vid, tb)) * inv - (vid - nz);
                acc += diff * diff;
                d[u] = two_over_n * diff * inv;
            } else {
                const float diff = rc[u] - vid;
                acc += diff * diff;
                d[u] = two_over_n * diff;
            }
        }
        *reinterpret_cast<f32x4*>(d_rows + i * 4) = d;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256) void recon_loss_final_kernel(const float* part, int nparts, float inv_n, float* loss) {
    __shared__ float sh[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) acc += part[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = sh[0] * inv_n;
}

int recon_loss_fwd_bwd(const float* recon, const float* video, const float* noise, const float* t, int B, int C, int T, int nh, int nw, int ps, int v_space,
                       float* loss, float* d_rows, float* part, hipStream_t s) {
    const int64_t n = (int64_t)B * C * T * nh * ps * nw * ps;
    const PatchGeom g{C, T, nh, nw, ps, C * ps * ps / 4};
    const dim3 grid = grid4(n / 4, TOK_LOSS_PARTS);
    const float two_over_n = (float)(2.0 / (double)n);
    if (v_space) hipLaunchKernelGGL(recon_loss_kernel<true>, grid, dim3(256), 0, s, recon, video, noise, t, g, n / 4, two_over_n, d_rows, part);
    else hipLaunchKernelGGL(recon_loss_kernel<false>, grid, dim3(256), 0, s, recon, video, noise, t, g, n / 4, two_over_n, d_rows, part);
    D4_LAUNCH_CHECK();
    hipLaunchKernelGGL(recon_loss_final_kernel, dim3(1), dim3(256), 0, s, part, (int)grid.x, (float)(1.0 / (double)n), loss);
    D4_LAUNCH_CHECK();
    return 0;
}

}  // namespace d4

// ------------------------------------------------------------------------------------ C entry points
static bool geom_ok(int B, int C, int T, int nh, int nw, int ps) {
    return B >= 1 && C >= 1 && T >= 1 && nh >= 1 && nw >= 1 && ps >= 1 && (int64_t)B * T * nh * nw * C * ps * ps / 4 <= 0x7fffffff;
}

extern "C" {

int d4_flow_noised_patches(const float* video, const float* noise, const float* t, float* rows, int B, int C, int T, int nh, int nw, int ps, void* stream) {
    D4_REQUIRE(video && rows && (!noise == !t), "d4_flow_noised_patches: null argument (noise and t are given together, or both null)");
    D4_REQUIRE(geom_ok(B, C, T, nh, nw, ps), "d4_flow_noised_patches: bad sizes");
    D4_REQUIRE((C * ps * ps) % 4 == 0 && ((uintptr_t)rows % 16) == 0, "d4_flow_noised_patches: the patch row (%d floats) must be a multiple of 4 and the rows 16-byte aligned",
               C * ps * ps);
    return d4::flow_noised_patches(video, noise, t, rows, B, C, T, nh, nw, ps, static_cast<hipStream_t>(stream));
}

size_t d4_tok_rows_part_floats(int rows, int dim) { return rows >= 1 && dim >= 1 ? d4::tok_rows_part_floats(rows, dim) : 0; }

static int rows_ok(const char* who, int rows, int dim, size_t part_floats) {
    D4_REQUIRE(rows >= 1 && dim >= 4 && dim % 4 == 0 && dim <= 256 * d4::TOK_NJ, "%s: %d rows of %d floats (at least one row; dim a multiple of 4, at most %d)", who, rows, dim,
               256 * d4::TOK_NJ);
    D4_REQUIRE(part_floats >= d4::tok_rows_part_floats(rows, dim), "%s: scratch too small (d4_tok_rows_part_floats)", who);
    return 0;
}

int d4_layernorm_rows_bwd(const float* x, int ldx, const float* dy, const float* g, float* dx, float* dg, float* part, size_t part_floats, int rows, int dim,
                          float eps, void* stream) {
    D4_REQUIRE(x && dy && g && dx && dg && part, "d4_layernorm_rows_bwd: null argument");
    if (int rc = rows_ok("d4_layernorm_rows_bwd", rows, dim, part_floats)) return rc;
    D4_REQUIRE(ldx >= dim && ldx % 4 == 0 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)g | (uintptr_t)dx | (uintptr_t)part) % 16) == 0,
               "d4_layernorm_rows_bwd: ldx must be a multiple of 4 (at least dim) and every pointer 16-byte aligned");
    return d4::layernorm_rows_bwd(x, ldx, dy, g, dx, dg, part, rows, dim, eps, static_cast<hipStream_t>(stream));
}

int d4_mask_rows_fwd(const float* x, const uint8_t* mask, const float* token, float* y, int rows, int dim, void* stream) {
    D4_REQUIRE(x && mask && token && y, "d4_mask_rows_fwd: null argument");
    D4_REQUIRE(rows >= 1 && dim >= 4 && dim % 4 == 0, "d4_mask_rows_fwd: %d rows of %d floats (at least one row; dim a multiple of 4)", rows, dim);
    D4_REQUIRE((((uintptr_t)x | (uintptr_t)token | (uintptr_t)y) % 16) == 0, "d4_mask_rows_fwd: every float pointer 16-byte aligned");
    return d4::mask_rows_fwd(x, mask, token, y, rows, dim, static_cast<hipStream_t>(stream));
}

int d4_mask_rows_bwd(const float* dy, const uint8_t* mask, float* dx, float* dtoken, float* part, size_t part_floats, int rows, int dim, void* stream) {
    D4_REQUIRE(dy && mask && dx && dtoken && part, "d4_mask_rows_bwd: null argument");
    if (int rc = rows_ok("d4_mask_rows_bwd", rows, dim, part_floats)) return rc;
    D4_REQUIRE((((uintptr_t)dy | (uintptr_t)dx | (uintptr_t)part) % 16) == 0, "d4_mask_rows_bwd: every float pointer 16-byte aligned");
    return d4::mask_rows_bwd(dy, mask, dx, dtoken, part, rows, dim, static_cast<hipStream_t>(stream));
}

int d4_recon_loss_fwd_bwd(const float* recon_rows, const float* video, const float* noise, const float* t, int B, int C, int T, int nh, int nw, int ps, int v_space,
                          float* loss, float* d_rows, float* part, size_t part_floats, void* stream) {
    D4_REQUIRE(recon_rows && video && loss && d_rows && part && (!v_space || (noise && t)), "d4_recon_loss_fwd_bwd: null argument");
    D4_REQUIRE(geom_ok(B, C, T, nh, nw, ps), "d4_recon_loss_fwd_bwd: bad sizes");
    D4_REQUIRE((C * ps * ps) % 4 == 0 && (((uintptr_t)recon_rows | (uintptr_t)d_rows) % 16) == 0,
               "d4_recon_loss_fwd_bwd: the patch row (%d floats) must be a multiple of 4 and the rows 16-byte aligned", C * ps * ps);
    D4_REQUIRE(part_floats >= (size_t)d4::TOK_LOSS_PARTS, "d4_recon_loss_fwd_bwd: scratch of at least %d floats", d4::TOK_LOSS_PARTS);
    return d4::recon_loss_fwd_bwd(recon_rows, video, noise, t, B, C, T, nh, nw, ps, v_space, loss, d_rows, part, static_cast<hipStream_t>(stream));
}

}  // extern "C"
