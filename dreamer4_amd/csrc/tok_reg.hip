// Latent regularisers of the VideoTokenizer training forward: each operator returns its loss and d loss / d x for a unit upstream
// gradient in one call, the shape of recon_loss_fwd_bwd.
//
//   sigreg_fwd_bwd        sigreg(x) without a mask (dreamer4.py:728-767) on x [K][N][d]: M unit slices, the empirical characteristic function of the
//                         projections at `knots` points of linspace(lo, hi), its weighted squared distance to exp(-t^2 / 2), trapezoid over the knots,
//                         mean over (K, M).  The reference materialises exp(i x_t) as K x N x M x knots complex numbers; here a projection lives in LDS
//                         for the time a block of 64 rows x 64 slices needs it and a sine / cosine in a register.
//   latent_ortho_fwd_bwd  orthogonal_loss(x) (dreamer4.py:389-402) on x [F][n][d]: per frame centre over n, normalise the rows, sum of the squared
//                         off-diagonal entries of the n x n Gram; mean over frames.  The Gram is formed entry by entry (never through the d x d
//                         identity, which cancels when the rows are nearly orthogonal).
//
// No float atomics: sums that cross a workgroup are per-block partials in the caller's `part`, reduced by a second launch in a fixed order; inside a
// block every sum has a fixed order too.  Equal inputs give equal bits.  Plain HIP C++; sines and cosines are one sincosf per (row, slice, knot): the
// angles reach hundreds of radians and the result is used in a difference of nearly equal numbers, so no recurrence and no fast intrinsic.
#include "common.h"
#include "kernels.h"

namespace d4 {

// torch.linspace in float32 (ATen RangeFactories): the first half from the start, the second from the end
struct Knots {
    float lo, hi, step;
    int T;
    __device__ __forceinline__ float at(int j) const { return j < T / 2 ? lo + step * (float)j : hi - step * (float)(T - 1 - j); }
    // trapezoid weight of knot j: half the distance between its neighbours (one-sided at the ends)
    __device__ __forceinline__ float trapezoid(int j) const { return 0.5f * (at(j < T - 1 ? j + 1 : j) - at(j > 0 ? j - 1 : j)); }
};

// us[SIGREG_SLICES][d + 1] = F.normalize(projs[m0 .. m0 + 63]) (eps 1e-12); slices past M are zero.  Ends with a barrier.
__device__ __forceinline__ void load_unit_slices(const float* projs, int M, int d, int m0, float* us) {
    const int ld = d + 1;
    for (int i = threadIdx.x; i < SIGREG_SLICES * d; i += blockDim.x) {
        const int m = i / d, c = i - m * d;
        us[m * ld + c] = m0 + m < M ? projs[(int64_t)(m0 + m) * d + c] : 0.f;
    }
    __syncthreads();
    if (threadIdx.x < SIGREG_SLICES) {
        float* u = us + threadIdx.x * ld;
        float ss = 0.f;
        for (int c = 0; c < d; ++c) ss += u[c] * u[c];
        const float den = fmaxf(sqrtf(ss), 1e-12f);
        for (int c = 0; c < d; ++c) u[c] /= den;
    }
    __syncthreads();
}

// wave-uniform row, one slice per lane: x_row . u_lane (the row is read at one address by the whole wave, the slice from LDS at stride d + 1)
__device__ __forceinline__ float project(const float* xr, const float* u, int d) {
    float p = 0.f;
    for (int c = 0; c < d; ++c) p = fmaf(xr[c], u[c], p);
    return p;
}

// ------------------------------------------------------------------------------------ SIGReg, pass 1: partial sums of the characteristic function
// grid (blocks of rows, tiles of slices, K).  The block projects its 64 rows on its 64 slices into LDS, then thread i owns pair (slice, knot) =
// (i / T, i % T) and adds cos and sin of t * projection over the block's rows in row order -> part[k][row block][m][j][2].
__global__ __launch_bounds__(256) void sigreg_ecf_kernel(const float* x, const float* projs, Knots kn, int N, int d, int M, int nrb, float* part) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* us = smem;                                      // [64][d + 1]
    float* ps = smem + SIGREG_SLICES * (d + 1);            // [64 rows][64 slices]
    const int rb = blockIdx.x, m0 = blockIdx.y * SIGREG_SLICES, k = blockIdx.z;
    const int r0 = rb * SIGREG_ROWS, nr = min(SIGREG_ROWS, N - r0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    load_unit_slices(projs, M, d, m0, us);
    const float* xk = x + ((int64_t)k * N + r0) * d;
    for (int r = wave; r < nr; r += 4) ps[r * SIGREG_SLICES + lane] = project(xk + (int64_t)r * d, us + lane * (d + 1), d);
    __syncthreads();
    const int T = kn.T, pairs = min(SIGREG_SLICES, M - m0) * T;
    float* out = part + ((((int64_t)k * nrb + rb) * M + m0) * T) * 2;
    for (int i = threadIdx.x; i < pairs; i += 256) {
        const int m = i / T;
        const float t = kn.at(i - m * T);
        float cs = 0.f, sn = 0.f;
        for (int r = 0; r < nr; ++r) {
            float s, c;
            sincosf(t * ps[r * SIGREG_SLICES + m], &s, &c);
            cs += c; sn += s;
        }
        out[2 * i] = cs; out[2 * i + 1] = sn;
    }
}

// fixed tree over the 256 values of a block
__device__ __forceinline__ float block_sum256(float v, float* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}

// ------------------------------------------------------------------------------------ SIGReg, pass 2: the characteristic function, the loss terms
// One thread per (k, m, j): adds the partials over the blocks of rows in order, C + iS = the mean of exp(i t p); its loss term w phi ((C - phi)^2 + S^2)
// (w the trapezoid weight) goes into a per-block sum; the two factors the backward needs, g (C - phi) and g S with g = 2 w phi t / (N K M), replace the
// partials of row block 0 (the thread that read them writes them).
__global__ __launch_bounds__(256) void sigreg_reduce_kernel(float* part, Knots kn, int64_t kmt, int mt, int nrb, float inv_n, float grad_scale, float* loss_part) {
    __shared__ float sh[256];
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float term = 0.f;
    if (q < kmt) {
        const int64_t k = q / mt, rem = q - k * mt;
        const int j = (int)(rem % kn.T);
        float* p = part + (k * nrb * mt + rem) * 2;
        float cs = 0.f, sn = 0.f;
        for (int rb = 0; rb < nrb; ++rb) {
            cs += p[(int64_t)rb * mt * 2];
            sn += p[(int64_t)rb * mt * 2 + 1];
        }
        const float t = kn.at(j), phi = expf(-0.5f * t * t), w = kn.trapezoid(j) * phi;
        const float e = cs * inv_n - phi, S = sn * inv_n;
        term = w * (e * e + S * S);
        const float g = grad_scale * w * t;
        p[0] = g * e; p[1] = g * S;
    }
    const float total = block_sum256(term, sh);
    if (threadIdx.x == 0) loss_part[blockIdx.x] = total;
}

// out[0] = scale * sum of part[0 .. n) in a fixed order (one block).  n is ceil(K M knots / 256) for SIGReg, the frames for the orthogonality loss: a
// few thousand at tokenizer sizes.  At the entry points' limits it reaches 6.7e7 values walked by this one block (correct, but slow): a caller of that size
// wants a second level here.
__global__ __launch_bounds__(256) void sum_parts_kernel(const float* part, int n, float scale, float* out) {
    __shared__ float sh[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
    const float total = block_sum256(acc, sh);
    if (threadIdx.x == 0) *out = total * scale;
}

// ------------------------------------------------------------------------------------ SIGReg, pass 3: d loss / d x
// grid (blocks of rows, K).  d loss / d projection(row, m) = sum_j cos(t_j p) gS_j - sin(t_j p) ge_j (pass 2's factors of (k, m)); the block walks the
// tiles of 64 slices: projections and that sum per (row, lane = slice), then dx[row][c] += sum_m dp[row][m] u_m[c] in slice order, each (row, c) by the
// same thread in every tile.
__global__ __launch_bounds__(256) void sigreg_grad_kernel(const float* x, const float* projs, const float* part, Knots kn, int N, int d, int M, int nrb, float* dx) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LG = SIGREG_SLICES + 1;
    float* us = smem;                                      // [64][d + 1]
    float* gs = smem + SIGREG_SLICES * (d + 1);            // [64 rows][64 slices + 1]
    const int rb = blockIdx.x, k = blockIdx.y;
    const int r0 = rb * SIGREG_ROWS, nr = min(SIGREG_ROWS, N - r0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = kn.T;
    const float* xk = x + ((int64_t)k * N + r0) * d;
    float* dxk = dx + ((int64_t)k * N + r0) * d;
    for (int m0 = 0; m0 < M; m0 += SIGREG_SLICES) {
        load_unit_slices(projs, M, d, m0, us);
        const bool live = m0 + lane < M;
        const float* f = part + (((int64_t)k * nrb * M) + (live ? m0 + lane : 0)) * T * 2;
        for (int r = wave; r < nr; r += 4) {
            float g = 0.f;
            if (live) {
                const float p = project(xk + (int64_t)r * d, us + lane * (d + 1), d);
                for (int j = 0; j < T; ++j) {
                    float s, c;
                    sincosf(kn.at(j) * p, &s, &c);
                    g += c * f[2 * j + 1] - s * f[2 * j];
                }
            }
            gs[r * LG + lane] = g;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < nr * d; i += 256) {
            const int r = i / d, c = i - r * d;
            float acc = 0.f;
            for (int m = 0; m < SIGREG_SLICES; ++m) acc = fmaf(gs[r * LG + m], us[m * (d + 1) + c], acc);
            dxk[i] = m0 == 0 ? acc : dxk[i] + acc;
        }
        __syncthreads();
    }
}

static size_t sigreg_loss_parts(int K, int M, int knots) { return (size_t)(((int64_t)K * M * knots + 255) / 256); }

size_t sigreg_part_floats(int K, int N, int M, int knots) {
    return (size_t)K * (size_t)cdiv(N, SIGREG_ROWS) * (size_t)M * knots * 2 + sigreg_loss_parts(K, M, knots);
}

int sigreg_fwd_bwd(const float* x, const float* projs, int K, int N, int d, int M, float lo, float hi, int knots, float* loss, float* dx, float* part,
                   hipStream_t s) {
    const int nrb = cdiv(N, SIGREG_ROWS), mtiles = cdiv(M, SIGREG_SLICES);
    const Knots kn{lo, hi, (hi - lo) / (float)(knots - 1), knots};
    const int64_t kmt = (int64_t)K * M * knots;
    const int nlp = (int)sigreg_loss_parts(K, M, knots);
    float* loss_part = part + (size_t)K * nrb * M * knots * 2;
    const size_t lds_ecf = sizeof(float) * (SIGREG_SLICES * (d + 1) + SIGREG_ROWS * SIGREG_SLICES);
    const size_t lds_grad = sizeof(float) * (SIGREG_SLICES * (d + 1) + SIGREG_ROWS * (SIGREG_SLICES + 1));
    hipLaunchKernelGGL(sigreg_ecf_kernel, dim3(nrb, mtiles, K), dim3(256), lds_ecf, s, x, projs, kn, N, d, M, nrb, part);
    D4_LAUNCH_CHECK();
    hipLaunchKernelGGL(sigreg_reduce_kernel, dim3(nlp), dim3(256), 0, s, part, kn, kmt, M * knots, nrb, (float)(1.0 / (double)N),
                       (float)(2.0 / ((double)N * K * M)), loss_part);
    D4_LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(256), 0, s, loss_part, nlp, (float)(1.0 / ((double)K * M)), loss);
    D4_LAUNCH_CHECK();
    hipLaunchKernelGGL(sigreg_grad_kernel, dim3(nrb, K), dim3(256), lds_grad, s, x, projs, part, kn, N, d, M, nrb, dx);
    D4_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------ latent orthogonality
// One block per frame, one wave per row i (every fourth), lane l holds columns l and l + 64.  y = the centred, normalised rows, recomputed from x, the
// column means and the rows' 1 / max(norm, 1e-12) (LDS) wherever they are read.  Row i: for j != i in order, G_ij = y_i . y_j (a wave sum),
// loss += G_ij^2, dy_i += G_ij y_j; then dy_i *= 4 / F, back through the normalisation (d xc_i = (dy_i - y_i (y_i . dy_i)) / norm_i; dy_i / 1e-12 where the
// norm was clamped) and, after the block's column sums of d xc met in LDS in wave order, through the centring (dx_i = d xc_i - mean_i d xc).
__global__ __launch_bounds__(256) void latent_ortho_kernel(const float* x, int n, int d, float scale, float* dx, float* frame_loss) {
    __shared__ float mean[ORTHO_MAX_DIM], rinv[ORTHO_MAX_ROWS], colw[4][ORTHO_MAX_DIM], lossw[4];
    __shared__ uint8_t clamped[ORTHO_MAX_ROWS];            // the row's norm is at or below F.normalize's eps: no gradient through the norm
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* xf = x + (int64_t)blockIdx.x * n * d;
    float* dxf = dx + (int64_t)blockIdx.x * n * d;
    const int c0 = lane, c1 = lane + 64;
    const bool h0 = c0 < d, h1 = c1 < d;
    const float inv_n = 1.f / (float)n;

    float s0 = 0.f, s1 = 0.f;
    for (int i = wave; i < n; i += 4) {
        s0 += h0 ? xf[i * d + c0] : 0.f;
        s1 += h1 ? xf[i * d + c1] : 0.f;
    }
    colw[wave][c0] = s0; colw[wave][c1] = s1;
    __syncthreads();
    if (threadIdx.x < ORTHO_MAX_DIM) mean[threadIdx.x] = (((colw[0][threadIdx.x] + colw[1][threadIdx.x]) + colw[2][threadIdx.x]) + colw[3][threadIdx.x]) * inv_n;
    __syncthreads();
    const float mu0 = mean[c0], mu1 = mean[c1];
    for (int i = wave; i < n; i += 4) {
        const float a0 = h0 ? xf[i * d + c0] - mu0 : 0.f, a1 = h1 ? xf[i * d + c1] - mu1 : 0.f;
        const float ss = wave_sum(a0 * a0 + a1 * a1);
        const float nrm = sqrtf(ss);
        if (lane == 0) { rinv[i] = 1.f / fmaxf(nrm, 1e-12f); clamped[i] = nrm <= 1e-12f; }
    }
    __syncthreads();

    float ca0 = 0.f, ca1 = 0.f, lsum = 0.f;
    for (int i = wave; i < n; i += 4) {
        const float ri = rinv[i];
        const float yi0 = h0 ? (xf[i * d + c0] - mu0) * ri : 0.f, yi1 = h1 ? (xf[i * d + c1] - mu1) * ri : 0.f;
        float g0 = 0.f, g1 = 0.f, li = 0.f;
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            const float rj = rinv[j];
            const float yj0 = h0 ? (xf[j * d + c0] - mu0) * rj : 0.f, yj1 = h1 ? (xf[j * d + c1] - mu1) * rj : 0.f;
            const float dot = wave_sum(yi0 * yj0 + yi1 * yj1);
            li += dot * dot;
            g0 = fmaf(dot, yj0, g0); g1 = fmaf(dot, yj1, g1);
        }
        lsum += li;
        g0 *= scale; g1 *= scale;
        const float proj = clamped[i] ? 0.f : wave_sum(yi0 * g0 + yi1 * g1);
        const float d0 = (g0 - yi0 * proj) * ri, d1 = (g1 - yi1 * proj) * ri;
        if (h0) dxf[i * d + c0] = d0;
        if (h1) dxf[i * d + c1] = d1;
        ca0 += d0; ca1 += d1;
    }
    __syncthreads();                                       // everyone is done with `mean` as the column means of x
    colw[wave][c0] = ca0; colw[wave][c1] = ca1;
    if (lane == 0) lossw[wave] = lsum;
    __syncthreads();
    if (threadIdx.x < ORTHO_MAX_DIM) mean[threadIdx.x] = (((colw[0][threadIdx.x] + colw[1][threadIdx.x]) + colw[2][threadIdx.x]) + colw[3][threadIdx.x]) * inv_n;
    if (threadIdx.x == 0) frame_loss[blockIdx.x] = ((lossw[0] + lossw[1]) + lossw[2]) + lossw[3];
    __syncthreads();
    const float m0 = mean[c0], m1 = mean[c1];
    for (int i = wave; i < n; i += 4) {                    // each lane takes back what it wrote itself
        if (h0) dxf[i * d + c0] -= m0;
        if (h1) dxf[i * d + c1] -= m1;
    }
}

int latent_ortho_fwd_bwd(const float* x, int F, int n, int d, float* loss, float* dx, float* part, hipStream_t s) {
    hipLaunchKernelGGL(latent_ortho_kernel, dim3(F), dim3(256), 0, s, x, n, d, (float)(4.0 / (double)F), dx, part);
    D4_LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(256), 0, s, part, F, (float)(1.0 / (double)F), loss);
    D4_LAUNCH_CHECK();
    return 0;
}

}  // namespace d4

// ------------------------------------------------------------------------------------ C entry points
extern "C" {

static int sigreg_sizes_ok(const char* who, int K, int N, int d, int M, int knots) {
    D4_REQUIRE(K >= 1 && K <= 65535 && N >= 1 && d >= 1 && M >= 1 && (int64_t)K * N * d <= ((int64_t)1 << 40), "%s: x is %d x %d x %d (K at most 65535)", who, K, N, d);
    D4_REQUIRE(d <= d4::SIGREG_MAX_DIM, "%s: dim %d is above the limit of %d", who, d, d4::SIGREG_MAX_DIM);
    D4_REQUIRE(knots >= 2 && knots <= d4::SIGREG_MAX_KNOTS, "%s: %d knots (2 to %d)", who, knots, d4::SIGREG_MAX_KNOTS);
    D4_REQUIRE(M <= d4::SIGREG_MAX_SLICES, "%s: %d slices (at most %d)", who, M, d4::SIGREG_MAX_SLICES);
    return 0;
}

size_t d4_sigreg_part_floats(int K, int N, int M, int num_knots) {
    return K >= 1 && N >= 1 && M >= 1 && num_knots >= 1 ? d4::sigreg_part_floats(K, N, M, num_knots) : 0;
}

int d4_sigreg_fwd_bwd(const float* x, const float* projs, int K, int N, int d, int M, float lo, float hi, int num_knots, float* loss, float* dx, float* part,
                      size_t part_floats, void* stream) {
    D4_REQUIRE(x && projs && loss && dx && part, "d4_sigreg_fwd_bwd: null argument");
    if (int rc = sigreg_sizes_ok("d4_sigreg_fwd_bwd", K, N, d, M, num_knots)) return rc;
    D4_REQUIRE(lo == lo && hi == hi && lo - lo == 0.f && hi - hi == 0.f, "d4_sigreg_fwd_bwd: the domain must be finite");
    D4_REQUIRE(part_floats >= d4::sigreg_part_floats(K, N, M, num_knots), "d4_sigreg_fwd_bwd: scratch too small (d4_sigreg_part_floats)");
    return d4::sigreg_fwd_bwd(x, projs, K, N, d, M, lo, hi, num_knots, loss, dx, part, static_cast<hipStream_t>(stream));
}

size_t d4_latent_ortho_part_floats(int F) { return F >= 1 ? (size_t)F : 0; }

int d4_latent_ortho_fwd_bwd(const float* x, int F, int n, int d, float* loss, float* dx, float* part, size_t part_floats, void* stream) {
    D4_REQUIRE(x && loss && dx && part, "d4_latent_ortho_fwd_bwd: null argument");
    D4_REQUIRE(F >= 1 && n >= 1 && d >= 1 && (int64_t)F * n * d <= ((int64_t)1 << 40), "d4_latent_ortho_fwd_bwd: x is %d x %d x %d", F, n, d);
    D4_REQUIRE(n <= d4::ORTHO_MAX_ROWS, "d4_latent_ortho_fwd_bwd: %d rows per frame (at most %d)", n, d4::ORTHO_MAX_ROWS);
    D4_REQUIRE(d <= d4::ORTHO_MAX_DIM, "d4_latent_ortho_fwd_bwd: dim %d is above the limit of %d", d, d4::ORTHO_MAX_DIM);
    D4_REQUIRE(part_floats >= (size_t)F, "d4_latent_ortho_fwd_bwd: scratch too small (d4_latent_ortho_part_floats)");
    return d4::latent_ortho_fwd_bwd(x, F, n, d, loss, dx, part, static_cast<hipStream_t>(stream));
}

}  // extern "C"
