// Trunk backward: the blocks of the AxialSpaceTimeTransformer as forward + backward operators on the REFERENCE parameter
// layout — FeedForward (D4:2079-2116) and Attention.forward (D4:1968-2075) in its three uses: within-frame self attention (RMSNorm, q/k/v,
// learned value-residual mix, K-head-RMSNorm, soft clamp, special-token mask, belief projection, head gates, to_out), time attention (the
// same with rotary positions and a causal mask, one problem per token column), and attention over a context (attention pools over the
// stack of layer hiddens, the special tokens' cross attention, learned-query pools) — so that each can be checked directly against
// autograd of the oracle's restatement (tests/test_gpu_backward.py) and composed into the dynamics training forward
// (dreamer4_amd/trunk_ops.py: D4:6956-7743).
//
// The matrix work is the engine's fp32 MFMA GEMM (transposed-operand forms for dX, split-K for dW); what is new here are the two
// attention-core backward kernels (one block per (group, head), everything for <= 32 / 64 items in LDS) and the SiLU-GLU / RMSNorm
// backward glue.  Every backward recomputes its forward: only the block inputs are kept between the two passes.  Nothing here is called
// by the imagination path.
#include "common.h"
#include "kernels.h"
#include "attn_tiled.h"
#include "../../include/d4hip.h"
#include <atomic>
#include <float.h>

namespace d4 {

static constexpr float RMS_EPS = 1.1920928955078125e-07f;   // torch.finfo(float32).eps (nn.RMSNorm eps=None)

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// ------------------------------------------------------------------------------------------------ SiLU-GLU glue
// hidden layout [rows][2 * Ip]: value half at column 0, gate half at column Ip (Ip = inner rounded up to 16, so that 2 Ip — the contraction
// length of the input-gradient GEMM — is a multiple of 32; pad columns are zero)
static inline int ff_ip(int inner) { return (inner + 15) / 16 * 16; }
__global__ void swiglu_fwd_kernel(const float* h, float* u, int rows, int I, int Ip) {
    const int64_t tot = (int64_t)rows * Ip;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Ip);
        const int64_t r = i / Ip;
        const float a = h[r * 2 * Ip + c], g = h[r * 2 * Ip + Ip + c];
        u[i] = c < I ? a * g * sigm(g) : 0.f;
    }
}
// dh = [du * silu(g) | du * a * silu'(g)]
__global__ void swiglu_bwd_kernel(const float* h, const float* du, float* dh, int rows, int I, int Ip) {
    const int64_t tot = (int64_t)rows * Ip;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < tot; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Ip);
        const int64_t r = i / Ip;
        const float a = h[r * 2 * Ip + c], g = h[r * 2 * Ip + Ip + c], d = du[i];
        const float s = sigm(g);
        dh[r * 2 * Ip + c] = c < I ? d * g * s : 0.f;
        dh[r * 2 * Ip + Ip + c] = c < I ? d * a * s * (1.f + g * (1.f - s)) : 0.f;
    }
}
static dim3 grid_for(int64_t n) { return dim3((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)); }
static int swiglu_fwd(const float* h, float* u, int rows, int I, int Ip, hipStream_t s) {
    hipLaunchKernelGGL(swiglu_fwd_kernel, grid_for((int64_t)rows * Ip), dim3(256), 0, s, h, u, rows, I, Ip);
    D4_LAUNCH_CHECK();
    return 0;
}
static int swiglu_bwd(const float* h, const float* du, float* dh, int rows, int I, int Ip, hipStream_t s) {
    hipLaunchKernelGGL(swiglu_bwd_kernel, grid_for((int64_t)rows * Ip), dim3(256), 0, s, h, du, dh, rows, I, Ip);
    D4_LAUNCH_CHECK();
    return 0;
}

static int gemm_f32(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias, int M, int N, int K, int flags, hipStream_t s) {
    GemmArgs g{A, lda, W, ldw, C, ldc, bias, nullptr, 0, M, N, K, flags, 0.f};
    return gemm(g, s);
}

// ------------------------------------------------------------------------------------------------ bf16 training arithmetic
// d4_train_arith_set(1): the three products of every Linear of the blocks (forward, input gradient, weight gradient) take bf16 images of their
// operands (round to nearest even, built into a scratch the caller binds for the call: d4_train_scratch_bind) on the bf16 matrix pipe, fp32 accumulate and
// fp32 results; everything else of a block is the fp32 path unchanged.  Which products: a rule on the Linear's shape only —
// out features >= 16 and in features >= 16 (so the forward / input-gradient product has N >= 16, K >= 16 and the weight-gradient product M >= 16,
// N >= 16), any number of rows; the heads-wide gate and mix projections are separate fp32 products by construction.
static std::atomic<int> g_train_arith{0};
// d4_train_wide_set(1): the within-frame and cross attentions accept up to ATT_MAX_FRAMES items per side, and take the tiled core
// (attn_tiled.hip) where a side has more than 64; at <= 64 items, and with the switch off, nothing changes (kernels, workspace sizes, refusals)
static std::atomic<int> g_train_wide{0};
static bool space_tiled(int tokens) { return g_space_attn_tiled != 0 || (g_train_wide.load() && tokens > 64); }
// d4_train_attn_products_set(1): wherever a launch takes the tiled core it takes the core's bf16-product form (attn_tiled_bf16.hip),
// whose bf16 images follow the planes in the workspace; the whole-problem-in-LDS kernels, and everything with the switch off, are unchanged
static std::atomic<int> g_train_attn_products{0};
static bool attn_bf16() { return g_train_attn_products.load() != 0; }
static bool cross_tiled(int nq, int nk) { return g_cross_attn_tiled != 0 || (g_train_wide.load() && (nq > 64 || nk > 64)); }
struct Bf16Ctx {
    uint16_t *a = nullptr, *b = nullptr, *w = nullptr; size_t act = 0, wgt = 0;      // images: two activation-sized, one weight-sized (elements)
    const float* a_src = nullptr; int a_ld = 0, a_rows = 0, a_cols = 0;               // what image `a` holds: a dY feeds two products of one call
};
static thread_local Bf16Ctx t_bf;
struct Bf16Scratch { void* p = nullptr; size_t bytes = 0; };
static thread_local Bf16Scratch t_scratch;       // d4_train_scratch_bind: this thread's scratch for the bf16 images of its next block calls
// image `a` = bf16 of rows x cols of src at row stride r64(cols), pad columns zero; converted once per call and source (no buffer of a block
// is rewritten between the two products that read it; the kernels that WRITE such a buffer call image_a_written on it all the same, so
// that a reordered backward cannot meet a stale image)
static inline void image_a_written(const float* buf) { if (t_bf.a_src == buf) t_bf.a_src = nullptr; }
static int image_a(const float* src, int ld, int rows, int cols, hipStream_t s) {
    Bf16Ctx& c = t_bf;
    if (c.a_src == src && c.a_ld == ld && c.a_rows == rows && c.a_cols == cols) return 0;
    const int cp = (cols + 63) / 64 * 64;
    if (int rc = cvt_pad_bf16(src, ld, c.a, cp, rows, cols, cp, s)) return rc;
    c.a_src = src; c.a_ld = ld; c.a_rows = rows; c.a_cols = cols;
    return 0;
}
static inline size_t r64(size_t n) { return (n + 63) / 64 * 64; }
static inline bool bf16_rule(int out_features, int in_features) { return out_features >= 16 && in_features >= 16; }
// scratch (bytes) of a block with `rows` token rows, activations up to `width` columns, weights up to wn x wk
static size_t bf16_extra_bytes(size_t rows, size_t width, size_t wn, size_t wk) {
    return 2 * (2 * r64(rows * r64(width)) + r64(r64(wn) * r64(wk)));
}
struct Bf16Scope {           // carves this thread's bound scratch for the helpers of one entry-point call
    Bf16Scope() {}
    ~Bf16Scope() { t_bf = Bf16Ctx{}; }
    int enter(const char* who, size_t rows, size_t width, size_t wn, size_t wk) {
        if (!g_train_arith.load(std::memory_order_relaxed)) {
            D4_REQUIRE(!t_scratch.p, "%s: a bf16 scratch is bound on this thread but the training arithmetic is fp32 (another thread changed d4_train_arith_set?)", who);
            return 0;
        }
        D4_REQUIRE(t_scratch.p && ((uintptr_t)t_scratch.p % 256) == 0 && t_scratch.bytes >= bf16_extra_bytes(rows, width, wn, wk),
                   "%s: the bf16 training arithmetic needs a 256-byte aligned scratch of the block's *_bf16_scratch_bytes bound on this thread (d4_train_scratch_bind)", who);
        Bf16Ctx c;
        c.act = r64(rows * r64(width)); c.wgt = r64(r64(wn) * r64(wk));
        c.a = reinterpret_cast<uint16_t*>(t_scratch.p); c.b = c.a + c.act; c.w = c.b + c.act;
        t_bf = c;
        return 0;
    }
};

// Y = A W^T (+ bias): the forward product of a Linear
static int gemm_b(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias, int M, int N, int K, int flags, hipStream_t s) {
    if (!t_bf.a || (flags & (GEMM_TRANS_A | GEMM_TRANS_B)) || !bf16_rule(N, K)) return gemm_f32(A, lda, W, ldw, C, ldc, bias, M, N, K, flags, s);
    const int Kp = (int)r64(K);
    D4_REQUIRE((size_t)M * Kp <= t_bf.act && (size_t)N * Kp <= t_bf.wgt, "bf16 training arithmetic: operand image larger than the scratch (%d x %d x %d)", M, N, K);
    int rc;
    if ((rc = image_a(A, lda, M, K, s))) return rc;
    if ((rc = cvt_pad_bf16(W, ldw, t_bf.w, Kp, N, K, Kp, s))) return rc;
    GemmArgs g{nullptr, Kp, nullptr, Kp, C, ldc, bias, nullptr, 0, M, N, Kp, flags, 0.f};
    g.Ab = t_bf.a; g.Wb = t_bf.w;
    return gemm_bf16a(g, s);
}

// dX[M][N] (+)= dY[M][K] W[K][N]: the input gradient of a Linear (W [out = K][in = N])
static int lin_dx(const float* dY, int ldy, const float* W, int ldw, float* dX, int ldx, int M, int N, int K, float* wt, hipStream_t s, bool accumulate = false) {
    if (!t_bf.a || !bf16_rule(K, N)) {
        if (!accumulate) return gemm_dx(dY, ldy, W, ldw, dX, ldx, M, N, K, wt, s);
        return gemm_f32(dY, ldy, W, ldw, dX, ldx, nullptr, M, N, K, GEMM_TRANS_B | GEMM_ACCUMULATE, s);
    }
    const int Kp = (int)r64(K);
    D4_REQUIRE((size_t)M * Kp <= t_bf.act && (size_t)N * Kp <= t_bf.wgt, "bf16 training arithmetic: operand image larger than the scratch (%d x %d x %d)", M, N, K);
    int rc;
    if ((rc = image_a(dY, ldy, M, K, s))) return rc;
    if ((rc = cvt_transpose_bf16(W, ldw, t_bf.w, Kp, K, N, Kp, s))) return rc;
    GemmArgs g{nullptr, Kp, nullptr, Kp, dX, ldx, nullptr, nullptr, 0, M, N, Kp, accumulate ? GEMM_ACCUMULATE : 0, 0.f};
    g.Ab = t_bf.a; g.Wb = t_bf.w;
    return gemm_bf16a(g, s);
}

// Weight gradient dW[M][N] = A^T B with A [K][M], B [K][N] row-major and K = token rows (thousands to tens of thousands) while M x N is one
// weight matrix (often only 64 tiles): split K over the grid's batch dimension into partial products, then one fixed-order reduce —
// without it these GEMMs run on a quarter of the CUs and were half of a training step (tools/train_step_time.py).
constexpr size_t DW_PART_FLOATS = (size_t)8 << 20;          // partial-product scratch per workspace (32 MB)
static int gemm_dw_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, float* part, hipStream_t s);
static int gemm_dw(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, float* part, hipStream_t s) {
    if (t_bf.a && bf16_rule(M, N)) {
        // bf16 training arithmetic: images of dY and X as they lie (rows = the contraction), transposed by the LDS read (gemm_tn_bf16.hip)
        const int Mp = (int)r64(M), Np = (N + 7) & ~7;          // (dY's image at the stride the input-gradient product reads it with)
        D4_REQUIRE((size_t)K * Mp <= t_bf.act && (size_t)K * Np <= t_bf.act, "bf16 training arithmetic: operand image larger than the scratch (%d x %d x %d)", M, N, K);
        int rc;
        if ((rc = image_a(A, lda, K, M, s))) return rc;
        if ((rc = cvt_pad_bf16(B, ldb, t_bf.b, Np, K, N, Np, s))) return rc;
        return gemm_tn_bf16(t_bf.a, Mp, t_bf.b, Np, C, ldc, M, N, K, part, part ? DW_PART_FLOATS : 0, s);
    }
    return gemm_dw_f32(A, lda, B, ldb, C, ldc, M, N, K, part, s);
}
static int gemm_dw_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, float* part, hipStream_t s) {
    // operands read straight into the MFMA layout, k split inside the workgroup and over slices (gemm_tn.hip); the transposed-operand form of
    // the general GEMM below remains for leading dimensions that are not multiples of 4
    if (gemm_tn_applicable(A, lda, B, ldb, C, ldc, M, N, K)) return gemm_tn(A, lda, B, ldb, C, ldc, M, N, K, part, part ? DW_PART_FLOATS : 0, s);
    const int64_t tiles = (int64_t)((M + 63) / 64) * ((N + 63) / 64);
    int S = (int)((1024 + tiles - 1) / tiles);
    if (S > K / 256) S = K / 256;
    if ((size_t)S * M * N > DW_PART_FLOATS) S = (int)(DW_PART_FLOATS / ((size_t)M * N));
    if (S <= 1 || !part) return gemm_f32(A, lda, B, ldb, C, ldc, nullptr, M, N, K, GEMM_TRANS_A | GEMM_TRANS_B, s);
    const int ks = ((K + S - 1) / S + 31) / 32 * 32;        // k per slice
    const int full = K / ks, rem = K - full * ks;
    int rc;
    GemmArgs g{A, lda, B, ldb, part, N, nullptr, nullptr, 0, M, N, ks, GEMM_TRANS_A | GEMM_TRANS_B, 0.f};
    g.batch = full; g.strideA = (int64_t)ks * lda; g.strideW = (int64_t)ks * ldb; g.strideC = (int64_t)M * N;
    if ((rc = gemm(g, s))) return rc;
    if (rem > 0 && (rc = gemm_f32(A + (int64_t)full * ks * lda, lda, B + (int64_t)full * ks * ldb, ldb, part + (int64_t)full * M * N, N, nullptr, M, N, rem,
                                GEMM_TRANS_A | GEMM_TRANS_B, s))) return rc;
    return splitk_reduce(part, full + (rem > 0), M, N, nullptr, 0, C, ldc, s);
}

// Several contiguous copies / zero fills in ONE launch (the concatenated weight images of a block and the pieces of their gradients: what
// used to be a memset and four to six device-to-device copies per block and pass).  Segments must not overlap.
struct MultiCopy {
    static constexpr int MAX = 10;
    float* dst[MAX]; const float* src[MAX]; int64_t n[MAX];       // src null: zero fill
    int count = 0;
    void add(float* d, const float* s, int64_t len) { if (len > 0) { dst[count] = d; src[count] = s; n[count] = len; ++count; } }
};
__global__ __launch_bounds__(256) void multi_copy_kernel(MultiCopy mc) {
    const int seg = blockIdx.y;
    float* __restrict__ d = mc.dst[seg];
    const float* __restrict__ s = mc.src[seg];
    const int64_t n = mc.n[seg];
    const bool vec = ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s)) & 15) == 0;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (vec) {
        const int64_t n4 = n / 4;
        for (int64_t i = tid; i < n4; i += stride)
            reinterpret_cast<float4*>(d)[i] = s ? reinterpret_cast<const float4*>(s)[i] : float4{0.f, 0.f, 0.f, 0.f};
        for (int64_t i = n4 * 4 + tid; i < n; i += stride) d[i] = s ? s[i] : 0.f;
    } else {
        for (int64_t i = tid; i < n; i += stride) d[i] = s ? s[i] : 0.f;
    }
}
static int multi_copy(const MultiCopy& mc, hipStream_t s) {
    if (mc.count == 0) return 0;
    D4_REQUIRE(mc.count <= MultiCopy::MAX, "multi_copy: too many segments");
    int64_t big = 0;
    for (int i = 0; i < mc.count; ++i) big = mc.n[i] > big ? mc.n[i] : big;
    const int bx = (int)((big / 4 + 255) / 256 < 1 ? 1 : ((big / 4 + 255) / 256 > 512 ? 512 : (big / 4 + 255) / 256));
    hipLaunchKernelGGL(multi_copy_kernel, dim3(bx, mc.count), dim3(256), 0, s, mc);
    D4_LAUNCH_CHECK();
    return 0;
}

struct FfWs {            // workspace carve-up (floats); all leading dimensions are multiples of 4
    float *xn, *w1p, *b1p, *w2p, *h, *u, *du, *dh, *dxn, *tg, *dw1p, *dw2p, *part, *wt;
    size_t total;
};
static FfWs ff_ws(float* base, int R, int D, int I) {
    const size_t Ip = (size_t)ff_ip(I);
    FfWs w{};
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 63) / 64 * 64; return p; };
    w.xn = take((size_t)R * D); w.w1p = take(2 * Ip * D); w.b1p = take(2 * Ip); w.w2p = take((size_t)D * Ip);
    w.h = take((size_t)R * 2 * Ip); w.u = take((size_t)R * Ip); w.du = take((size_t)R * Ip); w.dh = take((size_t)R * 2 * Ip);
    w.dxn = take((size_t)R * D); w.tg = take((size_t)R * D); w.dw1p = take(2 * Ip * D); w.dw2p = take((size_t)D * Ip);
    w.part = take(DW_PART_FLOATS);
    w.wt = take(2 * Ip * D);             // transposed weight image of the input-gradient GEMMs (gemm_dx)
    w.total = off;
    return w;
}

// padded copies of proj_in ([a rows | pad | g rows | pad]), its bias, and proj_out (columns padded), then the forward up to u
static int ff_recompute(const FfWs& w, const float* x, const float* norm_w, const float* w_in, const float* b_in, const float* w_out,
                        int R, int D, int I, hipStream_t s) {
    const int Ip = ff_ip(I);
    int rc;
    MultiCopy mc;
    mc.add(w.w1p, w_in, (int64_t)I * D); mc.add(w.w1p + (size_t)I * D, nullptr, (int64_t)(Ip - I) * D);
    mc.add(w.w1p + (size_t)Ip * D, w_in + (size_t)I * D, (int64_t)I * D); mc.add(w.w1p + (size_t)(Ip + I) * D, nullptr, (int64_t)(Ip - I) * D);
    mc.add(w.b1p, b_in, I); mc.add(w.b1p + I, nullptr, Ip - I); mc.add(w.b1p + Ip, b_in + I, I); mc.add(w.b1p + Ip + I, nullptr, Ip - I);
    if ((rc = multi_copy(mc, s))) return rc;
    if ((rc = pad_cols(w_out, w.w2p, D, I, Ip, s))) return rc;
    if ((rc = rmsnorm_rows(x, D, norm_w, w.xn, D, R, D, RMS_EPS, s))) return rc;
    if ((rc = gemm_b(w.xn, D, w.w1p, D, w.h, 2 * Ip, w.b1p, R, 2 * Ip, D, 0, s))) return rc;
    return swiglu_fwd(w.h, w.u, R, I, Ip, s);
}

// ------------------------------------------------------------------------------------------------ attention core backward
// (AttnBwdArgs, the argument block of the core: attn_tiled.h)

constexpr int AB_S = 64, AB_LD = 65;           // items (tokens of a frame / frames of a trajectory) per group: <= 64 (a score row = one wavefront)
// CAP: token capacity of the LDS arrays (16 or 32): at <= 16 tokens per group the block needs 27 KB instead of 60 KB of LDS, so five blocks
// instead of two share a CU — the kernel is a chain of LDS reads and wave reductions, and the extra waves are what hides them
template <int DH, int CAP>
__global__ __launch_bounds__(256) void attn_bwd_kernel(AttnBwdArgs p) {
    extern __shared__ float ab_s[];             // dynamic: 27 KB (CAP 16), 60 KB (32), 134 KB (64: one block per CU)
    float* qs = ab_s; float* kn = qs + CAP * AB_LD; float* kh = kn + CAP * AB_LD; float* vm = kh + CAP * AB_LD; float* dO = vm + CAP * AB_LD;
    float* dvm = dO + CAP * AB_LD;
    float* P = dvm + CAP * AB_LD; float* dsm = P + CAP * (CAP + 1);
    float* kinv = dsm + CAP * (CAP + 1); float* vinv = kinv + CAP; float* mxs = vinv + CAP; float* gts = mxs + CAP;
    __shared__ float gpart[4][64];
    const int S = p.S, hd = p.heads * DH;
    const int f = blockIdx.x / p.heads, h = blockIdx.x % p.heads;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool on = lane < DH;
    const int64_t row0 = (int64_t)(f / p.g_inner) * p.g_outer_stride + (f % p.g_inner);
    const int64_t ist = p.item_stride;
    const float sc = on ? (p.gamma[h * DH + lane] + 1.f) * sqrtf((float)DH) : 0.f;
    const float scale = rsqrtf((float)DH);
    const bool bwd = p.d_o3 != nullptr;

    // rotary (D4:1626-1659): t * cos + rotate_half(t) * sin with rotate_half(t)[d] = d < DH/2 ? -t[d + DH/2] : t[d - DH/2]; the partner
    // feature is lane ^ (DH/2).  rot_t is the transpose (backward): y * cos + rotate_half^T(y * sin), rotate_half^T(z)[d] = d < DH/2 ? z[d + DH/2] : -z[d - DH/2]
    const float freq = (p.inv_freq && on) ? p.inv_freq[lane & (DH / 2 - 1)] : 0.f;
    const bool lo_half = lane < DH / 2;
    auto rot = [&](float t, int pos) {
        if (!p.inv_freq) return t;
        float sn, cs;
        sincosf(freq * (float)pos, &sn, &cs);
        const float partner = __shfl(t, lane ^ (DH / 2));
        return on ? t * cs + (lo_half ? -partner : partner) * sn : 0.f;
    };
    auto rot_t = [&](float y, int pos) {
        if (!p.inv_freq) return y;
        float sn, cs;
        sincosf(freq * (float)pos, &sn, &cs);
        const float partner = __shfl(y * sn, lane ^ (DH / 2));
        return on ? y * cs + (lo_half ? partner : -partner) : 0.f;
    };

    // ---- phase A: per token j: value mix, key normalisation
    for (int j = w; j < S; j += 4) {
        const float* pr = p.proj + (row0 + j * ist) * p.ldp;
        const float qv = on ? pr[h * DH + lane] : 0.f, kv = on ? pr[hd + h * DH + lane] : 0.f;
        float vv = on ? pr[2 * hd + h * DH + lane] : 0.f;
        float mx = 0.f;
        if (p.rv) {
            mx = sigm(pr[3 * hd + p.hp4 + h]);
            const float r = on ? p.rv[(row0 + j * ist) * hd + h * DH + lane] : 0.f;
            vv = vv + mx * (r - vv);
        }
        const float ki = 1.f / fmaxf(sqrtf(wave_sum(kv * kv)), 1e-12f);
        const float vi = 1.f / fmaxf(sqrtf(wave_sum(vv * vv)), 1e-12f);
        qs[j * AB_LD + lane] = rot(qv, j); kh[j * AB_LD + lane] = kv * ki; kn[j * AB_LD + lane] = rot(kv * ki * sc, j);
        vm[j * AB_LD + lane] = vv;
        if (lane == 0) { kinv[j] = ki; vinv[j] = vi; mxs[j] = mx; gts[j] = sigm(pr[3 * hd + h]); }
    }
    __syncthreads();

    // ---- phase B: per query i (lane = key j for the score row, lane = feature for the vectors)
    const int first_special = S - p.num_special;
    for (int i = w; i < S; i += 4) {
        float dot = 0.f;
        if (lane < S) {
#pragma unroll 8
            for (int d = 0; d < DH; ++d) dot += qs[i * AB_LD + d] * kn[lane * AB_LD + d];
        }
        const float sim = dot * scale;
        float th = 0.f, simc = sim;
        if (p.softclamp > 0.f) { th = tanhf(sim / p.softclamp); simc = th * p.softclamp; }
        const bool visible = lane < S && !(i < first_special && lane >= first_special) && !(p.causal && lane > i);
        simc = visible ? simc : -FLT_MAX;
        float m = simc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
        const float e = visible ? expf(simc - m) : 0.f;
        const float pij = e / wave_sum(e);
        // o_i = sum_j P_ij vm_j
        float o = 0.f;
        for (int j = 0; j < S; ++j) o += __shfl(pij, j) * vm[j * AB_LD + lane];
        const float vni = vm[i * AB_LD + lane] * vinv[i];
        const float sdot = p.belief ? wave_sum(o * vni) : 0.f;
        const float o2 = o - sdot * vni;
        const float gt = gts[i];
        if (on) p.o3[(row0 + i * ist) * hd + h * DH + lane] = o2 * gt;
        if (!bwd) continue;
        const float d3 = on ? p.d_o3[(row0 + i * ist) * hd + h * DH + lane] : 0.f;
        const float dgl = wave_sum(d3 * o2) * gt * (1.f - gt);
        if (lane == 0) p.dproj[(row0 + i * ist) * p.ldp + 3 * hd + h] = dgl;
        const float d2 = d3 * gt;
        float dOi = d2, dvdir = 0.f;
        if (p.belief) {
            const float c2 = wave_sum(d2 * vni);
            dOi = d2 - c2 * vni;
            const float dvn = -(sdot * d2 + c2 * o);
            dvdir = (dvn - wave_sum(dvn * vni) * vni) * vinv[i];
        }
        dO[i * AB_LD + lane] = dOi;
        dvm[i * AB_LD + lane] = dvdir;
        // dP_ij = dO_i . vm_j  (lane = j)
        float dp = 0.f;
        if (lane < S) {
#pragma unroll 8
            for (int d = 0; d < DH; ++d) dp += dO[i * AB_LD + d] * vm[lane * AB_LD + d];
        }
        const float rowdot = wave_sum(pij * dp);
        float dsim = pij * (dp - rowdot);
        if (p.softclamp > 0.f) dsim *= 1.f - th * th;
        dsim *= scale;
        if (lane < S) { P[i * (CAP + 1) + lane] = pij; dsm[i * (CAP + 1) + lane] = dsim; }
        // dq_i = sum_j dsim_ij kn_j
        float dq = 0.f;
        for (int j = 0; j < S; ++j) dq += __shfl(dsim, j) * kn[j * AB_LD + lane];
        dq = rot_t(dq, i);
        if (on) p.dproj[(row0 + i * ist) * p.ldp + h * DH + lane] = dq;
    }
    if (!bwd) return;
    __syncthreads();

    // ---- phase C: per key / value token j (lane = feature)
    float gacc = 0.f;
    for (int j = w; j < S; j += 4) {
        float dkn = 0.f, dv = dvm[j * AB_LD + lane];
        for (int i = 0; i < S; ++i) {
            dkn += dsm[i * (CAP + 1) + j] * qs[i * AB_LD + lane];
            dv += P[i * (CAP + 1) + j] * dO[i * AB_LD + lane];
        }
        dkn = rot_t(dkn, j);
        const float khj = kh[j * AB_LD + lane];
        gacc += dkn * khj;
        const float dkh = dkn * sc;
        const float dk = (dkh - wave_sum(dkh * khj) * khj) * kinv[j];
        float* dr = p.dproj + (row0 + j * ist) * p.ldp;
        if (on) dr[hd + h * DH + lane] = dk;
        if (p.rv) {
            const float mx = mxs[j];
            const float* pr = p.proj + (row0 + j * ist) * p.ldp;
            const float vraw = on ? pr[2 * hd + h * DH + lane] : 0.f;
            const float r = on ? p.rv[(row0 + j * ist) * hd + h * DH + lane] : 0.f;
            const float dmx = wave_sum(dv * (r - vraw));
            if (on) { dr[2 * hd + h * DH + lane] = dv * (1.f - mx); p.d_rv[(row0 + j * ist) * hd + h * DH + lane] = dv * mx; }
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

// `tiled`: the per-row planes of the tiled core (attn_tiled.hip), given under the rule of attn_tiled(): the time geometry above AB_S frames, the
// within-frame geometry above AB_S tokens with d4_train_wide_set(1), either at any size when its test hook asks
static int attn_core(const AttnBwdArgs& a, int dh, hipStream_t s, float* tiled = nullptr) {
    if (a.F * a.heads == 0) return 0;
    if (tiled) return attn_bf16() ? attn_tiled_bf16_core(a, dh, tiled, s) : attn_tiled_core(a, dh, tiled, s);
    auto lds_of = [](int cap) { return (size_t)(6 * cap * AB_LD + 2 * cap * (cap + 1) + 4 * cap) * sizeof(float); };
    static DeviceOnce attr_set;
    if (attr_set.need()) {
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_kernel<64, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of(64)));
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_kernel<32, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of(64)));
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_kernel<16, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of(64)));
        attr_set.done();
    }
    const dim3 grid(a.F * a.heads), block(256);
    const int cap = a.S <= 16 ? 16 : (a.S <= 32 ? 32 : 64);
#define D4_AB_LAUNCH(DH_, CAP_) do { note_train_form(false, "attn_bwd_kernel<" #DH_ "," #CAP_ ">"); \
                                     hipLaunchKernelGGL((attn_bwd_kernel<DH_, CAP_>), grid, block, lds_of(CAP_), s, a); } while (0)
    if (dh == 64) { if (cap == 16) D4_AB_LAUNCH(64, 16); else if (cap == 32) D4_AB_LAUNCH(64, 32); else D4_AB_LAUNCH(64, 64); }
    else if (dh == 32) { if (cap <= 32) D4_AB_LAUNCH(32, 32); else D4_AB_LAUNCH(32, 64); }
    else { if (cap <= 32) D4_AB_LAUNCH(16, 32); else D4_AB_LAUNCH(16, 64); }
#undef D4_AB_LAUNCH
    D4_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ cross-attention core
// The trunk's cross attentions (D4:1968-2075 with a context): the AttentionPool over the stack of layer hiddens (one query per token,
// D4:2143-2177), the final special-token cross attention (D4:3227-3234) and the learned-query pools (D4:2179-2210).  No value residual,
// no belief projection (the reference skips it when a context is given), optional soft clamp.  One block per (group, head); up to 64
// queries and 64 keys in (dynamic) LDS.  projq rows: q @ 0, gate logit @ hd + head; projk rows: k @ 0, v @ hd.
// (XAttnArgs, the argument block of the core: attn_tiled.h)

constexpr int XA_N = 64;
template <int DH>
__global__ __launch_bounds__(256) void xattn_bwd_kernel(XAttnArgs p) {
    extern __shared__ float xa_s[];
    const int nq = p.nq, nk = p.nk, hd = p.heads * DH;
    float* kn = xa_s;                           // [nk][65]
    float* kh = kn + nk * AB_LD;
    float* vs = kh + nk * AB_LD;
    float* qs = vs + nk * AB_LD;                // [nq][65]
    float* dO = qs + nq * AB_LD;
    float* P = dO + nq * AB_LD;                 // [nq][65]
    float* dsm = P + nq * AB_LD;
    float* kinv = dsm + nq * AB_LD;             // [nk]
    float* gts = kinv + nk;                     // [nq]
    float* gpart = gts + nq;                    // [4][64]
    const int g = blockIdx.x / p.heads, h = blockIdx.x % p.heads;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool on = lane < DH;
    const float sc = on ? (p.gamma[h * DH + lane] + 1.f) * sqrtf((float)DH) : 0.f;
    const float scale = rsqrtf((float)DH);
    const bool bwd = p.d_o3 != nullptr;
    auto krow = [&](int j) { return p.item_major ? (int64_t)j * p.G + g : (int64_t)g * nk + j; };

    for (int j = w; j < nk; j += 4) {
        const float* pr = p.projk + krow(j) * p.ldk;
        const float kv = on ? pr[h * DH + lane] : 0.f, vv = on ? pr[hd + h * DH + lane] : 0.f;
        const float ki = 1.f / fmaxf(sqrtf(wave_sum(kv * kv)), 1e-12f);
        kh[j * AB_LD + lane] = kv * ki; kn[j * AB_LD + lane] = kv * ki * sc; vs[j * AB_LD + lane] = vv;
        if (lane == 0) kinv[j] = ki;
    }
    for (int i = w; i < nq; i += 4) {
        const float* pr = p.projq + ((int64_t)g * nq + i) * p.ldq;
        qs[i * AB_LD + lane] = on ? pr[h * DH + lane] : 0.f;
        if (lane == 0) gts[i] = sigm(pr[hd + h]);
    }
    __syncthreads();

    for (int i = w; i < nq; i += 4) {
        const int64_t qrow = (int64_t)g * nq + i;
        float dot = 0.f;
        if (lane < nk) {
#pragma unroll 8
            for (int d = 0; d < DH; ++d) dot += qs[i * AB_LD + d] * kn[lane * AB_LD + d];
        }
        const float sim = dot * scale;
        float th = 0.f, simc = sim;
        if (p.softclamp > 0.f) { th = tanhf(sim / p.softclamp); simc = th * p.softclamp; }
        simc = lane < nk ? simc : -FLT_MAX;
        float m = simc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
        const float e = lane < nk ? expf(simc - m) : 0.f;
        const float pij = e / wave_sum(e);
        float o = 0.f;
        for (int j = 0; j < nk; ++j) o += __shfl(pij, j) * vs[j * AB_LD + lane];
        const float gt = gts[i];
        if (on) p.o3[qrow * hd + h * DH + lane] = o * gt;
        if (!bwd) continue;
        const float d3 = on ? p.d_o3[qrow * hd + h * DH + lane] : 0.f;
        const float dgl = wave_sum(d3 * o) * gt * (1.f - gt);
        if (lane == 0) p.dprojq[qrow * p.ldq + hd + h] = dgl;
        const float dOi = d3 * gt;
        dO[i * AB_LD + lane] = dOi;
        float dp = 0.f;
        if (lane < nk) {
#pragma unroll 8
            for (int d = 0; d < DH; ++d) dp += dO[i * AB_LD + d] * vs[lane * AB_LD + d];
        }
        const float rowdot = wave_sum(pij * dp);
        float dsim = pij * (dp - rowdot);
        if (p.softclamp > 0.f) dsim *= 1.f - th * th;
        dsim *= scale;
        if (lane < nk) { P[i * AB_LD + lane] = pij; dsm[i * AB_LD + lane] = dsim; }
        float dq = 0.f;
        for (int j = 0; j < nk; ++j) dq += __shfl(dsim, j) * kn[j * AB_LD + lane];
        if (on) p.dprojq[qrow * p.ldq + h * DH + lane] = dq;
    }
    if (!bwd) return;
    __syncthreads();

    float gacc = 0.f;
    for (int j = w; j < nk; j += 4) {
        float dkn = 0.f, dv = 0.f;
        for (int i = 0; i < nq; ++i) {
            dkn += dsm[i * AB_LD + j] * qs[i * AB_LD + lane];
            dv += P[i * AB_LD + j] * dO[i * AB_LD + lane];
        }
        const float khj = kh[j * AB_LD + lane];
        gacc += dkn * khj;
        const float dkh = dkn * sc;
        const float dk = (dkh - wave_sum(dkh * khj) * khj) * kinv[j];
        float* dr = p.dprojk + krow(j) * p.ldk;
        if (on) { dr[h * DH + lane] = dk; dr[hd + h * DH + lane] = dv; }
    }
    gpart[w * 64 + lane] = gacc;
    __syncthreads();
    if (w == 0 && on) p.dgamma_part[(int64_t)g * hd + h * DH + lane] = (((gpart[lane] + gpart[64 + lane]) + gpart[128 + lane]) + gpart[192 + lane]) * sqrtf((float)DH);
}

// `tiled`: the planes of the tiled core, given when a side has more than XA_N items with d4_train_wide_set(1) (or the test hook asks)
static int xattn_core(const XAttnArgs& a, int dh, hipStream_t s, float* tiled = nullptr) {
    if (a.G * a.heads == 0) return 0;
    if (tiled) return attn_bf16() ? attn_tiled_bf16_cross_core(a, dh, tiled, s) : attn_tiled_cross_core(a, dh, tiled, s);
    const size_t lds = sizeof(float) * ((size_t)(3 * a.nk + 4 * a.nq) * AB_LD + a.nk + a.nq + 256);
    static DeviceOnce attr_set;
    if (attr_set.need()) {
        const int mx = (int)(sizeof(float) * ((size_t)7 * XA_N * AB_LD + 2 * XA_N + 256));
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn_bwd_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, mx));
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn_bwd_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, mx));
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn_bwd_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, mx));
        attr_set.done();
    }
    note_train_form(true, dh == 64 ? "xattn_bwd_kernel<64>" : dh == 32 ? "xattn_bwd_kernel<32>" : "xattn_bwd_kernel<16>");
    if (dh == 64) hipLaunchKernelGGL(xattn_bwd_kernel<64>, dim3(a.G * a.heads), dim3(256), lds, s, a);
    else if (dh == 32) hipLaunchKernelGGL(xattn_bwd_kernel<32>, dim3(a.G * a.heads), dim3(256), lds, s, a);
    else hipLaunchKernelGGL(xattn_bwd_kernel<16>, dim3(a.G * a.heads), dim3(256), lds, s, a);
    D4_LAUNCH_CHECK();
    return 0;
}

__global__ void zero_pad_cols_kernel(float* x, int rows, int ld, int c0, int c1) {
    const int n = c1 - c0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (int64_t)rows * n; i += (int64_t)gridDim.x * blockDim.x)
        x[(i / n) * ld + c0 + (int)(i % n)] = 0.f;
}
// columns c0 .. c1 of x [rows][ld] set to zero (nothing to do for an empty range)
static int zero_pad_cols(float* x, int rows, int ld, int c0, int c1, hipStream_t s) {
    if (c1 <= c0 || rows == 0) return 0;
    hipLaunchKernelGGL(zero_pad_cols_kernel, grid_for((int64_t)rows * (c1 - c0)), dim3(256), 0, s, x, rows, ld, c0, c1);
    D4_LAUNCH_CHECK();
    return 0;
}

struct AttnWs {
    float *xn, *wcat, *bcat, *proj, *dproj, *d_o3, *o3, *dwcat, *tg, *dxn, *gpart, *part, *wt;
    float* tiled;                    // per-row planes of the tiled core, last, so that every other offset is the same with and without them
    size_t total;
    int P, hp4;
};
static AttnWs attn_ws(float* base, int R, int F, int D, int heads, int dh, bool tiled = false) {
    AttnWs w{};
    const int hd = heads * dh;
    w.hp4 = (heads + 3) / 4 * 4;
    w.P = (3 * hd + 2 * w.hp4 + 31) / 32 * 32;       // a multiple of 32: P is the contraction length of the input-gradient GEMM (gemm_dx)
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 63) / 64 * 64; return p; };
    w.xn = take((size_t)R * D); w.wcat = take((size_t)w.P * D); w.bcat = take(w.P); w.proj = take((size_t)R * w.P); w.dproj = take((size_t)R * w.P);
    w.d_o3 = take((size_t)R * hd); w.o3 = take((size_t)R * hd); w.dwcat = take((size_t)w.P * D); w.tg = take((size_t)R * D); w.dxn = take((size_t)R * D);
    w.gpart = take((size_t)F * hd);
    w.part = take(DW_PART_FLOATS);
    w.wt = take((size_t)w.P * D);
    if (tiled) w.tiled = take(attn_bf16() && F > 0 ? attn_tiled_bf16_floats(F, R / F, heads, dh) : attn_tiled_floats(R, heads, dh));
    w.total = off;
    return w;
}

// bf16-arithmetic scratch of a block (bytes): see bf16_extra_bytes
static size_t ff_bf16_extra(int R, int D, int I) { const size_t w2 = 2 * (size_t)ff_ip(I); return bf16_extra_bytes(R, w2 > (size_t)D ? w2 : D, w2, D); }
static size_t attn_bf16_extra(int R, int D, int hd) { return bf16_extra_bytes(R, 3 * hd > D ? 3 * hd : D, 3 * hd, D); }

struct AttnParams { const float *norm_w, *wq, *wk, *wv, *wo, *wg, *wm, *bm, *gamma; };

// concatenated projection [q | k | v | gates (hp4) | mix (hp4)] and the forward up to the projections
static int attn_project(const AttnWs& w, const float* x, const AttnParams& prm, int R, int D, int heads, int dh, bool has_rv, hipStream_t s) {
    const int hd = heads * dh;
    int rc;
    {   // rows of wcat: q | k | v | gates, pad to hp4 | mix (or zero), pad to P;  bcat: zero but for the mix bias
        const int64_t blk = (int64_t)hd * D;
        const int mix0 = 3 * hd + w.hp4;
        MultiCopy mc;
        mc.add(w.wcat, prm.wq, blk); mc.add(w.wcat + blk, prm.wk, blk); mc.add(w.wcat + 2 * blk, prm.wv, blk);
        mc.add(w.wcat + 3 * blk, prm.wg, (int64_t)heads * D); mc.add(w.wcat + 3 * blk + (int64_t)heads * D, nullptr, (int64_t)(w.hp4 - heads) * D);
        mc.add(w.wcat + (int64_t)mix0 * D, has_rv ? prm.wm : nullptr, (int64_t)heads * D);
        mc.add(w.wcat + (int64_t)(mix0 + heads) * D, nullptr, (int64_t)(w.P - mix0 - heads) * D);
        mc.add(w.bcat, nullptr, mix0); mc.add(w.bcat + mix0, has_rv ? prm.bm : nullptr, heads); mc.add(w.bcat + mix0 + heads, nullptr, w.P - mix0 - heads);
        if ((rc = multi_copy(mc, s))) return rc;
    }
    if ((rc = rmsnorm_rows(x, D, prm.norm_w, w.xn, D, R, D, RMS_EPS, s))) return rc;
    if (!t_bf.a) return gemm_b(w.xn, D, w.wcat, D, w.proj, w.P, w.bcat, R, w.P, D, 0, s);
    // bf16 training arithmetic: q | k | v (their bias rows are zero) on the bf16 pipe, the heads-wide gate and mix logits stay an fp32 product
    if ((rc = gemm_b(w.xn, D, w.wcat, D, w.proj, w.P, nullptr, R, 3 * hd, D, 0, s))) return rc;
    return gemm_f32(w.xn, D, w.wcat + (size_t)3 * hd * D, D, w.proj + 3 * hd, w.P, w.bcat + 3 * hd, R, w.P - 3 * hd, D, 0, s);
}

}  // namespace d4

using namespace d4;

extern "C" {

size_t d4_ff_workspace_bytes(int rows, int dim, int inner) { return ff_ws(nullptr, rows, dim, inner).total * sizeof(float); }
size_t d4_ff_bf16_scratch_bytes(int rows, int dim, int inner) { return ff_bf16_extra(rows, dim, inner); }
int d4_train_scratch_bind(void* scratch, size_t bytes) { t_scratch.p = scratch; t_scratch.bytes = scratch ? bytes : 0; return 0; }
int d4_train_arith_set(int arith) { return g_train_arith.exchange(arith ? 1 : 0); }
int d4_train_arith_get(void) { return g_train_arith.load(); }
int d4_train_wide_set(int on) { return g_train_wide.exchange(on ? 1 : 0); }
int d4_train_attn_products_set(int products) {
    if (products != 0 && products != 1) { set_error("d4_train_attn_products_set: products %d (0: fp32, 1: bf16)", products); return -1; }
    return g_train_attn_products.exchange(products);
}

int d4_ff_forward(const float* x, const float* norm_w, const float* w_in, const float* b_in, const float* w_out, const float* b_out,
                  int rows, int dim, int inner, float* y, float* workspace, size_t workspace_bytes, void* stream) {
    D4_REQUIRE(x && norm_w && w_in && b_in && w_out && b_out && y && workspace, "d4_ff_forward: null argument");
    D4_REQUIRE(dim % 4 == 0 && ((uintptr_t)workspace % 256) == 0, "d4_ff_forward: dim must be a multiple of 4 and the workspace 256-byte aligned");
    D4_REQUIRE(workspace_bytes >= d4_ff_workspace_bytes(rows, dim, inner), "d4_ff_forward: workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rows == 0) return 0;
    const FfWs w = ff_ws(workspace, rows, dim, inner);
    const int Ip = ff_ip(inner);
    int rc;
    Bf16Scope bf;
    if ((rc = bf.enter("d4_ff_forward", rows, Ip * 2 > dim ? Ip * 2 : dim, 2 * Ip, dim))) return rc;
    if ((rc = ff_recompute(w, x, norm_w, w_in, b_in, w_out, rows, dim, inner, s))) return rc;
    return gemm_b(w.u, Ip, w.w2p, Ip, y, dim, b_out, rows, dim, Ip, 0, s);
}

// `reuse`: the workspace is the one the matching forward call ran in and still holds its intermediates (normalised input, padded weight
// images, pre-activation h, hidden u): nothing is recomputed.  Otherwise the forward up to u is recomputed from x first.
static int ff_backward_impl(const float* x, const float* dy, const float* norm_w, const float* w_in, const float* b_in, const float* w_out,
                   int rows, int dim, int inner, float* dx, float* d_norm_w, float* d_w_in, float* d_b_in, float* d_w_out, float* d_b_out,
                   float* workspace, size_t workspace_bytes, void* stream, bool reuse) {
    D4_REQUIRE(x && dy && norm_w && w_in && b_in && w_out && dx && d_norm_w && d_w_in && d_b_in && d_w_out && d_b_out && workspace, "d4_ff_backward: null argument");
    D4_REQUIRE(dim % 4 == 0 && ((uintptr_t)workspace % 256) == 0, "d4_ff_backward: dim must be a multiple of 4 and the workspace 256-byte aligned");
    D4_REQUIRE(workspace_bytes >= d4_ff_workspace_bytes(rows, dim, inner), "d4_ff_backward: workspace too small");
    D4_REQUIRE(rows >= 1, "d4_ff_backward: no rows");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int R = rows, D = dim, I = inner, Ip = ff_ip(inner);
    const FfWs w = ff_ws(workspace, R, D, I);
    int rc;
    Bf16Scope bf;
    if ((rc = bf.enter("d4_ff_backward", R, Ip * 2 > D ? Ip * 2 : D, 2 * Ip, D))) return rc;
    if (!reuse && (rc = ff_recompute(w, x, norm_w, w_in, b_in, w_out, R, D, I, s))) return rc;
    // y = u W2^T + b2
    if ((rc = gemm_dw(dy, D, w.u, Ip, w.dw2p, Ip, D, Ip, R, w.part, s))) return rc;                                    // dW2 = dy^T u
    if ((rc = copy_rows(w.dw2p, Ip, d_w_out, I, D, I, s))) return rc;
    if ((rc = lin_dx(dy, D, w.w2p, Ip, w.du, Ip, R, Ip, D, w.wt, s))) return rc;                                        // du = dy W2
    if ((rc = swiglu_bwd(w.h, w.du, w.dh, R, I, Ip, s))) return rc;
    image_a_written(w.dh);
    // h = xn W1^T + b1
    if ((rc = gemm_dw(w.dh, 2 * Ip, w.xn, D, w.dw1p, D, 2 * Ip, D, R, w.part, s))) return rc;                          // dW1 = dh^T xn
    {
        MultiCopy mc;
        mc.add(d_w_in, w.dw1p, (int64_t)I * D); mc.add(d_w_in + (size_t)I * D, w.dw1p + (size_t)Ip * D, (int64_t)I * D);
        if ((rc = multi_copy(mc, s))) return rc;
    }
    if ((rc = lin_dx(w.dh, 2 * Ip, w.w1p, D, w.dxn, D, R, D, 2 * Ip, w.wt, s))) return rc;                             // dxn = dh W1
    // xn = rmsnorm(x) * gamma
    if ((rc = rmsnorm_bwd(x, w.dxn, norm_w, w.tg, dx, R, D, RMS_EPS, s))) return rc;
    // the four column sums of the block (both bias gradients, the norm gain's) in one launch: their operands are all still in place
    ColsumBatch cb;
    cb.add(dy, D, R, D, d_b_out); cb.add(w.dh, 2 * Ip, R, I, d_b_in); cb.add(w.dh + Ip, 2 * Ip, R, I, d_b_in + I); cb.add(w.tg, D, R, D, d_norm_w);
    return colsum_batch(cb, s);
}

int d4_ff_backward(const float* x, const float* dy, const float* norm_w, const float* w_in, const float* b_in, const float* w_out,
                   int rows, int dim, int inner, float* dx, float* d_norm_w, float* d_w_in, float* d_b_in, float* d_w_out, float* d_b_out,
                   float* workspace, size_t workspace_bytes, void* stream) {
    return ff_backward_impl(x, dy, norm_w, w_in, b_in, w_out, rows, dim, inner, dx, d_norm_w, d_w_in, d_b_in, d_w_out, d_b_out, workspace, workspace_bytes, stream, false);
}
int d4_ff_backward_saved(const float* x, const float* dy, const float* norm_w, const float* w_in, const float* b_in, const float* w_out,
                         int rows, int dim, int inner, float* dx, float* d_norm_w, float* d_w_in, float* d_b_in, float* d_w_out, float* d_b_out,
                         float* workspace, size_t workspace_bytes, void* stream) {
    return ff_backward_impl(x, dy, norm_w, w_in, b_in, w_out, rows, dim, inner, dx, d_norm_w, d_w_in, d_b_in, d_w_out, d_b_out, workspace, workspace_bytes, stream, true);
}

size_t d4_attn_workspace_bytes(int frames, int tokens, int dim, int heads, int dim_head) {
    return attn_ws(nullptr, frames * tokens, frames, dim, heads, dim_head, space_tiled(tokens)).total * sizeof(float);
}
size_t d4_attn_bf16_scratch_bytes(int rows, int dim, int heads, int dim_head) { return attn_bf16_extra(rows, dim, heads * dim_head); }

// Operator-level test entry points of the glue launchers of this file: the launchers the blocks call.
int d4_swiglu(int bwd, const float* h, const float* du, float* out, int rows, int inner, int inner_pad, void* stream) {
    D4_REQUIRE(h && out && rows >= 1 && inner >= 1 && inner_pad >= inner && (bwd == 0 || (bwd == 1 && du)), "d4_swiglu: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return bwd ? swiglu_bwd(h, du, out, rows, inner, inner_pad, s) : swiglu_fwd(h, out, rows, inner, inner_pad, s);
}
int d4_multi_copy(int count, float* const* dst, const float* const* src, const int64_t* n, void* stream) {
    D4_REQUIRE(count >= 0 && count <= MultiCopy::MAX, "multi_copy: too many segments");
    D4_REQUIRE(count == 0 || (dst && src && n), "d4_multi_copy: bad arguments");
    MultiCopy mc;
    for (int i = 0; i < count; ++i) {
        D4_REQUIRE(n[i] >= 0 && (dst[i] || n[i] == 0), "d4_multi_copy: bad arguments of segment %d", i);
        mc.add(dst[i], src[i], n[i]);
    }
    return multi_copy(mc, static_cast<hipStream_t>(stream));
}
int d4_zero_pad_cols(float* x, int rows, int ld, int c0, int c1, void* stream) {
    D4_REQUIRE(x && rows >= 0 && c0 >= 0 && c1 >= c0 && ld >= c1, "d4_zero_pad_cols: bad arguments");
    return zero_pad_cols(x, rows, ld, c0, c1, static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace {

struct AttnGeom {                  // how the rows of x group into attention problems (see AttnBwdArgs)
    int groups, items, g_inner; int64_t g_outer_stride, item_stride;
    int causal, num_special; const float* inv_freq;
};

// the time geometry (causal, rotary) takes the tiled core above AB_S frames, and at any length under the test hook; the within-frame
// geometry (neither) above AB_S tokens with d4_train_wide_set(1), and at any size under its own hook
bool attn_tiled(const AttnGeom& g) {
    if (g.causal && g.inv_freq) return g.items > AB_S || g_time_attn_tiled != 0;
    return !g.causal && !g.inv_freq && space_tiled(g.items);
}

int attn_check(int rows, const AttnGeom& g, int dim, int heads, int dim_head, const float* workspace, size_t workspace_bytes) {
    if (g.causal && g.inv_freq) D4_REQUIRE(g.items >= 1 && g.items <= ATT_MAX_FRAMES, "time attention block: %d frames per trajectory (max %d)", g.items, ATT_MAX_FRAMES);
    else {
        const int cap = g_train_wide.load() ? ATT_MAX_FRAMES : AB_S;
        D4_REQUIRE(g.items >= 1 && g.items <= cap, "attention block: %d items per group (max %d)", g.items, cap);
    }
    D4_REQUIRE(dim_head == 16 || dim_head == 32 || dim_head == 64, "attention block: head dim %d (16, 32 or 64)", dim_head);
    D4_REQUIRE(dim % 4 == 0 && ((uintptr_t)workspace % 256) == 0, "attention block: dim must be a multiple of 4 and the workspace 256-byte aligned");
    D4_REQUIRE(workspace_bytes >= attn_ws(nullptr, rows, g.groups, dim, heads, dim_head, attn_tiled(g)).total * sizeof(float), "attention block: workspace too small");
    return 0;
}

void set_geom(AttnBwdArgs& a, const AttnGeom& g) {
    a.g_inner = g.g_inner; a.g_outer_stride = g.g_outer_stride; a.item_stride = g.item_stride; a.causal = g.causal; a.inv_freq = g.inv_freq;
}

int attn_block_forward(const float* x, const float* residual_values, const AttnParams& prm, int rows, const AttnGeom& g, int dim, int heads, int dim_head,
                       float softclamp, int belief, float* y, float* workspace, size_t workspace_bytes, hipStream_t s) {
    D4_REQUIRE(x && prm.norm_w && prm.wq && prm.wk && prm.wv && prm.wo && prm.wg && prm.gamma && y && workspace, "attention forward: null argument");
    D4_REQUIRE(!residual_values || (prm.wm && prm.bm), "attention forward: residual values need the mix projection");
    int rc;
    if ((rc = attn_check(rows, g, dim, heads, dim_head, workspace, workspace_bytes))) return rc;
    const int R = rows, hd = heads * dim_head;
    if (R == 0) return 0;
    const AttnWs w = attn_ws(workspace, R, g.groups, dim, heads, dim_head, attn_tiled(g));
    Bf16Scope bf;
    if ((rc = bf.enter("attention forward", R, 3 * hd > dim ? 3 * hd : dim, 3 * hd, dim))) return rc;
    if ((rc = attn_project(w, x, prm, R, dim, heads, dim_head, residual_values != nullptr, s))) return rc;
    AttnBwdArgs a{w.proj, w.P, residual_values, prm.gamma, nullptr, w.o3, nullptr, nullptr, nullptr, g.groups, g.items, heads, w.hp4, softclamp, g.num_special, belief};
    set_geom(a, g);
    if ((rc = attn_core(a, dim_head, s, w.tiled))) return rc;
    return gemm_b(w.o3, hd, prm.wo, hd, y, dim, nullptr, R, dim, hd, 0, s);
}

struct AttnGrads { float *dx, *d_rv, *d_norm_w, *d_wq, *d_wk, *d_wv, *d_wo, *d_wg, *d_wm, *d_bm, *d_gamma; };

int attn_block_backward(const float* x, const float* residual_values, const float* dy, const AttnParams& prm, int rows, const AttnGeom& g, int dim,
                        int heads, int dim_head, float softclamp, int belief, const AttnGrads& o, float* workspace, size_t workspace_bytes, hipStream_t s,
                        bool reuse = false) {
    D4_REQUIRE(x && dy && prm.norm_w && prm.wq && prm.wk && prm.wv && prm.wo && prm.wg && prm.gamma && workspace, "attention backward: null argument");
    D4_REQUIRE(o.dx && o.d_norm_w && o.d_wq && o.d_wk && o.d_wv && o.d_wo && o.d_wg && o.d_gamma, "attention backward: null gradient output");
    D4_REQUIRE(!residual_values || (prm.wm && prm.bm && o.d_rv && o.d_wm && o.d_bm), "attention backward: residual values need the mix projection and its gradients");
    int rc;
    if ((rc = attn_check(rows, g, dim, heads, dim_head, workspace, workspace_bytes))) return rc;
    D4_REQUIRE(rows >= 1, "attention backward: no rows");
    const int R = rows, D = dim, hd = heads * dim_head;
    const bool has_rv = residual_values != nullptr;
    const AttnWs w = attn_ws(workspace, R, g.groups, D, heads, dim_head, attn_tiled(g));
    Bf16Scope bf;
    if ((rc = bf.enter("attention backward", R, 3 * hd > D ? 3 * hd : D, 3 * hd, D))) return rc;
    if (!reuse && (rc = attn_project(w, x, prm, R, D, heads, dim_head, has_rv, s))) return rc;     // reuse: the forward's xn / wcat / proj are still there
    // out = o3 Wo^T
    if ((rc = lin_dx(dy, D, prm.wo, hd, w.d_o3, hd, R, hd, D, w.wt, s))) return rc;                                     // d_o3 = dy Wo
    AttnBwdArgs a{w.proj, w.P, residual_values, prm.gamma, w.d_o3, w.o3, w.dproj, o.d_rv, w.gpart, g.groups, g.items, heads, w.hp4, softclamp, g.num_special, belief};
    set_geom(a, g);
    if ((rc = attn_core(a, dim_head, s, w.tiled))) return rc;
    image_a_written(w.dproj);
    // the pad columns of the gate / mix logits and of the row carry no gradient
    if ((rc = zero_pad_cols(w.dproj, R, w.P, 3 * hd + heads, 3 * hd + w.hp4, s))) return rc;
    if ((rc = zero_pad_cols(w.dproj, R, w.P, 3 * hd + w.hp4 + heads, w.P, s))) return rc;
    if ((rc = gemm_dw(dy, D, w.o3, hd, o.d_wo, hd, D, hd, R, w.part, s))) return rc;                                     // dWo = dy^T o3
    // projections: dW = dproj^T xn, dxn = dproj Wcat
    if (!t_bf.a) { if ((rc = gemm_dw(w.dproj, w.P, w.xn, D, w.dwcat, D, w.P, D, R, w.part, s))) return rc; }
    else {          // q | k | v rows on the bf16 pipe, the gate / mix rows in fp32
        if ((rc = gemm_dw(w.dproj, w.P, w.xn, D, w.dwcat, D, 3 * hd, D, R, w.part, s))) return rc;
        if ((rc = gemm_dw_f32(w.dproj + 3 * hd, w.P, w.xn, D, w.dwcat + (size_t)3 * hd * D, D, w.P - 3 * hd, D, R, w.part, s))) return rc;
    }
    {
        const int64_t blk = (int64_t)hd * D;
        MultiCopy mc;
        mc.add(o.d_wq, w.dwcat, blk); mc.add(o.d_wk, w.dwcat + blk, blk); mc.add(o.d_wv, w.dwcat + 2 * blk, blk);
        mc.add(o.d_wg, w.dwcat + 3 * blk, (int64_t)heads * D);
        if (has_rv) mc.add(o.d_wm, w.dwcat + (size_t)(3 * hd + w.hp4) * D, (int64_t)heads * D);
        if ((rc = multi_copy(mc, s))) return rc;
    }
    if (!t_bf.a) { if ((rc = lin_dx(w.dproj, w.P, w.wcat, D, w.dxn, D, R, D, w.P, w.wt, s))) return rc; }
    else {          // the fp32 gate / mix part first, then the q | k | v part added on the bf16 pipe
        if ((rc = gemm_dx(w.dproj + 3 * hd, w.P, w.wcat + (size_t)3 * hd * D, D, w.dxn, D, R, D, w.P - 3 * hd, w.wt, s))) return rc;
        if ((rc = lin_dx(w.dproj, w.P, w.wcat, D, w.dxn, D, R, D, 3 * hd, w.wt, s, true))) return rc;
    }
    if ((rc = rmsnorm_bwd(x, w.dxn, prm.norm_w, w.tg, o.dx, R, D, RMS_EPS, s))) return rc;
    ColsumBatch cb;                                    // key gain, mix bias, norm gain: one launch
    cb.add(w.gpart, hd, g.groups, hd, o.d_gamma);
    if (has_rv) cb.add(w.dproj + 3 * hd + w.hp4, w.P, R, heads, o.d_bm);
    cb.add(w.tg, D, R, D, o.d_norm_w);
    return colsum_batch(cb, s);
}

struct XWs {
    float *qn, *cn, *wqg, *wkv, *projq, *projk, *dprojq, *dprojk, *d_o3, *o3, *dwqg, *dwkv, *tg, *dqn, *tgc, *dcn, *gpart, *part, *wt;
    float* tiled;                    // planes of the tiled core, last, so that every other offset is the same with and without them
    size_t total; int Pq, Pk, hp4;
};
XWs x_ws(float* base, int Rq, int Rk, int G, int D, int Dc, int heads, int dh, bool tiled = false) {
    XWs w{};
    const int hd = heads * dh;
    w.hp4 = (heads + 3) / 4 * 4; w.Pq = hd + w.hp4; w.Pk = 2 * hd;
    size_t off = 0;
    auto take = [&](size_t n) { float* p = base ? base + off : nullptr; off += (n + 63) / 64 * 64; return p; };
    w.qn = take((size_t)Rq * D); w.cn = take((size_t)Rk * Dc); w.wqg = take((size_t)w.Pq * D); w.wkv = take((size_t)w.Pk * Dc);
    w.projq = take((size_t)Rq * w.Pq); w.projk = take((size_t)Rk * w.Pk); w.dprojq = take((size_t)Rq * w.Pq); w.dprojk = take((size_t)Rk * w.Pk);
    w.d_o3 = take((size_t)Rq * hd); w.o3 = take((size_t)Rq * hd); w.dwqg = take((size_t)w.Pq * D); w.dwkv = take((size_t)w.Pk * Dc);
    w.tg = take((size_t)Rq * D); w.dqn = take((size_t)Rq * D); w.tgc = take((size_t)Rk * Dc); w.dcn = take((size_t)Rk * Dc); w.gpart = take((size_t)G * hd);
    w.part = take(DW_PART_FLOATS);
    w.wt = take((size_t)(w.Pk > w.Pq ? w.Pk : w.Pq) * (D > Dc ? D : Dc));
    if (tiled) w.tiled = take(attn_bf16() && G > 0 ? attn_tiled_bf16_cross_floats(G, Rq / G, Rk / G, heads, dh) : attn_tiled_cross_floats(Rq, Rk, heads, dh));
    w.total = off;
    return w;
}

struct XParams { const float *norm_w, *norm_ctx_w, *wq, *wk, *wv, *wo, *wg, *gamma; };

int x_project(const XWs& w, const float* q_tokens, const float* ctx, const XParams& prm, int Rq, int Rk, int D, int Dc, int heads, int dh, hipStream_t s) {
    const int hd = heads * dh;
    int rc;
    {
        MultiCopy mc;
        mc.add(w.wqg, prm.wq, (int64_t)hd * D); mc.add(w.wqg + (size_t)hd * D, prm.wg, (int64_t)heads * D);
        mc.add(w.wqg + (size_t)(hd + heads) * D, nullptr, (int64_t)(w.Pq - hd - heads) * D);
        mc.add(w.wkv, prm.wk, (int64_t)hd * Dc); mc.add(w.wkv + (size_t)hd * Dc, prm.wv, (int64_t)hd * Dc);
        if ((rc = multi_copy(mc, s))) return rc;
    }
    if ((rc = rmsnorm_rows(q_tokens, D, prm.norm_w, w.qn, D, Rq, D, RMS_EPS, s))) return rc;
    if (prm.norm_ctx_w) { if ((rc = rmsnorm_rows(ctx, Dc, prm.norm_ctx_w, w.cn, Dc, Rk, Dc, RMS_EPS, s))) return rc; }
    else if ((rc = copy_rows(ctx, Dc, w.cn, Dc, Rk, Dc, s))) return rc;
    if (!t_bf.a) { if ((rc = gemm_b(w.qn, D, w.wqg, D, w.projq, w.Pq, nullptr, Rq, w.Pq, D, 0, s))) return rc; }
    else {          // bf16 training arithmetic: the queries on the bf16 pipe, the heads-wide gate logits an fp32 product
        if ((rc = gemm_b(w.qn, D, w.wqg, D, w.projq, w.Pq, nullptr, Rq, hd, D, 0, s))) return rc;
        if ((rc = gemm_f32(w.qn, D, w.wqg + (size_t)hd * D, D, w.projq + hd, w.Pq, nullptr, Rq, w.Pq - hd, D, 0, s))) return rc;
    }
    return gemm_b(w.cn, Dc, w.wkv, Dc, w.projk, w.Pk, nullptr, Rk, w.Pk, Dc, 0, s);
}

size_t x_bf16_extra(int Rq, int Rk, int D, int Dc, int hd) {
    const int dm = D > Dc ? D : Dc;
    return bf16_extra_bytes(Rq > Rk ? Rq : Rk, 2 * hd > dm ? 2 * hd : dm, 2 * hd > dm ? 2 * hd : dm, 2 * hd > dm ? 2 * hd : dm);
}

int x_check(int G, int nq, int nk, int D, int Dc, int heads, int dh, const float* workspace, size_t workspace_bytes) {
    const int cap = g_train_wide.load() ? ATT_MAX_FRAMES : XA_N;
    D4_REQUIRE(nq >= 1 && nq <= cap && nk >= 1 && nk <= cap, "cross attention block: %d queries / %d keys per group (max %d)", nq, nk, cap);
    D4_REQUIRE(dh == 16 || dh == 32 || dh == 64, "cross attention block: head dim %d (16, 32 or 64)", dh);
    D4_REQUIRE(D % 4 == 0 && Dc % 4 == 0 && ((uintptr_t)workspace % 256) == 0, "cross attention block: dims must be multiples of 4 and the workspace 256-byte aligned");
    D4_REQUIRE(workspace_bytes >= x_ws(nullptr, G * nq, G * nk, G, D, Dc, heads, dh, cross_tiled(nq, nk)).total * sizeof(float), "cross attention block: workspace too small");
    return 0;
}

}  // namespace

extern "C" {

size_t d4_cross_attn_workspace_bytes(int groups, int nq, int nk, int dim, int dim_ctx, int heads, int dim_head) {
    return x_ws(nullptr, groups * nq, groups * nk, groups, dim, dim_ctx, heads, dim_head, cross_tiled(nq, nk)).total * sizeof(float);
}
size_t d4_cross_attn_bf16_scratch_bytes(int groups, int nq, int nk, int dim, int dim_ctx, int heads, int dim_head) {
    return x_bf16_extra(groups * nq, groups * nk, dim, dim_ctx, heads * dim_head);
}

int d4_cross_attn_forward(const float* q_tokens, const float* ctx, const float* norm_w, const float* norm_ctx_w, const float* wq, const float* wk,
                          const float* wv, const float* wo, const float* w_gates, const float* k_gamma, int groups, int nq, int nk, int ctx_item_major,
                          int dim, int dim_ctx, int heads, int dim_head, float softclamp, float* y, float* workspace, size_t workspace_bytes, void* stream) {
    D4_REQUIRE(q_tokens && ctx && norm_w && wq && wk && wv && wo && w_gates && k_gamma && y && workspace, "d4_cross_attn_forward: null argument");
    int rc;
    if ((rc = x_check(groups, nq, nk, dim, dim_ctx, heads, dim_head, workspace, workspace_bytes))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Rq = groups * nq, Rk = groups * nk, hd = heads * dim_head;
    if (Rq == 0) return 0;
    const XWs w = x_ws(workspace, Rq, Rk, groups, dim, dim_ctx, heads, dim_head, cross_tiled(nq, nk));
    const XParams prm{norm_w, norm_ctx_w, wq, wk, wv, wo, w_gates, k_gamma};
    Bf16Scope bf;
    {
        const int dm = dim > dim_ctx ? dim : dim_ctx, wd = 2 * hd > dm ? 2 * hd : dm;
        if ((rc = bf.enter("d4_cross_attn_forward", Rq > Rk ? Rq : Rk, wd, wd, wd))) return rc;
    }
    if ((rc = x_project(w, q_tokens, ctx, prm, Rq, Rk, dim, dim_ctx, heads, dim_head, s))) return rc;
    XAttnArgs a{w.projq, w.Pq, w.projk, w.Pk, k_gamma, nullptr, w.o3, nullptr, nullptr, nullptr, groups, nq, nk, heads, ctx_item_major, softclamp};
    if ((rc = xattn_core(a, dim_head, s, w.tiled))) return rc;
    return gemm_b(w.o3, hd, wo, hd, y, dim, nullptr, Rq, dim, hd, 0, s);
}

static int cross_attn_backward_impl(const float* q_tokens, const float* ctx, const float* dy, const float* norm_w, const float* norm_ctx_w, const float* wq,
                           const float* wk, const float* wv, const float* wo, const float* w_gates, const float* k_gamma, int groups, int nq, int nk,
                           int ctx_item_major, int dim, int dim_ctx, int heads, int dim_head, float softclamp,
                           float* d_q_tokens, float* d_ctx, float* d_norm_w, float* d_norm_ctx_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                           float* d_w_gates, float* d_k_gamma, float* workspace, size_t workspace_bytes, void* stream, bool reuse) {
    D4_REQUIRE(q_tokens && ctx && dy && norm_w && wq && wk && wv && wo && w_gates && k_gamma && workspace, "d4_cross_attn_backward: null argument");
    D4_REQUIRE(d_q_tokens && d_ctx && d_norm_w && d_wq && d_wk && d_wv && d_wo && d_w_gates && d_k_gamma && (!norm_ctx_w || d_norm_ctx_w),
               "d4_cross_attn_backward: null gradient output");
    int rc;
    if ((rc = x_check(groups, nq, nk, dim, dim_ctx, heads, dim_head, workspace, workspace_bytes))) return rc;
    D4_REQUIRE(groups >= 1, "d4_cross_attn_backward: no groups");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Rq = groups * nq, Rk = groups * nk, D = dim, Dc = dim_ctx, hd = heads * dim_head;
    const XWs w = x_ws(workspace, Rq, Rk, groups, D, Dc, heads, dim_head, cross_tiled(nq, nk));
    const XParams prm{norm_w, norm_ctx_w, wq, wk, wv, wo, w_gates, k_gamma};
    Bf16Scope bf;
    {
        const int dm = D > Dc ? D : Dc, wd = 2 * hd > dm ? 2 * hd : dm;
        if ((rc = bf.enter("d4_cross_attn_backward", Rq > Rk ? Rq : Rk, wd, wd, wd))) return rc;
    }
    if (!reuse && (rc = x_project(w, q_tokens, ctx, prm, Rq, Rk, D, Dc, heads, dim_head, s))) return rc;
    if ((rc = lin_dx(dy, D, wo, hd, w.d_o3, hd, Rq, hd, D, w.wt, s))) return rc;
    XAttnArgs a{w.projq, w.Pq, w.projk, w.Pk, k_gamma, w.d_o3, w.o3, w.dprojq, w.dprojk, w.gpart, groups, nq, nk, heads, ctx_item_major, softclamp};
    if ((rc = xattn_core(a, dim_head, s, w.tiled))) return rc;
    image_a_written(w.dprojq); image_a_written(w.dprojk);
    if (w.hp4 > heads && (rc = zero_pad_cols(w.dprojq, Rq, w.Pq, hd + heads, w.Pq, s))) return rc;
    if ((rc = gemm_dw(dy, D, w.o3, hd, d_wo, hd, D, hd, Rq, w.part, s))) return rc;
    // query side
    if (!t_bf.a) {
        if ((rc = gemm_dw(w.dprojq, w.Pq, w.qn, D, w.dwqg, D, w.Pq, D, Rq, w.part, s))) return rc;
        if ((rc = lin_dx(w.dprojq, w.Pq, w.wqg, D, w.dqn, D, Rq, D, w.Pq, w.wt, s))) return rc;
    } else {        // query rows on the bf16 pipe, gate rows in fp32 (as in x_project)
        if ((rc = gemm_dw(w.dprojq, w.Pq, w.qn, D, w.dwqg, D, hd, D, Rq, w.part, s))) return rc;
        if ((rc = gemm_dw_f32(w.dprojq + hd, w.Pq, w.qn, D, w.dwqg + (size_t)hd * D, D, w.Pq - hd, D, Rq, w.part, s))) return rc;
        if ((rc = gemm_dx(w.dprojq + hd, w.Pq, w.wqg + (size_t)hd * D, D, w.dqn, D, Rq, D, w.Pq - hd, w.wt, s))) return rc;
        if ((rc = lin_dx(w.dprojq, w.Pq, w.wqg, D, w.dqn, D, Rq, D, hd, w.wt, s, true))) return rc;
    }
    if ((rc = rmsnorm_bwd(q_tokens, w.dqn, norm_w, w.tg, d_q_tokens, Rq, D, RMS_EPS, s))) return rc;
    {
        ColsumBatch cb;                                // key gain and the query norm's gain: one launch
        cb.add(w.gpart, hd, groups, hd, d_k_gamma); cb.add(w.tg, D, Rq, D, d_norm_w);
        if ((rc = colsum_batch(cb, s))) return rc;
    }
    // context side
    if ((rc = gemm_dw(w.dprojk, w.Pk, w.cn, Dc, w.dwkv, Dc, w.Pk, Dc, Rk, w.part, s))) return rc;
    {   // the pieces of both concatenated weight gradients in one launch
        MultiCopy mc;
        mc.add(d_wq, w.dwqg, (int64_t)hd * D); mc.add(d_w_gates, w.dwqg + (size_t)hd * D, (int64_t)heads * D);
        mc.add(d_wk, w.dwkv, (int64_t)hd * Dc); mc.add(d_wv, w.dwkv + (size_t)hd * Dc, (int64_t)hd * Dc);
        if ((rc = multi_copy(mc, s))) return rc;
    }
    if (norm_ctx_w) {
        if ((rc = lin_dx(w.dprojk, w.Pk, w.wkv, Dc, w.dcn, Dc, Rk, Dc, w.Pk, w.wt, s))) return rc;
        if ((rc = rmsnorm_bwd(ctx, w.dcn, norm_ctx_w, w.tgc, d_ctx, Rk, Dc, RMS_EPS, s))) return rc;
        return colsum(w.tgc, Dc, Rk, Dc, d_norm_ctx_w, s, w.part, DW_PART_FLOATS);
    }
    return lin_dx(w.dprojk, w.Pk, w.wkv, Dc, d_ctx, Dc, Rk, Dc, w.Pk, w.wt, s);
}

#define D4_XBWD_PARAMS const float* q_tokens, const float* ctx, const float* dy, const float* norm_w, const float* norm_ctx_w, const float* wq,          \
                       const float* wk, const float* wv, const float* wo, const float* w_gates, const float* k_gamma, int groups, int nq, int nk,        \
                       int ctx_item_major, int dim, int dim_ctx, int heads, int dim_head, float softclamp, float* d_q_tokens, float* d_ctx,             \
                       float* d_norm_w, float* d_norm_ctx_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo, float* d_w_gates, float* d_k_gamma,    \
                       float* workspace, size_t workspace_bytes, void* stream
#define D4_XBWD_ARGS q_tokens, ctx, dy, norm_w, norm_ctx_w, wq, wk, wv, wo, w_gates, k_gamma, groups, nq, nk, ctx_item_major, dim, dim_ctx, heads, dim_head, \
                     softclamp, d_q_tokens, d_ctx, d_norm_w, d_norm_ctx_w, d_wq, d_wk, d_wv, d_wo, d_w_gates, d_k_gamma, workspace, workspace_bytes, stream
int d4_cross_attn_backward(D4_XBWD_PARAMS) { return cross_attn_backward_impl(D4_XBWD_ARGS, false); }
int d4_cross_attn_backward_saved(D4_XBWD_PARAMS) { return cross_attn_backward_impl(D4_XBWD_ARGS, true); }

size_t d4_time_attn_workspace_bytes(int batch, int frames, int tokens, int dim, int heads, int dim_head) {
    const bool tiled = frames > AB_S || g_time_attn_tiled != 0;       // the rule of attn_tiled(): at <= 64 frames the size is the LDS core's
    return attn_ws(nullptr, batch * frames * tokens, batch * tokens, dim, heads, dim_head, tiled).total * sizeof(float);
}

int d4_space_attn_forward(const float* x, const float* residual_values, const float* norm_w, const float* wq, const float* wk, const float* wv,
                          const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma,
                          int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int num_special, int belief,
                          float* y, float* workspace, size_t workspace_bytes, void* stream) {
    const AttnParams prm{norm_w, wq, wk, wv, wo, w_gates, w_mix, b_mix, k_gamma};
    const AttnGeom g{frames, tokens, 1, tokens, 1, 0, num_special, nullptr};
    return attn_block_forward(x, residual_values, prm, frames * tokens, g, dim, heads, dim_head, softclamp, belief, y, workspace, workspace_bytes,
                              static_cast<hipStream_t>(stream));
}

int d4_space_attn_backward(const float* x, const float* residual_values, const float* dy, const float* norm_w, const float* wq, const float* wk,
                           const float* wv, const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma,
                           int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int num_special, int belief,
                           float* dx, float* d_residual_values, float* d_norm_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                           float* d_w_gates, float* d_w_mix, float* d_b_mix, float* d_k_gamma,
                           float* workspace, size_t workspace_bytes, void* stream) {
    const AttnParams prm{norm_w, wq, wk, wv, wo, w_gates, w_mix, b_mix, k_gamma};
    const AttnGeom g{frames, tokens, 1, tokens, 1, 0, num_special, nullptr};
    const AttnGrads o{dx, d_residual_values, d_norm_w, d_wq, d_wk, d_wv, d_wo, d_w_gates, d_w_mix, d_b_mix, d_k_gamma};
    return attn_block_backward(x, residual_values, dy, prm, frames * tokens, g, dim, heads, dim_head, softclamp, belief, o, workspace, workspace_bytes,
                               static_cast<hipStream_t>(stream));
}

int d4_space_attn_backward_saved(const float* x, const float* residual_values, const float* dy, const float* norm_w, const float* wq, const float* wk,
                           const float* wv, const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma,
                           int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int num_special, int belief,
                           float* dx, float* d_residual_values, float* d_norm_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                           float* d_w_gates, float* d_w_mix, float* d_b_mix, float* d_k_gamma,
                           float* workspace, size_t workspace_bytes, void* stream) {
    const AttnParams prm{norm_w, wq, wk, wv, wo, w_gates, w_mix, b_mix, k_gamma};
    const AttnGeom g{frames, tokens, 1, tokens, 1, 0, num_special, nullptr};
    const AttnGrads o{dx, d_residual_values, d_norm_w, d_wq, d_wk, d_wv, d_wo, d_w_gates, d_w_mix, d_b_mix, d_k_gamma};
    return attn_block_backward(x, residual_values, dy, prm, frames * tokens, g, dim, heads, dim_head, softclamp, belief, o, workspace, workspace_bytes,
                               static_cast<hipStream_t>(stream), true);
}

int d4_time_attn_forward(const float* x, const float* residual_values, const float* norm_w, const float* wq, const float* wk, const float* wv,
                         const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma, const float* inv_freq,
                         int batch, int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int belief,
                         float* y, float* workspace, size_t workspace_bytes, void* stream) {
    D4_REQUIRE(inv_freq, "d4_time_attn_forward: null rotary frequencies");
    const AttnParams prm{norm_w, wq, wk, wv, wo, w_gates, w_mix, b_mix, k_gamma};
    const AttnGeom g{batch * tokens, frames, tokens, (int64_t)frames * tokens, tokens, 1, 0, inv_freq};
    return attn_block_forward(x, residual_values, prm, batch * frames * tokens, g, dim, heads, dim_head, softclamp, belief, y, workspace, workspace_bytes,
                              static_cast<hipStream_t>(stream));
}

int d4_time_attn_backward(const float* x, const float* residual_values, const float* dy, const float* norm_w, const float* wq, const float* wk,
                          const float* wv, const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma,
                          const float* inv_freq, int batch, int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int belief,
                          float* dx, float* d_residual_values, float* d_norm_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                          float* d_w_gates, float* d_w_mix, float* d_b_mix, float* d_k_gamma,
                          float* workspace, size_t workspace_bytes, void* stream) {
    D4_REQUIRE(inv_freq, "d4_time_attn_backward: null rotary frequencies");
    const AttnParams prm{norm_w, wq, wk, wv, wo, w_gates, w_mix, b_mix, k_gamma};
    const AttnGeom g{batch * tokens, frames, tokens, (int64_t)frames * tokens, tokens, 1, 0, inv_freq};
    const AttnGrads o{dx, d_residual_values, d_norm_w, d_wq, d_wk, d_wv, d_wo, d_w_gates, d_w_mix, d_b_mix, d_k_gamma};
    return attn_block_backward(x, residual_values, dy, prm, batch * frames * tokens, g, dim, heads, dim_head, softclamp, belief, o, workspace,
                               workspace_bytes, static_cast<hipStream_t>(stream));
}

int d4_time_attn_backward_saved(const float* x, const float* residual_values, const float* dy, const float* norm_w, const float* wq, const float* wk,
                          const float* wv, const float* wo, const float* w_gates, const float* w_mix, const float* b_mix, const float* k_gamma,
                          const float* inv_freq, int batch, int frames, int tokens, int dim, int heads, int dim_head, float softclamp, int belief,
                          float* dx, float* d_residual_values, float* d_norm_w, float* d_wq, float* d_wk, float* d_wv, float* d_wo,
                          float* d_w_gates, float* d_w_mix, float* d_b_mix, float* d_k_gamma,
                          float* workspace, size_t workspace_bytes, void* stream) {
    D4_REQUIRE(inv_freq, "d4_time_attn_backward: null rotary frequencies");
    const AttnParams prm{norm_w, wq, wk, wv, wo, w_gates, w_mix, b_mix, k_gamma};
    const AttnGeom g{batch * tokens, frames, tokens, (int64_t)frames * tokens, tokens, 1, 0, inv_freq};
    const AttnGrads o{dx, d_residual_values, d_norm_w, d_wq, d_wk, d_wv, d_wo, d_w_gates, d_w_mix, d_b_mix, d_k_gamma};
    return attn_block_backward(x, residual_values, dy, prm, batch * frames * tokens, g, dim, heads, dim_head, softclamp, belief, o, workspace,
                               workspace_bytes, static_cast<hipStream_t>(stream), true);
}

// ---- operator-level entries of the attention cores (tests/test_gpu_train_cores.py): the argument block filled from the arguments and the core the
// blocks call; core 0: the whole-problem-in-LDS kernel, core 1: the tiled core on the caller's planes.  No arithmetic of their own.
size_t d4_train_attn_core_plane_floats(int rows, int heads, int dim_head) {
    return rows > 0 && heads > 0 && dim_head > 0 ? attn_tiled_floats(rows, heads, dim_head) : 0;
}
size_t d4_train_xattn_core_plane_floats(int q_rows, int k_rows, int heads, int dim_head) {
    return q_rows > 0 && k_rows > 0 && heads > 0 && dim_head > 0 ? attn_tiled_cross_floats(q_rows, k_rows, heads, dim_head) : 0;
}
// (the bf16-product form of the tiled core: its images are padded per problem, so the size depends on the items and not on the rows alone)
size_t d4_train_attn_core_bf16_plane_floats(int groups, int items, int heads, int dim_head) {
    return groups > 0 && items > 0 && heads > 0 && dim_head > 0 ? attn_tiled_bf16_floats(groups, items, heads, dim_head) : 0;
}
size_t d4_train_xattn_core_bf16_plane_floats(int groups, int nq, int nk, int heads, int dim_head) {
    return groups > 0 && nq > 0 && nk > 0 && heads > 0 && dim_head > 0 ? attn_tiled_bf16_cross_floats(groups, nq, nk, heads, dim_head) : 0;
}

}  // extern "C"

// `who`: the entry's name in its refusals; bf16: the entry of the tiled core's bf16-product form (core 1 only)
static int train_attn_core_entry(const char* who, bool bf16, const float* proj, int ldp, const float* rv, const float* gamma, const float* d_o3,
                                 float* o3, float* dproj, float* d_rv, float* dgamma_part,
                                 int groups, int items, int heads, int dim_head, float softclamp, int num_special, int belief,
                                 int g_inner, int64_t g_outer_stride, int64_t item_stride, int causal, const float* inv_freq,
                                 int core, float* planes, size_t plane_floats, void* stream) {
    D4_REQUIRE(proj && gamma && o3, "%s: null proj, gamma or o3", who);
    D4_REQUIRE(!d_o3 || (dproj && dgamma_part), "%s: d_o3 given with null dproj or dgamma_part", who);
    D4_REQUIRE(!d_o3 || !rv || d_rv, "%s: d_o3 and rv given with null d_rv", who);
    D4_REQUIRE(dim_head == 16 || dim_head == 32 || dim_head == 64, "%s: dim_head %d (16, 32 or 64)", who, dim_head);
    D4_REQUIRE(groups >= 1 && heads >= 1, "%s: groups %d, heads %d (at least 1)", who, groups, heads);
    D4_REQUIRE(items >= 1, "%s: items %d (at least 1)", who, items);
    D4_REQUIRE(!bf16 || core != 0, "%s: core 0 (the whole-problem-in-LDS kernels have no bf16 form; 1: tiled)", who);
    D4_REQUIRE(bf16 ? core == 1 : (core == 0 || core == 1), bf16 ? "%s: core %d (1: tiled)" : "%s: core %d (0: LDS kernel, 1: tiled)", who, core);
    D4_REQUIRE(core != 0 || items <= AB_S, "%s: items %d with core 0 (max %d)", who, items, AB_S);
    D4_REQUIRE(core != 1 || items <= ATT_MAX_FRAMES, "%s: items %d with core 1 (max %d)", who, items, ATT_MAX_FRAMES);
    const int hd = heads * dim_head, hp4 = (heads + 3) / 4 * 4;
    D4_REQUIRE(ldp >= 3 * hd + hp4 + heads, "%s: ldp %d below 3 * heads * dim_head + hp4 + heads = %d", who, ldp, 3 * hd + hp4 + heads);
    D4_REQUIRE((causal != 0) == (inv_freq != nullptr), "%s: causal and inv_freq go together (the time geometry) or are both absent", who);
    D4_REQUIRE(num_special >= 0 && num_special <= items, "%s: num_special %d outside 0..items (%d)", who, num_special, items);
    D4_REQUIRE(num_special == 0 || !causal, "%s: num_special %d with causal", who, num_special);
    D4_REQUIRE(g_inner >= 1 && g_outer_stride >= 0 && item_stride >= 1, "%s: g_inner %d, g_outer_stride %lld, item_stride %lld",
               who, g_inner, (long long)g_outer_stride, (long long)item_stride);
    if (core == 1) {
        D4_REQUIRE(planes && ((uintptr_t)planes % 16) == 0, "%s: core 1 needs planes (16-byte aligned)", who);
        const size_t need = bf16 ? attn_tiled_bf16_floats(groups, items, heads, dim_head) : attn_tiled_floats(groups * items, heads, dim_head);
        D4_REQUIRE(plane_floats >= need, "%s: plane_floats %zu below %s_plane_floats = %zu", who, plane_floats, who, need);
    }
    AttnBwdArgs a{proj, ldp, rv, gamma, d_o3, o3, dproj, d_rv, dgamma_part, groups, items, heads, hp4, softclamp, num_special, belief ? 1 : 0};
    a.g_inner = g_inner; a.g_outer_stride = g_outer_stride; a.item_stride = item_stride; a.causal = causal ? 1 : 0; a.inv_freq = inv_freq;
    // the form is the entry's, whatever d4_train_attn_products_set says: `planes` was sized and checked for it
    if (bf16) return attn_tiled_bf16_core(a, dim_head, planes, static_cast<hipStream_t>(stream));
    if (core == 1) return attn_tiled_core(a, dim_head, planes, static_cast<hipStream_t>(stream));
    return attn_core(a, dim_head, static_cast<hipStream_t>(stream));
}

static int train_xattn_core_entry(const char* who, bool bf16, const float* projq, int ldq, const float* projk, int ldk, const float* gamma, const float* d_o3,
                                  float* o3, float* dprojq, float* dprojk, float* dgamma_part,
                                  int groups, int nq, int nk, int heads, int dim_head, int item_major, float softclamp,
                                  int core, float* planes, size_t plane_floats, void* stream) {
    D4_REQUIRE(projq && projk && gamma && o3, "%s: null projq, projk, gamma or o3", who);
    D4_REQUIRE(!d_o3 || (dprojq && dprojk && dgamma_part), "%s: d_o3 given with null dprojq, dprojk or dgamma_part", who);
    D4_REQUIRE(dim_head == 16 || dim_head == 32 || dim_head == 64, "%s: dim_head %d (16, 32 or 64)", who, dim_head);
    D4_REQUIRE(groups >= 1 && heads >= 1, "%s: groups %d, heads %d (at least 1)", who, groups, heads);
    D4_REQUIRE(nq >= 1, "%s: nq %d (at least 1)", who, nq);
    D4_REQUIRE(nk >= 1, "%s: nk %d (at least 1)", who, nk);
    D4_REQUIRE(!bf16 || core != 0, "%s: core 0 (the whole-problem-in-LDS kernels have no bf16 form; 1: tiled)", who);
    D4_REQUIRE(bf16 ? core == 1 : (core == 0 || core == 1), bf16 ? "%s: core %d (1: tiled)" : "%s: core %d (0: LDS kernel, 1: tiled)", who, core);
    D4_REQUIRE(core != 0 || (nq <= XA_N && nk <= XA_N), "%s: nq %d / nk %d with core 0 (max %d)", who, nq, nk, XA_N);
    D4_REQUIRE(core != 1 || (nq <= ATT_MAX_FRAMES && nk <= ATT_MAX_FRAMES), "%s: nq %d / nk %d with core 1 (max %d)", who, nq, nk, ATT_MAX_FRAMES);
    const int hd = heads * dim_head;
    D4_REQUIRE(ldq >= hd + heads, "%s: ldq %d below heads * dim_head + heads = %d", who, ldq, hd + heads);
    D4_REQUIRE(ldk >= 2 * hd, "%s: ldk %d below 2 * heads * dim_head = %d", who, ldk, 2 * hd);
    if (core == 1) {
        D4_REQUIRE(planes && ((uintptr_t)planes % 16) == 0, "%s: core 1 needs planes (16-byte aligned)", who);
        const size_t need = bf16 ? attn_tiled_bf16_cross_floats(groups, nq, nk, heads, dim_head) : attn_tiled_cross_floats(groups * nq, groups * nk, heads, dim_head);
        D4_REQUIRE(plane_floats >= need, "%s: plane_floats %zu below %s_plane_floats = %zu", who, plane_floats, who, need);
    }
    XAttnArgs a{projq, ldq, projk, ldk, gamma, d_o3, o3, dprojq, dprojk, dgamma_part, groups, nq, nk, heads, item_major ? 1 : 0, softclamp};
    if (bf16) return attn_tiled_bf16_cross_core(a, dim_head, planes, static_cast<hipStream_t>(stream));
    if (core == 1) return attn_tiled_cross_core(a, dim_head, planes, static_cast<hipStream_t>(stream));
    return xattn_core(a, dim_head, static_cast<hipStream_t>(stream));
}

#define D4_CORE_PARAMS const float* proj, int ldp, const float* rv, const float* gamma, const float* d_o3, float* o3, float* dproj, float* d_rv,           \
                       float* dgamma_part, int groups, int items, int heads, int dim_head, float softclamp, int num_special, int belief, int g_inner,     \
                       int64_t g_outer_stride, int64_t item_stride, int causal, const float* inv_freq, int core, float* planes, size_t plane_floats,      \
                       void* stream
#define D4_CORE_ARGS proj, ldp, rv, gamma, d_o3, o3, dproj, d_rv, dgamma_part, groups, items, heads, dim_head, softclamp, num_special, belief, g_inner, \
                     g_outer_stride, item_stride, causal, inv_freq, core, planes, plane_floats, stream
#define D4_XCORE_PARAMS const float* projq, int ldq, const float* projk, int ldk, const float* gamma, const float* d_o3, float* o3, float* dprojq,         \
                        float* dprojk, float* dgamma_part, int groups, int nq, int nk, int heads, int dim_head, int item_major, float softclamp,          \
                        int core, float* planes, size_t plane_floats, void* stream
#define D4_XCORE_ARGS projq, ldq, projk, ldk, gamma, d_o3, o3, dprojq, dprojk, dgamma_part, groups, nq, nk, heads, dim_head, item_major, softclamp, core, \
                      planes, plane_floats, stream

extern "C" {

int d4_train_attn_core(D4_CORE_PARAMS) { return train_attn_core_entry("d4_train_attn_core", false, D4_CORE_ARGS); }
int d4_train_attn_core_bf16(D4_CORE_PARAMS) { return train_attn_core_entry("d4_train_attn_core_bf16", true, D4_CORE_ARGS); }
int d4_train_xattn_core(D4_XCORE_PARAMS) { return train_xattn_core_entry("d4_train_xattn_core", false, D4_XCORE_ARGS); }
int d4_train_xattn_core_bf16(D4_XCORE_PARAMS) { return train_xattn_core_entry("d4_train_xattn_core_bf16", true, D4_XCORE_ARGS); }

}  // extern "C"
