// fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact f32, 64 FLOP/clk/SIMD).
//
//   C[m, n] = epilogue( rowscale[m] * sum_k A[m, k] * W[n, k] )            ("NT": both K-contiguous)
//
// This one kernel family carries every dense projection of the imagination path
// (reference: Attention.to_q/k/v/out D4:1985-2068, FeedForward.proj_in/out D4:2105-2116,
// AttentionPool / LQAP projections D4:2143-2210, head MLPs D4:4950, 5095).  The reference runs
// RMSNorm -> Linear -> activation -> residual as separate ATen ops; here
//   * RMSNorm is folded: gamma is pre-multiplied into W (engine prepare), and the per-row
//     1/rms is accumulated from the A tiles as they stream through LDS and applied in the epilogue,
//   * bias, SiLU, SiLU-GLU pairing and the residual add run in the epilogue.
//
// Tiling: BM x BN block tile, BK = 32 or 16, WGM x WGN waves (4, 8 or 16), each wave owns
// TM x TN MFMA 32x32 sub-tiles.  LDS tiles are row-major [rows][BK + 4] (the +4 keeps 16-byte
// alignment and spreads ds_read_b128 over the 64 banks), double-buffered, one barrier per k-tile.
// Staging is global -> registers -> LDS with a 2-deep register prefetch: k-tile j+2 is in flight
// while k-tile j+1 (loaded an iteration earlier) is written to the other LDS buffer between the
// MFMA groups of k-tile j.  Eight tile configurations exist (enum TileCfg); the first launch of a
// shape times the valid ones and the choice is cached (all of them produce identical bits).
// The MFMA consumes k in the order lanes<32: {8q+e}, lanes>=32: {8q+4+e} so that each lane's
// operand for four consecutive k-steps is one ds_read_b128 (summation order inside a k-tile is a
// fixed permutation; results are deterministic).
//
// Below the kernel sits the dispatcher every dense product passes through: ONE route function (which family runs a call: route), ONE table of the
// families that are tuned (kFamilies) with ONE tuner and ONE tuned launch over it, and ONE timed launch for the profile classes (timed_launch).
#include "common.h"
#include <string.h>
#include <hip/hip_ext.h>
#include "kernels.h"
#include "../../include/d4hip.h"     // the D4_GEMM_* family codes
#include <mutex>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <tuple>
#include <type_traits>
#include <vector>

namespace d4 {


template <int BM, int BN, int WGM, int WGN, int BK, int KS, bool TA, bool TB, bool KTAIL>
__global__ __launch_bounds__(WGM * WGN * 64 * KS) void gemm_kernel(GemmArgs p) {
    constexpr int LDS_LD = BK + 4;
    constexpr int RF4 = BK / 4;                 // float4 per tile row
    constexpr int NT = WGM * WGN * 64 * KS;     // threads per block (KS > 1: intra-block split of each k-tile across wave groups)
    constexpr int TM = BM / WGM / 32;
    constexpr int TN = BN / WGN / 32;
    static_assert(TM >= 1 && TN >= 1, "tile");
    constexpr int A_F4 = BM * BK / 4 / NT;    // float4 per thread per A tile
    constexpr int B_F4 = BN * BK / 4 / NT;
    static_assert(A_F4 >= 1 && B_F4 >= 1, "tile too small for the thread count");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                                 // [2][BM][LDS_LD]
    float* Bs = smem + 2 * BM * LDS_LD;               // [2][BN][LDS_LD]
    float* rowscale_s = Bs + 2 * BN * LDS_LD;         // [BM]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = (tid >> 6) % (WGM * WGN);
    const int ks = (tid >> 6) / (WGM * WGN);    // which share of the k-steps of every tile this wave group takes
    const int wm = wave / WGN, wn = wave % WGN;

    // XCD-aware block order: consecutive blocks on one XCD share the same A row-panel.
    int bid = blockIdx.x;
    const int nbn = (p.N + BN - 1) / BN;
    const int nbm = (p.M + BM - 1) / BM;
    const int nblk = nbm * nbn;
    {
        const int nx = 8;
        int q = nblk / nx, r = nblk % nx, x = bid % nx, o = bid / nx;
        bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + o;
    }
    const int bm0 = (bid / nbn) * BM;
    const int bn0 = (bid % nbn) * BN;

    // Operands are read through buffer descriptors (wave-uniform, built from kernel arguments and the block
    // index only): out-of-range rows fall outside num_records and return 0 in hardware, so the staging loads are
    // branch-free; logically-invalid lanes (k tail, partial float4 of a transposed operand) are steered to an
    // out-of-range offset / masked with selects instead of exec-mask branches around each load.
    constexpr uint32_t OOB = 0x80000000u;
    const int rowsA = min(BM, p.M - bm0), rowsB = min(BN, p.N - bn0);
    const int bz = blockIdx.y;
    p.A += bz * p.strideA; p.W += bz * p.strideW; p.C += bz * p.strideC;
    if (p.R) p.R += bz * p.strideC;
    const float* baseA = TA ? p.A + bm0 : p.A + (int64_t)bm0 * p.lda;
    const float* baseB = TB ? p.W + bn0 : p.W + (int64_t)bn0 * p.ldw;
    const int64_t elemsA = TA ? (int64_t)(p.K - 1) * p.lda + rowsA : (int64_t)(rowsA - 1) * p.lda + p.K;
    const int64_t elemsB = TB ? (int64_t)(p.K - 1) * p.ldw + rowsB : (int64_t)(rowsB - 1) * p.ldw + p.K;
    // make the descriptor inputs PROVABLY wave-uniform (readfirstlane), otherwise hipcc wraps every buffer load
    // in a waterfall loop (cdna_hip_programming.md T20)
    auto uniform_rsrc = [](const float* base, int64_t bytes) {
        const uint64_t b = reinterpret_cast<uint64_t>(base);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
        const int nb = __builtin_amdgcn_readfirstlane((int)(bytes < 0x7FFFFFFF ? bytes : 0x7FFFFFFF));
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, nb, 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t rsA = uniform_rsrc(baseA, elemsA * 4);
    const __amdgpu_buffer_rsrc_t rsB = uniform_rsrc(baseB, elemsB * 4);

    // Two register sets for the global->LDS staging: the loads of k-tile j+2 are in flight while k-tile j+1 (loaded one
    // iteration earlier, certainly arrived) is written to the other LDS buffer in the shadow of the MFMAs of tile j.
    f32x4 ra[2][A_F4], rb[2][B_F4];
    // Row sums of squares for the folded RMSNorm, in ONE canonical order whatever the tile configuration: eight running sums
    // per row (16-byte chunk index mod 8 along k), each fed in k order with an explicitly fused a0^2 + a1^2 + a2^2 + a3^2, then
    // the tree ((0+1)+(2+3)) + ((4+5)+(6+7)).  With BK = 32 a thread owns one chunk position; with BK = 16 it owns position c of
    // even k-tiles and 4 + c of odd ones.  (Needed for the tuner's freedom: every configuration must give the same bits.)
    static_assert(BK == 16 || BK == 32, "canonical row-sum order is defined for BK = 16 / 32");
    constexpr int NPAR = 32 / BK;
    float ssq[A_F4][NPAR];
#pragma unroll
    for (int i = 0; i < A_F4; ++i)
#pragma unroll
        for (int h = 0; h < NPAR; ++h) ssq[i][h] = 0.f;

    // one operand tile -> registers.  Non-transposed: memory [rows][K], float4 along K.  Transposed: memory
    // [K][rows], float4 along rows (scattered into LDS by store_tile).
    auto load_operand = [&](auto& regs, const __amdgpu_buffer_rsrc_t rs, int ld, int rows_valid, int k0, auto trans_tag, auto rows_tag) {
        constexpr bool T = decltype(trans_tag)::value;
        constexpr int ROWS = decltype(rows_tag)::value;
        constexpr int NF4 = ROWS * BK / 4 / NT;
#pragma unroll
        for (int i = 0; i < NF4; ++i) {
            const int idx = tid + i * NT;
            if constexpr (!T) {
                const int r = idx / RF4, c = (idx % RF4) * 4;
                const int gk = k0 + c;
                uint32_t off = (uint32_t)((r * ld + gk) * 4);
                if (KTAIL) off = gk < p.K ? off : OOB;
                f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
                if (KTAIL) {
#pragma unroll
                    for (int e = 1; e < 4; ++e) v[e] = gk + e < p.K ? v[e] : 0.f;
                }
                regs[i] = v;
            } else {
                const int kk = idx / (ROWS / 4), c = (idx % (ROWS / 4)) * 4;
                const int gk = k0 + kk;
                uint32_t off = (uint32_t)((gk * ld + c) * 4);
                off = (gk < p.K && c < rows_valid) ? off : OOB;
                f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
#pragma unroll
                for (int e = 1; e < 4; ++e) v[e] = c + e < rows_valid ? v[e] : 0.f;
                regs[i] = v;
            }
        }
    };
    auto load_tile = [&](int k0, auto set_tag) {
        constexpr int SET = decltype(set_tag)::value;
        load_operand(ra[SET], rsA, p.lda, rowsA, k0, std::integral_constant<bool, TA>{}, std::integral_constant<int, BM>{});
        load_operand(rb[SET], rsB, p.ldw, rowsB, k0, std::integral_constant<bool, TB>{}, std::integral_constant<int, BN>{});
    };

    auto store_tile = [&](int buf, auto set_tag, auto parity_tag) {
        constexpr int SET = decltype(set_tag)::value;
        constexpr int PAR = decltype(parity_tag)::value % NPAR;
        float* as = As + buf * BM * LDS_LD;
        float* bs = Bs + buf * BN * LDS_LD;
#pragma unroll
        for (int i = 0; i < A_F4; ++i) {
            int idx = tid + i * NT;
            const f32x4 v = ra[SET][i];
            if constexpr (!TA) {
                int r = idx / RF4, c = (idx % RF4) * 4;
                *reinterpret_cast<f32x4*>(as + r * LDS_LD + c) = v;
                ssq[i][PAR] = ssq[i][PAR] + __builtin_fmaf(v[3], v[3], __builtin_fmaf(v[2], v[2], __builtin_fmaf(v[1], v[1], v[0] * v[0])));
            } else {
                int kk = idx / (BM / 4), c = (idx % (BM / 4)) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) as[(c + e) * LDS_LD + kk] = v[e];
            }
        }
#pragma unroll
        for (int i = 0; i < B_F4; ++i) {
            int idx = tid + i * NT;
            const f32x4 v = rb[SET][i];
            if constexpr (!TB) {
                int r = idx / RF4, c = (idx % RF4) * 4;
                *reinterpret_cast<f32x4*>(bs + r * LDS_LD + c) = v;
            } else {
                int kk = idx / (BN / 4), c = (idx % (BN / 4)) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) bs[(c + e) * LDS_LD + kk] = v[e];
            }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    using Set0 = std::integral_constant<int, 0>;
    using Set1 = std::integral_constant<int, 1>;
    const int nk = (p.K + BK - 1) / BK;
    load_tile(0, Set0{});
    store_tile(0, Set0{}, Set0{});
    if (nk > 1) load_tile(BK, Set0{});            // k-tile j lives in register set (j - 1) & 1 until it is staged
    if (nk > 2) load_tile(2 * BK, Set1{});
    __syncthreads();

    const int lrow = lane & 31;
    const int lhalf = lane >> 5;

    auto mfma_steps = [&](int cur, int q0, int q1) {
        const float* as = As + cur * BM * LDS_LD + (wm * TM * 32 + lrow) * LDS_LD + lhalf * 4;
        const float* bs = Bs + cur * BN * LDS_LD + (wn * TN * 32 + lrow) * LDS_LD + lhalf * 4;
#pragma unroll
        for (int q = q0; q < q1; ++q) {
            if (KS > 1 && (q % KS) != ks) continue;
            f32x4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(as + i * 32 * LDS_LD + q * 8);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(bs + j * 32 * LDS_LD + q * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
    };
    auto iteration = [&](int kt, auto set_tag, auto next_parity) {
        const int cur = kt & 1;
        mfma_steps(cur, 0, 1);
        if (kt + 1 < nk) store_tile(cur ^ 1, set_tag, next_parity);   // k-tile kt+1: in registers since the previous iteration
        if (kt + 3 < nk) load_tile((kt + 3) * BK, set_tag);     // refill the set just drained
        mfma_steps(cur, 1, BK / 8);
        __syncthreads();
    };
    for (int kt = 0; kt < nk; kt += 2) {
        iteration(kt, Set0{}, Set1{});                            // kt even: the tile staged is odd
        if (kt + 1 < nk) iteration(kt + 1, Set1{}, Set0{});
    }

    // ---- intra-block split-K: fold the partner group's accumulators through LDS (fixed order: group 0 + group 1)
    if constexpr (KS > 1) {
        static_assert(KS == 2, "");
        constexpr int GT = WGM * WGN * 64;
        float* xch = smem;                       // the operand tiles are dead after the last barrier of the main loop
        const int gt = tid % GT;
        if (ks == 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) xch[((i * TN + j) * 16 + e) * GT + gt] = acc[i][j][e];
        }
        __syncthreads();
        if (ks == 0) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] += xch[((i * TN + j) * 16 + e) * GT + gt];
        }
    }

    // ---- per-row 1/rms of A (RMSNorm folded into the GEMM) -----------------------------------
    if (p.flags & GEMM_RMS_ROWSCALE) {
        if constexpr (!TA) {
#pragma unroll
            for (int i = 0; i < A_F4; ++i) {
                float s = ssq[i][0];
                s += dpp_f<0xB1>(s);
                s += dpp_f<0x4E>(s);    // RF4 (4 or 8) consecutive lanes share one row
                if constexpr (NPAR == 1) {
                    s += dpp_f<0x141>(s);                          // (0123) + (4567): the other half of the row's 8 lanes
                } else {
                    float s1 = ssq[i][1];
                    s1 += dpp_f<0xB1>(s1);
                    s1 += dpp_f<0x4E>(s1);
                    s = s + s1;                                    // (0123) + (4567)
                }
                int r = (tid + i * NT) / RF4;
                if ((tid % RF4) == 0) rowscale_s[r] = rsqrtf(s / (float)p.K + p.rms_eps);
            }
        }
        __syncthreads();
    }

    // ---- epilogue ----------------------------------------------------------------------------
    if (KS > 1 && ks != 0) return;
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
    const bool swiglu = (p.flags & GEMM_SWIGLU) != 0;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int lr = wm * TM * 32 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
            const int gm = bm0 + lr;
            if (gm >= p.M) continue;
            const float rs = (p.flags & GEMM_RMS_ROWSCALE) ? rowscale_s[lr] : 1.f;
            if (swiglu) {
                static_assert(TN >= 1, "");
                if constexpr (TN % 2 == 0) {
#pragma unroll
                    for (int j = 0; j < TN; j += 2) {
                        const int gn = bn0 + wn * TN * 32 + j * 32 + lrow;       // packed column of the value
                        if (gn + 32 >= p.N + 32 || gn >= p.N) continue;
                        float val = acc[i][j][e] * rs, gate = acc[i][j + 1][e] * rs;
                        if (p.bias) { val += p.bias[gn]; gate += p.bias[gn + 32]; }
                        const int on = (gn / 64) * 32 + (gn % 64);                 // output (hidden) column
                        p.C[(int64_t)gm * p.ldc + on] = val * siluf(gate);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int gn = bn0 + wn * TN * 32 + j * 32 + lrow;
                    if (gn >= p.N) continue;
                    float v = acc[i][j][e] * rs;
                    if (p.bias) v += p.bias[gn];
                    if (p.flags & GEMM_SILU) v = siluf(v);
                    if (p.R) v += p.R[(int64_t)gm * p.ldr + gn];
                    if (p.flags & GEMM_ACCUMULATE) v += p.C[(int64_t)gm * p.ldc + gn];
                    p.C[(int64_t)gm * p.ldc + gn] = v;
                    if (p.C2) {
                        const int ts = gm % p.c2_S;
                        const int keep = p.c2_hi - p.c2_lo;
                        const int rank = (ts >= p.c2_lo && ts < p.c2_hi) ? ts - p.c2_lo : ((p.c2_last && ts == p.c2_S - 1) ? keep : -1);
                        if (rank >= 0) p.C2[((int64_t)(gm / p.c2_S) * (keep + p.c2_last) + rank) * p.ldc2 + gn] = v;
                    }
                }
            }
        }
    }
}

// ---- optional per-launch timing (bench.py roofline leg): HIP events on the launch stream --------------------
struct ProfRec { hipEvent_t a, b; int cls; double flops; int M, N, K, flags, batch, bm, bn; };
static int g_prof_mask = 0;            // bit c set: time launches of profile class c
static int g_prof_stride = 1;          // ... every g_prof_stride-th of them
static int g_prof_tick = 0;
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_event_pool;

static hipEvent_t prof_event() {
    if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

bool gemm_bf16_profile_active();
bool glue_profile_active();            // prof.cpp: event-timed launches cannot be captured into a graph either
bool gemm_profile_active() { return g_prof_mask != 0 || gemm_bf16_profile_active() || glue_profile_active(); }

// The dispatcher's process-global state (tile choices per shape, the tuning-cache file, the profiling log and its event pool, the static
// per-instantiation attribute flags) is guarded by ONE recursive mutex taken at its entries (gemm, gemm_pair, gemm_x3sk_fill): ctypes releases the
// GIL, and two engines may be driven from two host threads (tools/two_stream_rollout.py).  Launches are asynchronous, so the lock is held for
// microseconds except while a shape is being timed for the first time.
static std::recursive_mutex g_gemm_mu;

int gemm_profile_enable(int mask) {
    std::lock_guard<std::recursive_mutex> lock(g_gemm_mu);
    g_prof_stride = (mask >> 27) > 0 ? (mask >> 27) : 1;          // bits 27..30: stride; bits 0..26: profile classes (27 of them)
    mask &= 0x7FFFFFF;
    g_prof_tick = 0;
    g_prof_mask = mask;
    return 0;
}

// Sums elapsed time / algorithmic flops / launch count per profile class and clears the log.
int gemm_profile_read(double* ms, double* flops, int64_t* count, int nclass) {
    std::lock_guard<std::recursive_mutex> lock(g_gemm_mu);
    for (int i = 0; i < nclass; ++i) { ms[i] = 0; flops[i] = 0; count[i] = 0; }
    // D4_GEMM_LOG=1: also print a per-shape table (launches, total ms, TFLOP/s) to stderr
    static const bool log_shapes = getenv("D4_GEMM_LOG") != nullptr;
    struct Agg { ProfRec r; double ms, fl; int64_t n; };
    std::vector<Agg> shapes;
    for (auto& r : g_prof) {
        D4_HIP(hipEventSynchronize(r.b));
        float t = 0.f;
        D4_HIP(hipEventElapsedTime(&t, r.a, r.b));
        if (r.cls < nclass) { ms[r.cls] += t; flops[r.cls] += r.flops; count[r.cls] += 1; }
        if (log_shapes) {
            bool hit = false;
            for (auto& a : shapes)
                if (a.r.M == r.M && a.r.N == r.N && a.r.K == r.K && a.r.flags == r.flags && a.r.batch == r.batch) { a.ms += t; a.fl += r.flops; a.n += 1; hit = true; break; }
            if (!hit) shapes.push_back(Agg{r, t, r.flops, 1});
        }
        g_event_pool.push_back(r.a);
        g_event_pool.push_back(r.b);
    }
    if (log_shapes) {
        double tot = 0;
        for (auto& a : shapes) tot += a.ms;
        for (auto& a : shapes)
            fprintf(stderr, "[d4 gemm] M %6d N %5d K %5d batch %2d flags %3d tile %3dx%-3d : %6lld launches %9.3f ms (%5.1f %%) avg %7.1f us %6.1f TF/s\n",
                    a.r.M, a.r.N, a.r.K, a.r.batch, a.r.flags, a.r.bm, a.r.bn, (long long)a.n, a.ms, 100 * a.ms / tot, 1e3 * a.ms / a.n, a.fl / a.ms / 1e9);
    }
    g_prof.clear();
    return 0;
}

static inline double gemm_flops(const GemmArgs& p) { return p.algo_flops > 0 ? p.algo_flops : 2.0 * p.M * p.N * p.K * (p.batch > 0 ? p.batch : 1); }

// THE timed launch: every launch of the dispatcher goes through here.  `launch(ea, eb)` enqueues the kernel; when profile class `cls` is enabled and this
// launch is due by the stride it gets an event pair from the pool and a log record (`shape`: what the per-shape table prints; bm x bn: the tile).  The two
// events ride on the dispatch itself (hipExtLaunchKernelGGL: its begin / end timestamps): no extra barrier packets on the stream, and the elapsed time is
// the kernel's own duration (what rocprofv3 --kernel-trace reports).
template <class Launch>
static int timed_launch(int cls, const GemmArgs& shape, int bm, int bn, double flops, Launch&& launch) {
    const bool timed = ((g_prof_mask >> cls) & 1) && (g_prof_tick++ % g_prof_stride) == 0;
    if (!timed) return launch(nullptr, nullptr);
    const ProfRec rec{prof_event(), prof_event(), cls, flops, shape.M, shape.N, shape.K, shape.flags, shape.batch, bm, bn};
    if (int rc = launch(rec.a, rec.b)) return rc;
    g_prof.push_back(rec);
    return 0;
}

static inline double tile_cost(const GemmArgs& p, int BM, int BN, int slots) {
    // co-resident blocks share a CU's matrix pipes: a CU's time ~ (blocks it hosts) x (tile area)
    const double blocks = (double)cdiv(p.M, BM) * cdiv(p.N, BN) * (p.batch > 0 ? p.batch : 1);
    return ceil(blocks / slots) * BM * BN;
}

template <int BM, int BN, int WGM, int WGN, int BK, int KS, bool TA, bool TB>
static int launch_cfg(const GemmArgs& p, hipStream_t stream, hipEvent_t ea, hipEvent_t eb) {
    constexpr int LDS_LD = BK + 4;
    const int nblk = cdiv(p.M, BM) * cdiv(p.N, BN);
    const size_t lds = (size_t)(2 * BM * LDS_LD + 2 * BN * LDS_LD + BM) * sizeof(float);
    const bool ktail = (p.K % BK) != 0;
    auto k = ktail ? gemm_kernel<BM, BN, WGM, WGN, BK, KS, TA, TB, true> : gemm_kernel<BM, BN, WGM, WGN, BK, KS, TA, TB, false>;
    static DeviceOnce attr_set[2];
    if (attr_set[ktail].need()) {
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set[ktail].done();
    }
    const dim3 grid(nblk, p.batch > 0 ? p.batch : 1), block(WGM * WGN * 64 * KS);
    if (ea) hipExtLaunchKernelGGL(k, grid, block, (uint32_t)lds, stream, ea, eb, 0, p);
    else hipLaunchKernelGGL(k, grid, block, lds, stream, p);
    D4_LAUNCH_CHECK();
    return 0;
}

// ---- the first family's tile configurations ------------------------------------------------------------------
// All configurations walk k in the same order with the same MFMA, so every output element is the same
// bit pattern whichever one runs: the choice is a pure performance decision.
enum TileCfg { T128x128_2x4 = 0, T128x128_4x2, T128x96_4x1, T64x128_2x2, T64x64_2x2, T256x128_4x4, T64x128_k16, T64x64_k16, N_TILE_CFG };
static const char* const kTileName[N_TILE_CFG] = {"128x128/2x4", "128x128/4x2", "128x96/4x1", "64x128/2x2", "64x64/2x2", "256x128/4x4", "64x128/2x2/k16", "64x64/2x2/k16"};
static const int kTileBM[N_TILE_CFG] = {128, 128, 128, 64, 64, 256, 64, 64}, kTileBN[N_TILE_CFG] = {128, 128, 96, 128, 64, 128, 128, 64};
// rocprofv3 shows the instantiation as d4::gemm_kernel<BM, BN, WGM, WGN, BK, 1, transA, transB, ktail>
static const char* const kTileKernel[N_TILE_CFG] = {
    "gemm_kernel<128, 128, 2, 4, 32, 1", "gemm_kernel<128, 128, 4, 2, 32, 1", "gemm_kernel<128, 96, 4, 1, 32, 1", "gemm_kernel<64, 128, 2, 2, 32, 1",
    "gemm_kernel<64, 64, 2, 2, 32, 1", "gemm_kernel<256, 128, 4, 4, 32, 1", "gemm_kernel<64, 128, 2, 2, 16, 1", "gemm_kernel<64, 64, 2, 2, 16, 1"};

template <bool TA, bool TB>
static bool cfg_valid(int id, const GemmArgs& p) {
    const bool swiglu = (p.flags & GEMM_SWIGLU) != 0;
    switch (id) {
        case T128x128_2x4: return !swiglu;
        case T128x128_4x2: return true;
        case T128x96_4x1: return !swiglu && !TA && !TB;
        case T64x128_2x2: return true;
        case T64x64_2x2: return !swiglu;
        case T256x128_4x4: return !swiglu && !TA && !TB;
        case T64x128_k16: return !TA && !TB;
        case T64x64_k16: return !swiglu && !TA && !TB;
    }
    return false;
}

template <bool TA, bool TB>
static int launch_id(int id, const GemmArgs& p, hipStream_t stream, hipEvent_t ea, hipEvent_t eb) {
    switch (id) {
        // 8 waves (2 x 4, wave tile 64 x 32): two co-resident blocks put 4 waves on every SIMD
        case T128x128_2x4: return launch_cfg<128, 128, 2, 4, 32, 1, TA, TB>(p, stream, ea, eb);
        // (the SiLU-GLU epilogue pairs two N sub-tiles inside one wave -> 4 x 2 waves, wave tile 32 x 64)
        case T128x128_4x2: return launch_cfg<128, 128, 4, 2, 32, 1, TA, TB>(p, stream, ea, eb);
        case T128x96_4x1:
            if constexpr (!TA && !TB) return launch_cfg<128, 96, 4, 1, 32, 1, TA, TB>(p, stream, ea, eb);
            break;
        case T64x128_2x2: return launch_cfg<64, 128, 2, 2, 32, 1, TA, TB>(p, stream, ea, eb);
        case T64x64_2x2: return launch_cfg<64, 64, 2, 2, 32, 1, TA, TB>(p, stream, ea, eb);
        case T256x128_4x4:
            if constexpr (!TA && !TB) return launch_cfg<256, 128, 4, 4, 32, 1, TA, TB>(p, stream, ea, eb);
            break;
        case T64x128_k16:
            if constexpr (!TA && !TB) return launch_cfg<64, 128, 2, 2, 16, 1, TA, TB>(p, stream, ea, eb);
            break;
        case T64x64_k16:
            if constexpr (!TA && !TB) return launch_cfg<64, 64, 2, 2, 16, 1, TA, TB>(p, stream, ea, eb);
            break;
    }
    D4_REQUIRE(false, "gemm: tile configuration %d not available for this operand layout", id);
}

// Static choice (used for shapes that cannot be timed: tiny, non-idempotent, or first seen under stream capture).
template <bool TA, bool TB>
static int heuristic_cfg(const GemmArgs& p) {
    const bool swiglu = (p.flags & GEMM_SWIGLU) != 0;
    const int nb = p.batch > 0 ? p.batch : 1;
    const int64_t b128 = (int64_t)cdiv(p.M, 128) * cdiv(p.N, 128) * nb;
    // 256 CUs: prefer the big tile once it yields >= ~1.5 blocks per CU; long-K backward GEMMs (dW = dZ^T X with
    // K = batch*time rows) take it earlier: one big tile per CU beats two rounds of small ones.
    if (b128 >= 360 || (b128 >= 192 && p.K >= 2048)) {
        if (swiglu) return T128x128_4x2;
        // 128 x 96 tiles when they quantise better onto the 256 CUs (the fused q|k|v projection, N = 1552: 30 x 13 = 390
        // tiles of 128 x 128 leave half the CUs with one block and half with two; 30 x 17 = 510 fit once).
        if (!TA && !TB && tile_cost(p, 128, 96, 256) < 0.8 * tile_cost(p, 128, 128, 256)) return T128x96_4x1;
        return T128x128_2x4;
    }
    if (swiglu || (p.N > 64 && (int64_t)cdiv(p.M, 64) * cdiv(p.N, 128) * nb >= 256)) return T64x128_2x2;
    return T64x64_2x2;
}

// The first family as the family table sees it: plain functions that pick the (transA, transB) instantiation inside.
#define D4_TILE_BY_LAYOUT(fn, ...)                                                          \
    const bool ta = p.flags & GEMM_TRANS_A, tb = p.flags & GEMM_TRANS_B;                    \
    if (!ta && !tb) return fn<false, false>(__VA_ARGS__);                                   \
    if (!ta && tb) return fn<false, true>(__VA_ARGS__);                                     \
    if (ta && tb) return fn<true, true>(__VA_ARGS__);                                       \
    return fn<true, false>(__VA_ARGS__)
static int tile_configs() { return N_TILE_CFG; }
static bool tile_config_valid(int c, const GemmArgs& p) { D4_TILE_BY_LAYOUT(cfg_valid, c, p); }
static int tile_launch(int c, const GemmArgs& p, hipStream_t stream, hipEvent_t ea, hipEvent_t eb) { D4_TILE_BY_LAYOUT(launch_id, c, p, stream, ea, eb); }
static const char* tile_config_name(int c) { return kTileName[c]; }
static void tile_config_tile(int c, int* bm, int* bn) { *bm = kTileBM[c]; *bn = kTileBN[c]; }
static int tile_heuristic(const GemmArgs& p) { D4_TILE_BY_LAYOUT(heuristic_cfg, p); }
// the tuner leaves the 128-row tiles out under 64 tiles of 128 x 128
static bool tile_tune_skip(int c, const GemmArgs& p) {
    return (c == T256x128_4x4 || c == T128x128_2x4 || c == T128x128_4x2) && (int64_t)cdiv(p.M, 128) * cdiv(p.N, 128) * (p.batch > 0 ? p.batch : 1) < 64;
}
#undef D4_TILE_BY_LAYOUT

int gemm_configs() { return N_TILE_CFG; }
// would gemm() under gemm_force_config(c) run configuration c of THIS family on the call?  (The few-row kernel and the mirror-weight families come first there.)
bool gemm_config_valid(int c, const GemmArgs& p) {
    if (c < 0 || c >= N_TILE_CFG || p.Wb || p.M < 1 || gemm_skinny_applicable(p)) return false;
    return tile_config_valid(c, p);
}

// ---- profile classes: the tuned families' configurations in table order, then the single-form kernels ---------------------------------------
static const int kClsTile = 0, kClsV2 = N_TILE_CFG, kClsX3 = kClsV2 + gemm2_configs();
static const int kClsX3SK = kClsX3 + gemm_x3_configs();       // the persistent split-operand form (gemm_x3sk.hip), plain and filled
static const int kClsH2 = kClsX3SK + 1;                       // the fp16x2 family (gemm_h2.hip): ONE class for all its tiles
static const int kClsKsplit = kClsX3SK + 2;                   // the few-row k-split form (gemm2.hip)
int gemm_profile_classes() { return kClsKsplit + 1; }
const char* gemm_profile_class_name(int c) {
    if (c == kClsKsplit) return "gemm2_ksplit_kernel";
    if (c == kClsH2) return "gemm_h2_kernel";
    if (c == kClsX3SK) return gemm_x3sk_name();
    if (c >= kClsX3) return gemm_x3_config_name(c - kClsX3);
    if (c >= kClsV2) return gemm2_config_name(c - kClsV2);
    return c >= 0 ? kTileKernel[c] : "";
}

// ---- the tuned families ------------------------------------------------------------------------------------------------------------------------
// Shape -> configuration, per family, filled by timing every valid configuration the first time a shape is seen (the engine's
// shapes are fixed by (batch, frames, config), a few dozen in all).  D4_GEMM_AUTOTUNE=0 keeps the static choice.
struct TuneKey {
    int M, N, K, flags, batch;
    bool operator<(const TuneKey& o) const { return std::tie(M, N, K, flags, batch) < std::tie(o.M, o.N, o.K, o.flags, o.batch); }
};
static std::map<TuneKey, int> g_tuned[4];

// One row per family whose configurations all give the same bits, so that the choice among them is free: what the tuner, the tuning-cache file, the
// force hook and the timed launch need to know about it.
struct Family {
    int code;                                  // D4_GEMM_*
    const char* tag;                           // D4_GEMM_LOG: "[d4 <tag>] tuned ..."
    int (*configs)();
    bool (*config_valid)(int, const GemmArgs&);
    int (*launch)(int, const GemmArgs&, hipStream_t, hipEvent_t, hipEvent_t);
    const char* (*config_name)(int);
    void (*config_tile)(int, int*, int*);
    int (*heuristic)(const GemmArgs&);         // the static choice, for a shape that cannot be timed
    bool (*tune_skip)(int, const GemmArgs&);   // configurations the tuner leaves out (null: none)
    int id_base;                               // configuration c is id_base + c in the tuning-cache files
    int first_class;                           // profile class of configuration 0 ...
    bool class_per_config;                     // ... one class per configuration, or that one for the family
    bool strict_few_rows;                      // D4_GEMM_AUTOTUNE=strict: a product of <= 512 rows missing from the table takes the static choice
    std::map<TuneKey, int>* tuned;
};
enum { FAM_TILE = 0, FAM_V2, FAM_X3, FAM_H2, N_FAMILIES };
static const Family kFamilies[N_FAMILIES] = {
    {D4_GEMM_TILE, "gemm", tile_configs, tile_config_valid, tile_launch, tile_config_name, tile_config_tile, tile_heuristic, tile_tune_skip, 0, kClsTile, true, true, &g_tuned[FAM_TILE]},
    {D4_GEMM_V2, "gemm2", gemm2_configs, gemm2_config_valid, gemm2_launch, gemm2_config_name, gemm2_config_tile, gemm2_heuristic, nullptr, 100, kClsV2, true, true, &g_tuned[FAM_V2]},
    {D4_GEMM_X3, "gemm_x3", gemm_x3_configs, gemm_x3_config_valid, gemm_x3_launch, gemm_x3_config_name, gemm_x3_config_tile, gemm_x3_heuristic, nullptr, 300, kClsX3, true, false, &g_tuned[FAM_X3]},
    {D4_GEMM_H2, "gemm_h2", gemm_h2_configs, gemm_h2_config_valid, gemm_h2_launch, gemm_h2_config_name, gemm_h2_config_tile, gemm_h2_heuristic, nullptr, 400, kClsH2, false, false, &g_tuned[FAM_H2]},
};

// ---- the test hook (d4_gemm_force_config): THE decoding of its codes --------------------------------------------------------------------------
//   < 0 nothing forced | c < 100 configuration c of the first family | 100 + c of gemm2.hip | 199 the few-row k-split form on any shape it can run |
//   200 + c of gemm_bf16.hip | 300 + c of gemm_x3.hip | 400 + c of gemm_h2.hip | 500 + c of gemm_bf16a.hip
struct Forced { int family = -1, config = -1; };       // family: a D4_GEMM_* code; -1: the rules and the tuner decide
static Forced forced_decode(int code) {
    if (code < 0) return {};
    if (code < 100) return {D4_GEMM_TILE, code};
    if (code == 199) return {D4_GEMM_V2_KSPLIT, 0};
    if (code < 200) return {D4_GEMM_V2, code - 100};
    if (code < 300) return {D4_GEMM_BF16, code - 200};
    if (code < 400) return {D4_GEMM_X3, code - 300};
    if (code < 500) return {D4_GEMM_H2, code - 400};
    return {D4_GEMM_BF16A, code - 500};
}
// the two bf16 kernels keep their hooks in gemm_bf16.hip (they have one form per call, chosen there); to the fp32 families such a code forces nothing
static Forced forced_fp32(const Forced& f) { return f.family == D4_GEMM_BF16 || f.family == D4_GEMM_BF16A ? Forced{} : f; }
static Forced g_forced;
// One family is forced at a time: every call first clears the hooks of the other families.  Returns the number of configurations of the family addressed
// (nothing forced: the first family's).
int gemm_force_config(int code) {
    const Forced f = forced_decode(code);
    gemm_bf16a_force_config(f.family == D4_GEMM_BF16A ? f.config : -1);
    const int n_bf16 = gemm_bf16_force_config(f.family == D4_GEMM_BF16 ? f.config : -1);
    g_forced = forced_fp32(f);
    switch (f.family) {
        case D4_GEMM_V2: case D4_GEMM_V2_KSPLIT: return gemm2_configs();
        case D4_GEMM_BF16: return n_bf16;
        case D4_GEMM_X3: return gemm_x3_configs();
        case D4_GEMM_H2: return gemm_h2_configs();
        case D4_GEMM_BF16A: return gemm_bf16a_configs();
    }
    return N_TILE_CFG;
}

// D4_GEMM_TUNE_CACHE=<file>: the shape -> configuration table is read at first use and every new entry is appended, so a
// later process (a profiler pass, a restarted trainer) starts with the choices already made and never re-times.
static const char* tune_cache_path() {
    static const char* path = getenv("D4_GEMM_TUNE_CACHE");
    return path;
}
static void tune_cache_read(const char* path) {
    if (!path) return;
    if (FILE* f = fopen(path, "r")) {
        char line[256];
        while (fgets(line, sizeof(line), f)) {
            TuneKey k; int id;
            if (line[0] == '#' || sscanf(line, "%d %d %d %d %d %d", &k.M, &k.N, &k.K, &k.flags, &k.batch, &id) != 6) continue;
            for (const Family& F : kFamilies)
                if (id >= F.id_base && id < F.id_base + F.configs()) (*F.tuned)[k] = id - F.id_base;
        }
        fclose(f);
    }
}
// D4_GEMM_TUNE_DEFAULT (set by dreamer4_amd._lib to the table shipped in the package): preloaded read-only, so the shapes of the
// benchmark configurations never time anything (no first-call synchronisation, the same choice on every run);
// D4_GEMM_TUNE_CACHE=<file>: read as well, and every newly tuned shape is appended to it.
static void tune_cache_load() {
    static bool loaded = false;
    if (loaded) return;
    loaded = true;
    tune_cache_read(getenv("D4_GEMM_TUNE_DEFAULT"));
    tune_cache_read(tune_cache_path());
}
static void tune_cache_append(const TuneKey& k, int id) {
    const char* path = tune_cache_path();
    if (!path) return;
    if (FILE* f = fopen(path, "a")) {
        fprintf(f, "%d %d %d %d %d %d\n", k.M, k.N, k.K, k.flags, k.batch, id);
        fclose(f);
    }
}

// D4_GEMM_AUTOTUNE: 1 / unset = time a new shape's configurations at first use; 0 = never time (static choice); strict = never time AND fail
// on a shape that would have been timed (the multi-rank bench: every rank must take its choices from the shipped table, not from its own clock).
static int tune_mode() {
    static const int mode = [] {
        const char* v = getenv("D4_GEMM_AUTOTUNE");
        if (!v) return 1;
        if (!strcmp(v, "strict")) return 2;
        return atoi(v) == 0 ? 0 : 1;
    }();
    return mode;
}
static int tune_strict_check(const GemmArgs& p) {
    D4_REQUIRE(tune_mode() != 2, "gemm: shape M=%d N=%d K=%d flags=%d batch=%d is not in the shipped tile table (dreamer4_amd/gemm_tune_default.txt) and "
               "D4_GEMM_AUTOTUNE=strict forbids timing it here: run the workload once on one GPU with D4_GEMM_TUNE_CACHE=<file> and merge the new lines",
               p.M, p.N, p.K, p.flags, p.batch > 0 ? p.batch : 1);
    return 0;
}

// One launch of configuration c of a family, under its profile class.
static int family_launch(const Family& F, int c, const GemmArgs& p, hipStream_t stream) {
    int bm, bn;
    F.config_tile(c, &bm, &bn);
    return timed_launch(F.first_class + (F.class_per_config ? c : 0), p, bm, bn, gemm_flops(p), [&](hipEvent_t ea, hipEvent_t eb) { return F.launch(c, p, stream, ea, eb); });
}

// THE tuner: one warm launch, then the best of two timed pairs, for every valid configuration.
static int autotune(const Family& F, const GemmArgs& p, hipStream_t stream, int* best_out) {
    hipEvent_t e0 = prof_event(), e1 = prof_event();
    int best = -1, rc = 0;
    float best_ms = 0.f;
    for (int c = 0; c < F.configs() && !rc; ++c) {
        if (!F.config_valid(c, p) || (F.tune_skip && F.tune_skip(c, p))) continue;
        if ((rc = F.launch(c, p, stream, nullptr, nullptr))) break;              // warm (attribute set, code resident)
        float ms = 1e30f;
        for (int rep = 0; rep < 2 && !rc; ++rep) {
            (void)hipEventRecord(e0, stream);
            if ((rc = F.launch(c, p, stream, nullptr, nullptr))) break;
            if ((rc = F.launch(c, p, stream, nullptr, nullptr))) break;
            (void)hipEventRecord(e1, stream);
            if (hipEventSynchronize(e1) != hipSuccess) { rc = 1; break; }
            float t = 0.f;
            (void)hipEventElapsedTime(&t, e0, e1);
            ms = t < ms ? t : ms;
        }
        if (!rc && (best < 0 || ms < best_ms)) { best = c; best_ms = ms; }
    }
    g_event_pool.push_back(e0);
    g_event_pool.push_back(e1);
    if (rc) return rc;
    D4_REQUIRE(best >= 0, "%s: no configuration for M=%d N=%d K=%d flags=%d", F.tag, p.M, p.N, p.K, p.flags);
    if (getenv("D4_GEMM_LOG"))
        fprintf(stderr, "[d4 %s] tuned M %6d N %5d K %5d batch %2d flags %3d -> %s (%.1f us)\n", F.tag, p.M, p.N, p.K, p.batch, p.flags, F.config_name(best), 500.f * best_ms);
    *best_out = best;
    return 0;
}

// THE tuned launch of a family: the forced configuration where it is valid, else the table's, else — for a call that can be timed — the tuner's, which is
// remembered and appended to the cache file; every other call takes the static choice.
static int tuned_launch(const Family& F, const GemmArgs& p, hipStream_t stream) {
    if (g_forced.family == F.code && F.config_valid(g_forced.config, p)) return family_launch(F, g_forced.config, p, stream);
    const TuneKey key{p.M, p.N, p.K, p.flags, p.batch};
    tune_cache_load();
    auto it = F.tuned->find(key);
    if (it != F.tuned->end() && F.config_valid(it->second, p)) return family_launch(F, it->second, p, stream);
    // timing repeats the launch, so the call must be idempotent (no accumulate, no in-place residual), worth it
    // (>= 0.1 GFLOP), and the stream must not be capturing
    const bool idempotent = !(p.flags & GEMM_ACCUMULATE) && p.R != p.C && p.A != p.C;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cap);
    if (tune_mode() == 0 || !idempotent || cap != hipStreamCaptureStatusNone || 2.0 * p.M * p.N * p.K * (p.batch > 0 ? p.batch : 1) < 1e8)
        return family_launch(F, F.heuristic(p), p, stream);
    // strict mode: a FEW-ROW product missing from the table (the heads' MLPs at a per-rank batch other than the shipped 256: M = the batch) takes the static
    // choice — a rule on the shape, so every rank still makes the same one without a clock; anything larger must be in the table
    if (tune_mode() == 2 && F.strict_few_rows && p.M <= 512) return family_launch(F, F.heuristic(p), p, stream);
    if (int rc = tune_strict_check(p)) return rc;
    int best = 0;
    if (int rc = autotune(F, p, stream, &best)) return rc;
    (*F.tuned)[key] = best;
    tune_cache_append(key, F.id_base + best);
    return family_launch(F, best, p, stream);
}

// ---- the single-form kernels under their profile classes ----------------------------------------------------------------------------------------
static int launch_ksplit(const GemmArgs& p, hipStream_t stream) {
    return timed_launch(kClsKsplit, p, 32, 64, gemm_flops(p), [&](hipEvent_t ea, hipEvent_t eb) { return gemm2_ksplit_launch(p, stream, ea, eb); });
}
static int launch_x3sk(const GemmArgs& p, hipStream_t stream) {
    return timed_launch(kClsX3SK, p, 128, 128, gemm_flops(p), [&](hipEvent_t ea, hipEvent_t eb) { return gemm_x3sk_launch(p, stream, ea, eb); });
}
// The filled form of the persistent kernel (gemm_x3sk.hip): accounted under the SAME profile class as the plain form, with the flops of both problems —
// the class list does not grow (gemm_profile_enable keeps its stride field at bit 27).
int gemm_x3sk_fill(const GemmArgs& p, const GemmArgs& fill, int fill_tiles, hipStream_t stream) {
    std::lock_guard<std::recursive_mutex> lock(g_gemm_mu);
    const double fill_flops = fill_tiles > 0 ? 2.0 * fill.M * fill.N * fill.K * fill_tiles / (double)gemm_x3sk_fill_tiles(fill) : 0.0;
    return timed_launch(kClsX3SK, p, 128, 128, gemm_flops(p) + fill_flops,
                        [&](hipEvent_t ea, hipEvent_t eb) { return gemm_x3sk_fill_launch(p, fill, fill_tiles, stream, ea, eb); });
}

// ---- THE route: which family runs a call --------------------------------------------------------------------------------------------------------
// A RULE on the call's shape and layout, never a timing: the families sum k in different orders, so a timing-dependent choice between them would make
// results depend on the tuner.  (DESIGN.md 29 has the table.)

// The output row map (GemmArgs::rm_*): well formed, and on a call whose epilogue the two mapped kernels implement (bias and row scale only).
bool gemm_rowmap_ok(const GemmArgs& p) {
    if (p.rm_Sc <= 0) return true;
    return p.rm_lo <= p.rm_Sc && p.C && !p.R && !p.C2 && !p.Cb && !p.C2b &&
           !(p.flags & ~GEMM_RMS_ROWSCALE);
}
// A launcher that does not implement the map must not ignore it.
int gemm_rowmap_refused(const GemmArgs& p, const char* who) {
    D4_REQUIRE(p.rm_Sc <= 0, "%s: this kernel family does not implement the output row map (M=%d N=%d K=%d flags=%d)", who, p.M, p.N, p.K, p.flags);
    return 0;
}

// Which calls of an fp16x2 engine that family takes.  Measured on MI355X (tools/gemm_h2_bench.py, profiles/r05c_*): x1.2-2.0 the f32-input MFMA kernels
// wherever a launch has a few hundred rows, N >= 256 and a k loop of some length; level or behind on launches of under ~1.2 G multiply-adds (the
// 512 x 512 / 256 x 512 projections at 3584 rows) and at K < 128; few-row calls stay on the few-row kernel.
static bool h2_rule(const GemmArgs& p, const Forced& f) {
    if (!gemm_h2_applicable(p) || gemm_skinny_applicable(p)) return false;
    if (f.family >= 0) return f.family == D4_GEMM_H2;       // a forced tile of this family: every call it can run; of another family: none
    return p.M >= 256 && p.K >= 128 && p.N >= 64 && (double)p.M * p.N * p.K * (p.batch > 0 ? p.batch : 1) >= 1.2e9;
}

static GemmRoute route(const GemmArgs& p, const Forced& f) {
    GemmRoute r{D4_GEMM_TILE, p};
    GemmArgs& q = r.args;
    const bool by_rule = f.family < 0;
    // fp16x2 engine mode (two fp16 planes of W + row scales, gemm_h2.hip): every call the rule does not name drops the planes and runs on the f32-input kernels
    if (q.Wb && q.wplane > 0 && q.wscale) {
        if (h2_rule(q, f)) { r.family = D4_GEMM_H2; return r; }
        q.Wb = nullptr; q.wplane = 0; q.wscale = nullptr; q.aexp = nullptr;
    }
    // split-operand fp32 (three bf16 planes of W).  Measured on MI355X (tools/gemm_x3_bench.py, profiles/r02_gemm_split_operands.txt): it wins where a
    // launch has enough wide tiles to hide its heavier staging — the SiLU-GLU input projections (N = 2 x 1376 ... 5504: 1.2-1.35x the f32-input MFMA
    // kernels) and other N >= 2048 projections (level to 1.3x) — and loses on the N <= 1552 shapes (0.8-0.95x; with the whole rollout as the clock
    // +3 .. +6 ms: profiles/r05b_x3_every_call_ab.txt); few-row calls stay on the few-row kernel.  Every such call of >= 1024 rows runs on the PERSISTENT
    // form (gemm_x3sk.hip: whole rounds as plain tiles, a last round that is at most half full as 128 x 64 half tiles — bit-identical to the plain kernel;
    // same-box A/B pairs, profiles/r03l_ab_late_changes.txt: 188.8 vs 191.8-192.4 (half-tile calls only) vs 199.3-200.0 ms (never) per step on a
    // mid-speed box, level on the fastest one).  Every other call drops the planes.
    if (q.Wb && q.wplane > 0) {
        const bool wide = ((q.flags & GEMM_SWIGLU) || q.N >= 2048) && !gemm_skinny_applicable(q);
        const int rm = q.rule_M > 0 ? q.rule_M : q.M;       // (rule_M: a caller that runs a subset of a product's rows keeps the family of the whole product)
        if (wide && by_rule && (gemm_x3sk_rule(q) || (gemm_x3sk_applicable(q) && rm >= 1024))) { r.family = D4_GEMM_X3SK; return r; }
        if (wide && rm >= 256 && gemm_x3_applicable(q)) { r.family = D4_GEMM_X3; return r; }
        q.Wb = nullptr; q.wplane = 0;
    }
    // bf16 engine: with a bf16 image of the activation both operands come by LDS-DMA
    if (q.Wb) { r.family = q.Ab && gemm_bf16a_applicable(q) ? D4_GEMM_BF16A : D4_GEMM_BF16; return r; }
    // f32 operands.  A forced configuration of the LDS-DMA family runs wherever it is valid, ahead of the few-row kernel
    if (f.family == D4_GEMM_V2 && gemm2_config_valid(f.config, q)) r.family = D4_GEMM_V2;
    else if (gemm_skinny_applicable(q)) r.family = D4_GEMM_SKINNY;
    // few rows x long K (the heads' hidden layers at rollout batch): the contraction cut four ways inside the workgroup
    else if (by_rule ? gemm2_ksplit_rule(q) : (f.family == D4_GEMM_V2_KSPLIT && gemm2_ksplit_applicable(q))) r.family = D4_GEMM_V2_KSPLIT;
    // (a forced tile of a mirror-weight family leaves the f32 calls to the rule)
    else if ((by_rule || f.family == D4_GEMM_X3 || f.family == D4_GEMM_H2) && gemm2_applicable(q)) r.family = D4_GEMM_V2;
    return r;
}
GemmRoute gemm_route(const GemmArgs& p, int forced) { return route(p, forced_fp32(forced_decode(forced))); }

// The engine asks these before it replaces a product by a kernel that carries a family's bits (engine.hip: the latent-token ends, the last layer's
// split projection, the FF fill): would gemm() run this call — these exact arguments, weight planes and rule_M included — there BY ITS RULES?  A forced
// configuration answers false to the first two (a forced call is not taken by rule).
bool gemm_rule_takes_x3sk(const GemmArgs& p) { return route(p, g_forced).family == D4_GEMM_X3SK; }
bool gemm_rule_takes_v2(const GemmArgs& p) { return g_forced.family < 0 && route(p, g_forced).family == D4_GEMM_V2; }
bool gemm_h2_takes(const GemmArgs& p) { return route(p, g_forced).family == D4_GEMM_H2; }

static int gemm_check(const GemmArgs& p) {
    const bool ta = p.flags & GEMM_TRANS_A, tb = p.flags & GEMM_TRANS_B;
    D4_REQUIRE(p.M >= 0 && p.N > 0 && p.K > 0, "gemm: bad sizes M=%d N=%d K=%d", p.M, p.N, p.K);
    if (p.M == 0) return 0;                      // nothing to run, nothing else to check
    D4_REQUIRE((p.lda % 4) == 0 && (p.ldw % 4) == 0, "gemm: lda/ldw must be multiples of 4 (got %d, %d)", p.lda, p.ldw);
    D4_REQUIRE(((uintptr_t)p.A % 16) == 0 && ((uintptr_t)p.W % 16) == 0, "gemm: operands must be 16-byte aligned");
    D4_REQUIRE(!((p.flags & GEMM_RMS_ROWSCALE) && ta), "gemm: rms rowscale needs a non-transposed A");
    D4_REQUIRE(!((p.flags & GEMM_SWIGLU) && (p.N % 64) != 0), "gemm: swiglu needs N %% 64 == 0 (packed pairs)");
    D4_REQUIRE(!((p.flags & GEMM_SWIGLU) && (ta || tb)), "gemm: swiglu epilogue is forward-only");
    D4_REQUIRE(gemm_rowmap_ok(p), "gemm: bad output row map (Sc=%d lo=%d nr=%d) or an epilogue it does not cover (flags=%d)", p.rm_Sc, p.rm_lo, p.rm_nr, p.flags);
    return 0;
}
// d4_gemm_route: the family gemm() would run the call on under the current hook, after gemm()'s own argument checks
int gemm_route_checked(const GemmArgs& p, int* family) {
    if (int rc = gemm_check(p)) return rc;
    *family = route(p, g_forced).family;
    return 0;
}

int gemm(const GemmArgs& p, hipStream_t stream) {
    std::lock_guard<std::recursive_mutex> lock(g_gemm_mu);
    if (int rc = gemm_check(p)) return rc;
    if (p.M == 0) return 0;
    const GemmRoute r = route(p, g_forced);
    const GemmArgs& q = r.args;
    switch (r.family) {
        case D4_GEMM_H2:
            if (int rc = gemm_rowmap_refused(q, "gemm_h2")) return rc;
            return tuned_launch(kFamilies[FAM_H2], q, stream);
        case D4_GEMM_X3SK: return launch_x3sk(q, stream);
        case D4_GEMM_X3: return tuned_launch(kFamilies[FAM_X3], q, stream);
        case D4_GEMM_BF16A:
            if (int rc = gemm_rowmap_refused(q, "gemm_bf16")) return rc;
            return gemm_bf16a(q, stream);
        case D4_GEMM_BF16: return gemm_bf16(q, stream);             // (refuses the map itself)
        case D4_GEMM_SKINNY: return gemm_skinny(q, stream);
        case D4_GEMM_V2_KSPLIT: return launch_ksplit(q, stream);
        case D4_GEMM_V2: return tuned_launch(kFamilies[FAM_V2], q, stream);
    }
    if (int rc = gemm_rowmap_refused(q, "gemm (first fp32 family)")) return rc;
    return tuned_launch(kFamilies[FAM_TILE], q, stream);
}

// Two independent non-transposed fp32 GEMMs (the attention pool's query and key projections): ONE grid on the LDS-DMA family when the route sends both
// calls to gemm2.hip's kernels anyway (same k order, same bits as two launches of that family), else one after the other.  The pair form keeps two
// limits of its own: nothing forced, and a call that carries mirror weights only below N = 2048.  The tile configuration is the one chosen for the
// larger problem.
int gemm_pair(const GemmArgs& a_in, const GemmArgs& b_in, hipStream_t stream) {
    std::lock_guard<std::recursive_mutex> lock(g_gemm_mu);
    if (int rc = gemm_rowmap_refused(a_in, "gemm_pair")) return rc;
    if (int rc = gemm_rowmap_refused(b_in, "gemm_pair")) return rc;
    const GemmRoute ra = route(a_in, g_forced), rb = route(b_in, g_forced);
    const GemmArgs &a = ra.args, &b = rb.args;
    auto lds_dma = [](const GemmArgs& in, const GemmRoute& r) { return (r.family == D4_GEMM_V2 || r.family == D4_GEMM_V2_KSPLIT) && (!in.Wb || in.N < 2048); };
    if (g_forced.family < 0 && lds_dma(a_in, ra) && lds_dma(b_in, rb) && a.K == b.K && gemm2_pair_applicable(a, b)) {
        const Family& F = kFamilies[FAM_V2];
        const GemmArgs& big = (double)a.M * a.N >= (double)b.M * b.N ? a : b;
        tune_cache_load();
        auto it = F.tuned->find(TuneKey{big.M, big.N, big.K, big.flags, big.batch});
        const int c = it != F.tuned->end() ? it->second : F.heuristic(big);
        if (gemm2_pair_config_ok(c) && gemm2_config_valid(c, a) && gemm2_config_valid(c, b)) {
            GemmArgs both = big;                  // what the per-shape table shows for the launch
            both.M = a.M + b.M; both.batch = 2;
            int bm, bn;
            F.config_tile(c, &bm, &bn);
            return timed_launch(F.first_class + c, both, bm, bn, 2.0 * a.M * a.N * a.K + 2.0 * b.M * b.N * b.K,
                                [&](hipEvent_t ea, hipEvent_t eb) { return gemm2_pair_launch(c, a, b, stream, ea, eb); });
        }
    }
    if (int rc = gemm(a_in, stream)) return rc;
    return gemm(b_in, stream);
}

}  // namespace d4
