// fp32 GEMM, second kernel family: v_mfma_f32_16x16x4_f32 fed by an LDS-DMA ring.
//
//   C[m, n] = epilogue( rowscale[m] * sum_k A[m, k] * W[n, k] )      (both operands K-contiguous, K % 32 == 0; k-tiles of 32 or 16)
//
// Same contract and epilogues as gemm_kernel (gemm.hip: RMSNorm folded as a row scale, bias, SiLU, SiLU-GLU pairing, residual,
// accumulate, row-compacted second output); what differs is how the matrix pipes are fed:
//   * operand tiles go global -> LDS directly (`buffer_load_dwordx4 ... lds`, 1 KB per wave-instruction) into a ring of NS stages
//     with counted `s_waitcnt vmcnt(N)` and one raw `s_barrier` per k-tile, so NS-2 k-tiles are in flight beyond the one being
//     multiplied and the next one (whose first fragments are read from LDS under the current MFMAs: the fragment registers are
//     software-pipelined by half k-tiles), and no VGPR or ds_write is spent on staging.  The LDS image is the plain [rows][32 floats] tile with the 16-byte chunks of a row XOR-swizzled by
//     (row & 7) on the SOURCE address (the DMA writes lane-linear), which makes every ds_read_b128 fragment read conflict-free.
//   * 16x16x4 MFMA (32-cycle issue, 4 accumulator registers per 16x16 sub-tile): block tiles are multiples of 16 rows, so a shape
//     can be cut into exactly 256 / 512 tiles (e.g. 3584 x 512 -> 32 x 8 tiles of 112 x 64: one per CU) instead of the 1.75 tiles per
//     CU a 64 x 64 grid gives.  The operands are swapped (W rows on the MFMA's row side) so that a lane ends up holding four
//     CONSECUTIVE columns of one output row: 16-byte epilogue loads / stores.
// Within this family every configuration walks k in the same order (chunk kq + 4h of each 32-k tile on lane group kq), so all of
// them give the same bits and the choice among them can be made by timing; the family itself is chosen by rule (shape only).
// The folded RMSNorm's row sums use the same canonical order as gemm_kernel (eight running sums per row, one per 16-byte chunk
// position, fused a0^2+a1^2+a2^2+a3^2, then the tree ((0+1)+(2+3))+((4+5)+(6+7))), so the row scale is bit-identical across families.
#include "common.h"
#include <hip/hip_ext.h>
#include "kernels.h"
#include "gemm2_body.h"      // gemm2_body: the tile body (also instantiated by gemm_x3sk.hip's filled form)
#include <stdlib.h>
#include <type_traits>

namespace d4 {

template <int WGM, int WGN, int TM, int TN, int NS, int BK, bool RMS>
__global__ __launch_bounds__(WGM* WGN * 64) void gemm2_kernel(GemmArgs p) {
    gemm2_body<WGM, WGN, TM, TN, NS, BK, RMS>(p, blockIdx.x, blockIdx.y);
}

// the single / batched launch with the row-mapped store (GemmArgs::rm_Sc > 0; plain epilogue only: launch2 checks)
template <int WGM, int WGN, int TM, int TN, int NS, int BK, bool RMS>
__global__ __launch_bounds__(WGM* WGN * 64) void gemm2_rowmap_kernel(GemmArgs p) {
    gemm2_body<WGM, WGN, TM, TN, NS, BK, RMS, true>(p, blockIdx.x, blockIdx.y);
}

// Two independent GEMMs in ONE grid (blocks [0, nblk_a) work on `a`, the rest on `b`): launch ramp and tail are paid once.  Used for the
// attention pool's query and key projections (same K, same epilogue class); each problem keeps its own XCD-aware tile order and the bits of
// every output are those of the separate launches (same body, same k order).
template <int WGM, int WGN, int TM, int TN, int NS, int BK, bool RMS>
__global__ __launch_bounds__(WGM* WGN * 64) void gemm2_pair_kernel(GemmArgs a, GemmArgs b, int nblk_a) {
    const int bid = blockIdx.x;
    if (bid < nblk_a) gemm2_body<WGM, WGN, TM, TN, NS, BK, RMS>(a, bid, 0);
    else gemm2_body<WGM, WGN, TM, TN, NS, BK, RMS>(b, bid - nblk_a, 0);
}

// ---- few rows x long K: the contraction cut FOUR ways inside the workgroup (round 6) ---------------------------------------------------
// The heads' hidden layers at rollout batch (256 x 2048 x 2048, 128 x 4096 x 4096 at config 5) are 512 tiles of 32 x 32 whose 64 k-tiles run one after
// the other: 40 us of k-loop LATENCY at 54 TF/s with half the chip idle.  Here a workgroup of 16 waves owns one 32 x 64 tile and its four wave groups
// (each exactly the 32 x 64 configuration above: 2 x 2 waves, wave tile 16 x 32, its own ring of three stages) each multiply one QUARTER of K; the four
// partial tiles meet in LDS (the rings are free by then) and are summed in group order — a fixed order, nothing crosses between workgroups, no atomics:
// deterministic, but NOT the bits of the family's other configurations (their k order is one chain), so this form is taken by a RULE on the shape
// (gemm2_ksplit_rule), never by the tuner.  Epilogue on the row-contiguous image: bias, SiLU, residual, 16-byte stores.
constexpr int KS_GROUPS = 4, KS_NS = 3, KS_BM = 32, KS_BN = 64, KS_BK = 32;
constexpr int KS_STAGE_F = (KS_BM + KS_BN) * KS_BK;                 // floats per ring stage of one group
constexpr int KS_RING_F = KS_NS * KS_STAGE_F;                       // 9216 floats = 36 KB per group
constexpr int KS_LDP = KS_BN + 4;                                   // partial tile row stride (floats)

__global__ __launch_bounds__(1024) void gemm2_ksplit_kernel(GemmArgs p) {
    constexpr int BK = KS_BK, CH = 8, RPP = 8, BM = KS_BM, BN = KS_BN, NS = KS_NS, LPW = 3, NSLOT = (BM + BN) / RPP;      // 12 pieces per stage, 3 per wave
    extern __shared__ __attribute__((aligned(16))) float smem[];    // [4 groups][3 stages][96 rows][32]; afterwards [4][32][68] partial tiles
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, w = wave & 3, wm = w >> 1, wn = w & 1;
    int bid = blockIdx.x;
    const int nbn = (p.N + BN - 1) / BN, nbm = (p.M + BM - 1) / BM;
    {
        const int nblk = nbm * nbn, nx = 8;
        const int q = nblk / nx, r = nblk % nx, x = bid % nx, o = bid / nx;
        bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + o;
    }
    const int bm0 = (bid / nbn) * BM, bn0 = (bid % nbn) * BN;
    const int rowsA = min(BM, p.M - bm0), rowsB = min(BN, p.N - bn0);
    auto uniform_rsrc = [](const float* base, int64_t bytes) {
        const uint64_t b = reinterpret_cast<uint64_t>(base);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
        const int nb = __builtin_amdgcn_readfirstlane((int)(bytes < 0x7FFFFFFF ? bytes : 0x7FFFFFFF));
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, nb, 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t rsA = uniform_rsrc(p.A + (int64_t)bm0 * p.lda, ((int64_t)(rowsA - 1) * p.lda + p.K) * 4);
    const __amdgpu_buffer_rsrc_t rsB = uniform_rsrc(p.W + (int64_t)bn0 * p.ldw, ((int64_t)(rowsB - 1) * p.ldw + p.K) * 4);
    uint32_t voff[LPW];
    const int prow = lane / CH;
    const int src_chunk = (lane % CH) ^ chunk_swizzle<BK>(prow);
#pragma unroll
    for (int i = 0; i < LPW; ++i) {
        const int slot = w + 4 * i;
        const int r = slot * RPP + prow;
        voff[i] = (uint32_t)((slot * RPP < BM ? r * p.lda : (r - BM) * p.ldw) * 4 + src_chunk * 16);
    }
    float* ring = smem + grp * KS_RING_F;
    // this group's k-tiles: the first (nkt % 4) groups take one more; every group RUNS nk = ceil(nkt / 4) iterations (same barrier sequence) and a
    // group's tile past its share is "loaded" through a zero-record descriptor: zeros in LDS, its MFMAs add nothing
    const int nkt = p.K / BK, nk = (nkt + KS_GROUPS - 1) / KS_GROUPS;
    const int mine = nkt / KS_GROUPS + (grp < nkt % KS_GROUPS ? 1 : 0);
    const int kt0 = grp * (nkt / KS_GROUPS) + min(grp, nkt % KS_GROUPS);
    const __amdgpu_buffer_rsrc_t rs0 = uniform_rsrc(p.A, 0);
#define D4_KS_ISSUE(KT, BUF)                                                                                                      \
    _Pragma("unroll") for (int i_ = 0; i_ < LPW; ++i_) {                                                                           \
        const int slot_ = w + 4 * i_;                                                                                               \
        float* dst_ = ring + (BUF) * KS_STAGE_F + slot_ * 256;                                                                      \
        const __amdgpu_buffer_rsrc_t rs_ = (KT) < mine ? (slot_ * RPP < BM ? rsA : rsB) : rs0;                                    \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_, (lds_void_ptr)dst_, 16, (uint32_t)voff[i_], (kt0 + (KT)) * BK * 4, 0, 0);           \
    }
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int kq = lane >> 4, frow = lane & 15;
    const int foff0 = frow * BK + ((kq ^ chunk_swizzle<BK>(frow)) << 2);
    const int a_base = wm * 16 * BK, b_base = BM * BK + wn * 32 * BK;
    auto wait_allow = [&](int stages) {
        if (stages >= 2) wait_vmcnt<2 * LPW>();
        else if (stages == 1) wait_vmcnt<LPW>();
        else wait_vmcnt<0>();
    };
    f32x4 af[2], bf[2][2];
    auto read_frags = [&](const float* st, int set, int second_half) {
        const int fo = second_half ? (foff0 ^ 16) : foff0;
        af[set] = *reinterpret_cast<const f32x4*>(st + a_base + fo);
        bf[set][0] = *reinterpret_cast<const f32x4*>(st + b_base + fo);
        bf[set][1] = *reinterpret_cast<const f32x4*>(st + b_base + 16 * BK + fo);
    };
#pragma unroll
    for (int st = 0; st < NS - 1; ++st)
        if (st < nk) { D4_KS_ISSUE(st, st) }
    wait_allow(min(NS - 2, nk - 1));
    __builtin_amdgcn_s_barrier();
    read_frags(ring, 0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) {
            wait_allow(min(kt + NS - 2, nk - 1) - (kt + 1));
            __builtin_amdgcn_s_barrier();
            if (kt + NS - 1 < nk) { D4_KS_ISSUE(kt + NS - 1, (kt + NS - 1) % NS) }
        }
        const float* st = ring + (kt % NS) * KS_STAGE_F;
        const float* nxt = ring + ((kt + 1) % NS) * KS_STAGE_F;
        read_frags(st, 1, 1);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[0][j][e], af[0][e], acc[j], 0, 0, 0);
        if (kt + 1 < nk) read_frags(nxt, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[1][j][e], af[1][e], acc[j], 0, 0, 0);
    }
#undef D4_KS_ISSUE
    __syncthreads();                                                 // every group is past its last fragment read: the rings become the partial tiles
    float* part = smem + grp * KS_RING_F;                            // [32][KS_LDP]
#pragma unroll
    for (int j = 0; j < 2; ++j)
        *reinterpret_cast<f32x4*>(part + (wm * 16 + frow) * KS_LDP + wn * 32 + j * 16 + kq * 4) = acc[j];
    __syncthreads();
    if (tid >= BM * BN / 4) return;
    const int row = tid / (BN / 4), c4 = (tid % (BN / 4)) * 4;
    const int gm = bm0 + row, gn = bn0 + c4;
    if (gm >= p.M || gn >= p.N) return;
    f32x4 v = *reinterpret_cast<const f32x4*>(smem + row * KS_LDP + c4);
#pragma unroll
    for (int g = 1; g < KS_GROUPS; ++g) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(smem + g * KS_RING_F + row * KS_LDP + c4);
        v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
    }
    const bool full = gn + 3 < p.N;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!full && gn + e >= p.N) continue;
        float x = v[e];
        if (p.bias) x += p.bias[gn + e];
        if (p.flags & GEMM_SILU) x = siluf(x);
        if (p.R) x += p.R[(int64_t)gm * p.ldr + gn + e];
        v[e] = x;
    }
    float* cp = p.C + (int64_t)gm * p.ldc + gn;
    if (full && (p.ldc % 4) == 0 && ((uintptr_t)p.C % 16) == 0) *reinterpret_cast<f32x4*>(cp) = v;
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (full || gn + e < p.N) cp[e] = v[e];
    }
}

// Measured (tools/gemm2_ksplit_probe.py, profiles/r06_gemm2_ksplit.txt): 256 x 2048 x 2048 27.2 us against 30.8 us for the best tiled configuration (40 us in
// situ), 128 x 4096 x 4096 46 against 55 us; 512 rows lose (51.5 vs 44.8 us) -> at most 256 rows.  Same-box A/B of the whole rollout: cfg 2 181.75 -> 180.32 ms,
// cfg 5 (bf16, B = 128, 6 frames) 78.0 -> 76.9 ms.
// the calls that take it: few rows (at most 256), a long contraction in whole quarters of 32-k tiles, at most ~4 workgroups per CU, plain epilogue
bool gemm2_ksplit_applicable(const GemmArgs& p) {               // what the kernel can run at all (test hook: d4_gemm_force_config(199))
    return gemm2_applicable(p) && p.batch <= 1 && !p.C2 && !p.Wb && !p.Ab && !(p.flags & ~GEMM_SILU) && p.K >= 4 * KS_BK;
}
bool gemm2_ksplit_rule(const GemmArgs& p) {
    if (!gemm2_ksplit_applicable(p)) return false;
    const int M = p.rule_M > 0 ? p.rule_M : p.M;
    const int64_t tiles = (int64_t)cdiv(M, KS_BM) * cdiv(p.N, KS_BN);
    if (M <= 256) return p.K >= 1024 && tiles >= 64 && tiles <= 1024;
    return false;
}

int gemm2_ksplit_launch(const GemmArgs& p, hipStream_t stream, hipEvent_t ea, hipEvent_t eb) {
    if (int rc = gemm_rowmap_refused(p, "gemm2_ksplit")) return rc;
    D4_REQUIRE(gemm2_ksplit_applicable(p), "gemm2_ksplit: call not supported (M=%d N=%d K=%d flags=%d)", p.M, p.N, p.K, p.flags);
    const size_t lds = (size_t)KS_GROUPS * KS_RING_F * sizeof(float);
    static DeviceOnce attr_set;
    if (attr_set.need()) {
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm2_ksplit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set.done();
    }
    const dim3 grid(cdiv(p.M, KS_BM) * cdiv(p.N, KS_BN)), block(1024);
    if (ea) hipExtLaunchKernelGGL(gemm2_ksplit_kernel, grid, block, (uint32_t)lds, stream, ea, eb, 0, p);
    else hipLaunchKernelGGL(gemm2_ksplit_kernel, grid, block, lds, stream, p);
    D4_LAUNCH_CHECK();
    return 0;
}

// ---- configurations -------------------------------------------------------------------------------------------
// name          waves   wave tile   block tile  BK  LDS ring     blocks (waves) / CU
// 64x64         2 x 2     32 x 32     64 x 64   32  3 x 16 KB    3 (12)
// 64x64/s       4 x 1     16 x 64     64 x 64   32  3 x 16 KB    3 (12)   SiLU-GLU capable: a wave spans 64 columns
// 128x64/8      4 x 2     32 x 32    128 x 64   32  3 x 24 KB    2 (16)
// 128x64/s      4 x 1     32 x 64    128 x 64   32  3 x 24 KB    2 (8)    SiLU-GLU capable
// 128x64/k16    4 x 2     32 x 32    128 x 64   16  4 x 12 KB    3 (24)
// 128x128/k16   4 x 2     32 x 64    128 x 128  16  3 x 16 KB    3 (24)   SiLU-GLU capable
// 32x64         2 x 2     16 x 32     32 x 64   32  3 x 12 KB    4 (16)   small GEMMs (< 2 blocks of 64 x 64 per CU): twice the blocks
// 32x64/s       2 x 1     16 x 64     32 x 64   32  3 x 12 KB    4 (8)    SiLU-GLU capable
// Measured on the engine's shapes (tools/gemm2_bench.py, profiles/r02_gemm_families.txt) and dropped: 128x128 with 4 or 8 waves and
// 256x128 at either BK (one or two blocks per CU leave every barrier exposed: 1.3-3x slower on the N <= 512 shapes), 112x64 /
// 128x64 with 4 waves, 64x64 with a 4-deep ring or at BK = 16, 32x128 (SiLU-GLU capable) and 32x64 at BK = 16 (never ahead of the forms
// above).  Waves per CU is what pays: the 32-row tiles added last (4-6 blocks per CU) win every N <= 512 shape.
enum { V2_64x64 = 0, V2_64x64_s, V2_128x64_8, V2_128x64_s, V2_128x64_k16, V2_128x128_k16, V2_32x64, V2_32x64_s, V2_32x32, V2_64x32, V2_N };
static const char* const kV2Kernel[V2_N] = {"gemm2_kernel<2, 2, 2, 2, 3, 32", "gemm2_kernel<4, 1, 1, 4, 3, 32", "gemm2_kernel<4, 2, 2, 2, 3, 32", "gemm2_kernel<4, 1, 2, 4, 3, 32",
                                            "gemm2_kernel<4, 2, 2, 2, 4, 16", "gemm2_kernel<4, 2, 2, 4, 3, 16", "gemm2_kernel<2, 2, 1, 2, 3, 32", "gemm2_kernel<2, 1, 1, 4, 3, 32", "gemm2_kernel<2, 2, 1, 1, 3, 32", "gemm2_kernel<4, 1, 1, 2, 3, 32"};
static const int kV2BM[V2_N] = {64, 64, 128, 128, 128, 128, 32, 32, 32, 64}, kV2BN[V2_N] = {64, 64, 64, 64, 64, 128, 64, 64, 32, 32};

int gemm2_configs() { return V2_N; }
const char* gemm2_config_name(int c) { return c >= 0 && c < V2_N ? kV2Kernel[c] : ""; }
void gemm2_config_tile(int c, int* bm, int* bn) { *bm = kV2BM[c]; *bn = kV2BN[c]; }

bool gemm2_applicable(const GemmArgs& p) {
    return !(p.flags & (GEMM_TRANS_A | GEMM_TRANS_B)) && (p.K % 32) == 0 && (p.lda % 4) == 0 && (p.ldw % 4) == 0 && p.M >= 1;
}

bool gemm2_config_valid(int c, const GemmArgs& p) {
    if (c < 0 || c >= V2_N || !gemm2_applicable(p)) return false;
    if (p.flags & GEMM_SWIGLU) return c == V2_64x64_s || c == V2_128x64_s || c == V2_128x128_k16 || c == V2_32x64_s;
    return true;
}

// Static choice, for a shape that cannot be timed: 64x64 with three blocks per CU or its SiLU-GLU capable form — the best or within a few per cent of it on
// every shape measured; the timed choice refines this where a call can be repeated
int gemm2_heuristic(const GemmArgs& p) { return (p.flags & GEMM_SWIGLU) ? V2_64x64_s : V2_64x64; }

template <int WGM, int WGN, int TM, int TN, int NS, int BK>
static int launch2(const GemmArgs& p, hipStream_t stream, hipEvent_t ea, hipEvent_t eb) {
    constexpr int BM = WGM * TM * 16, BN = WGN * TN * 16;
    const size_t lds = (size_t)(NS * (BM + BN) * BK + BM) * sizeof(float);
    const bool rms = (p.flags & GEMM_RMS_ROWSCALE) != 0, rmap = p.rm_Sc > 0;
    D4_REQUIRE(gemm_rowmap_ok(p), "gemm2: bad output row map (Sc=%d lo=%d nr=%d) or an epilogue it does not cover (flags=%d)", p.rm_Sc, p.rm_lo, p.rm_nr, p.flags);
    auto k = rmap ? (rms ? gemm2_rowmap_kernel<WGM, WGN, TM, TN, NS, BK, true> : gemm2_rowmap_kernel<WGM, WGN, TM, TN, NS, BK, false>)
                  : (rms ? gemm2_kernel<WGM, WGN, TM, TN, NS, BK, true> : gemm2_kernel<WGM, WGN, TM, TN, NS, BK, false>);
    static DeviceOnce attr_set[4];
    if (attr_set[2 * rmap + rms].need()) {
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set[2 * rmap + rms].done();
    }
    const dim3 grid(cdiv(p.M, BM) * cdiv(p.N, BN), p.batch > 0 ? p.batch : 1), block(WGM * WGN * 64);
    if (ea) hipExtLaunchKernelGGL(k, grid, block, (uint32_t)lds, stream, ea, eb, 0, p);
    else hipLaunchKernelGGL(k, grid, block, lds, stream, p);
    D4_LAUNCH_CHECK();
    return 0;
}

template <int WGM, int WGN, int TM, int TN, int NS, int BK>
static int launch2_pair(const GemmArgs& a, const GemmArgs& b, hipStream_t stream, hipEvent_t ea, hipEvent_t eb) {
    constexpr int BM = WGM * TM * 16, BN = WGN * TN * 16;
    const size_t lds = (size_t)(NS * (BM + BN) * BK + BM) * sizeof(float);
    const bool rms = (a.flags & GEMM_RMS_ROWSCALE) != 0;
    auto k = rms ? gemm2_pair_kernel<WGM, WGN, TM, TN, NS, BK, true> : gemm2_pair_kernel<WGM, WGN, TM, TN, NS, BK, false>;
    static DeviceOnce attr_set[2];
    if (attr_set[rms].need()) {
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set[rms].done();
    }
    const int na = cdiv(a.M, BM) * cdiv(a.N, BN), nb = cdiv(b.M, BM) * cdiv(b.N, BN);
    const dim3 grid(na + nb), block(WGM * WGN * 64);
    if (ea) hipExtLaunchKernelGGL(k, grid, block, (uint32_t)lds, stream, ea, eb, 0, a, b, na);
    else hipLaunchKernelGGL(k, grid, block, lds, stream, a, b, na);
    D4_LAUNCH_CHECK();
    return 0;
}

bool gemm2_pair_config_ok(int c) { return c == V2_64x64 || c == V2_128x64_8 || c == V2_128x64_k16 || c == V2_32x64 || c == V2_32x32 || c == V2_64x32; }

bool gemm2_pair_applicable(const GemmArgs& a, const GemmArgs& b) {
    const int fa = a.flags & ~GEMM_RMS_ROWSCALE, fb = b.flags & ~GEMM_RMS_ROWSCALE;
    return gemm2_applicable(a) && gemm2_applicable(b) && a.batch <= 1 && b.batch <= 1 && ((a.flags ^ b.flags) & GEMM_RMS_ROWSCALE) == 0 &&
           !(fa & GEMM_SWIGLU) && !(fb & GEMM_SWIGLU) && a.M > 0 && b.M > 0;
}

int gemm2_pair_launch(int c, const GemmArgs& a, const GemmArgs& b, hipStream_t stream, hipEvent_t ea, hipEvent_t eb) {
    if (int rc = gemm_rowmap_refused(a, "gemm2 pair")) return rc;
    if (int rc = gemm_rowmap_refused(b, "gemm2 pair")) return rc;
    D4_REQUIRE(gemm2_pair_applicable(a, b) && gemm2_config_valid(c, a) && gemm2_config_valid(c, b), "gemm2 pair: configuration %d is not valid for these calls", c);
    switch (c) {
        case V2_64x64: return launch2_pair<2, 2, 2, 2, 3, 32>(a, b, stream, ea, eb);
        case V2_128x64_8: return launch2_pair<4, 2, 2, 2, 3, 32>(a, b, stream, ea, eb);
        case V2_128x64_k16: return launch2_pair<4, 2, 2, 2, 4, 16>(a, b, stream, ea, eb);
        case V2_32x64: return launch2_pair<2, 2, 1, 2, 3, 32>(a, b, stream, ea, eb);
        case V2_32x32: return launch2_pair<2, 2, 1, 1, 3, 32>(a, b, stream, ea, eb);
        case V2_64x32: return launch2_pair<4, 1, 1, 2, 3, 32>(a, b, stream, ea, eb);
    }
    return 2;       // the remaining configurations are not instantiated in pair form
}

int gemm2_launch(int c, const GemmArgs& p, hipStream_t stream, hipEvent_t ea, hipEvent_t eb) {
    D4_REQUIRE(gemm2_config_valid(c, p), "gemm2: configuration %d is not valid for this call", c);
    switch (c) {
        case V2_64x64: return launch2<2, 2, 2, 2, 3, 32>(p, stream, ea, eb);
        case V2_64x64_s: return launch2<4, 1, 1, 4, 3, 32>(p, stream, ea, eb);
        case V2_128x64_8: return launch2<4, 2, 2, 2, 3, 32>(p, stream, ea, eb);
        case V2_128x64_s: return launch2<4, 1, 2, 4, 3, 32>(p, stream, ea, eb);
        case V2_128x64_k16: return launch2<4, 2, 2, 2, 4, 16>(p, stream, ea, eb);
        case V2_128x128_k16: return launch2<4, 2, 2, 4, 3, 16>(p, stream, ea, eb);
        case V2_32x64: return launch2<2, 2, 1, 2, 3, 32>(p, stream, ea, eb);
        case V2_32x64_s: return launch2<2, 1, 1, 4, 3, 32>(p, stream, ea, eb);
        case V2_32x32: return launch2<2, 2, 1, 1, 3, 32>(p, stream, ea, eb);
        case V2_64x32: return launch2<4, 1, 1, 2, 3, 32>(p, stream, ea, eb);
    }
    return 2;
}

}  // namespace d4
