// Wide-frame attention core of the inference path (attn_wide.h holds the kernel's skeleton) with fp32 products: ProdF32, the kernel
// wide_attn_kernel<DH>, and the host entry of both product forms with all validation.
//
// Both products run on v_mfma_f32_16x16x4_f32.  LDS: Ks / Vs [64 keys][DH + 4] floats, the prepared rows in natural feature order; with rows
// of DH + 4 floats the float4 reads of K (16 rows per 16 lanes) and the scalar reads of V (4 rows x 16 columns) are bank-conflict free.
// Static LDS: 2 x 64 x (DH + 4) floats = 34 KB at DH 64.
#include "attn_wide.h"

namespace d4 {

int g_small_attn_wide = 0;

namespace {

template <int DH>
struct ProdF32 {
    static constexpr int NS = DH / 16, LD = DH + 4;
    struct __attribute__((aligned(16))) Lds { float Ks[WIDE_WT * LD], Vs[WIDE_WT * LD]; };
    struct QFrag { f32x4 q4[NS]; };                       // B fragments of Q K^T: q[i][16 s + 4 kq .. + 3]

    static __device__ __forceinline__ void load_q(QFrag& q, const float* qrow, bool ok, int kq) {
#pragma unroll
        for (int s = 0; s < NS; ++s) q.q4[s] = ok ? *reinterpret_cast<const f32x4*>(qrow + 16 * s + 4 * kq) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    static __device__ __forceinline__ void stage(Lds& lds, int jl, int, int, int kq, const f32x4 (&k4)[NS], const f32x4 (&v4)[NS], float nrm, const f32x4 (&gk)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            f32x4 kn;
#pragma unroll
            for (int e = 0; e < 4; ++e) kn[e] = k4[s][e] / nrm * gk[s][e];
            *reinterpret_cast<f32x4*>(lds.Ks + jl * LD + 16 * s + 4 * kq) = kn;
            *reinterpret_cast<f32x4*>(lds.Vs + jl * LD + 16 * s + 4 * kq) = v4[s];
        }
    }
    static __device__ __forceinline__ f32x4 scores(const Lds& lds, int kt, int tok, int kq, const QFrag& q) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const f32x4 k4 = *reinterpret_cast<const f32x4*>(lds.Ks + (16 * kt + tok) * LD + 16 * s + 4 * kq);
#pragma unroll
            for (int e = 0; e < 4; ++e) st = __builtin_amdgcn_mfma_f32_16x16x4f32(k4[e], q.q4[s][e], st, 0, 0, 0);
        }
        return st;
    }
    static __device__ __forceinline__ void pv(const Lds& lds, const f32x4 (&pr)[4], f32x4 (&o)[NS], int j0, int jmax, int tok, int kq) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (j0 + 16 * kt > jmax) continue;              // (wave-uniform)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* vrow = lds.Vs + (16 * kt + 4 * kq + e) * LD + tok;
#pragma unroll
                for (int t = 0; t < NS; ++t) o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[kt][e], vrow[16 * t], o[t], 0, 0, 0);
            }
        }
    }
};

template <int DH>
__global__ __launch_bounds__(256) void wide_attn_kernel(SmallAttnArgs p) { wide_attn_body<DH, ProdF32<DH>>(p); }

}  // namespace

// Validates, then launches; *form names the kernel that ran (nullptr: nothing to do).  `out_b` (optional) is written by the kernel's epilogue.
int wide_attn(const SmallAttnArgs& p, hipStream_t stream, const char** form) {
    *form = nullptr;
    D4_REQUIRE(p.nq >= 1 && p.nk >= 1 && p.nq <= WIDE_ATTN_MAX && p.nk <= WIDE_ATTN_MAX,
               "wide attention: %d queries x %d keys out of range [1,%d] per side", p.nq, p.nk, WIDE_ATTN_MAX);
    D4_REQUIRE(p.dh == 16 || p.dh == 32 || p.dh == 64, "wide attention: head dim %d (16, 32 or 64)", p.dh);
    D4_REQUIRE(!p.belief || p.nq == p.nk, "wide attention: belief needs self attention (nq=%d, nk=%d)", p.nq, p.nk);
    D4_REQUIRE(p.q_lo == 0 && p.q_hi == 0, "wide attention: the query restriction (q_lo=%d, q_hi=%d) is not implemented", p.q_lo, p.q_hi);
    // (the specials are the last items of both sides, and an ordinary query must see at least one key: key 0 opens every online softmax)
    D4_REQUIRE(p.mask_special >= 0 && p.mask_special <= (p.nq < p.nk ? p.nq : p.nk) && (p.mask_special >= p.nq || p.mask_special < p.nk),
               "wide attention: %d special items with %d queries x %d keys", p.mask_special, p.nq, p.nk);
    D4_REQUIRE(p.out != nullptr && p.q && p.k && p.v && p.k_gamma && (!p.vres || p.mix), "wide attention: null operand");
    auto al4 = [](const void* q, int64_t a, int64_t b) { return ((uintptr_t)q % 16) == 0 && (a % 4) == 0 && (b % 4) == 0; };
    // (the value residual may be misaligned: the kernel then reads it by floats)
    D4_REQUIRE(al4(p.q, p.q_group_stride, p.q_item_stride) && al4(p.k, p.k_group_stride, p.k_item_stride) && al4(p.v, p.v_group_stride, p.v_item_stride) &&
               al4(p.out, p.o_group_stride, p.o_item_stride), "wide attention: q / k / v / output rows must be 16-byte aligned");
    const int64_t units = (int64_t)p.groups * p.heads;
    D4_REQUIRE(p.groups >= 0 && p.heads >= 0 && units <= 0x7fffffff, "wide attention: %d groups x %d heads", p.groups, p.heads);
    if (units == 0) return 0;
    if (p.wide == 2) return wide_attn_bf16_launch(p, stream, form);      // bf16 products (attn_wide_bf16.hip): the same validation, grid and refusals
    D4_WIDE_ATTN_LAUNCH(wide_attn_kernel, p, stream, form);
    return 0;
}

}  // namespace d4
