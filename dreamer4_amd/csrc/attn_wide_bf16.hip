// Wide-frame attention core of the inference path (attn_wide.h holds the kernel's skeleton) with both products on the bf16 matrix pipe
// (opt-in: SmallAttnArgs::wide == 2): ProdBf16 and the kernel wide_attn_bf16_kernel<DH>; the semantics, arguments, refusals and grid of
// attn_wide_mfma.hip's wide_attn_kernel<DH>.
//
// Arithmetic: k' = k / max(|k|, 1e-12) (gamma + 1) sqrt(dh) and v' = v + sigmoid(mix) (vres - v) in fp32, then rounded to bf16 (nearest
// even) on their way into LDS; q rounded to bf16 in registers; S = q^ k^'^T on v_mfma_f32_16x16x32_bf16 with fp32 accumulate; scale,
// soft clamp, special-token rule and the online softmax per 64-key tile in fp32; p = exp(s - m_running) rounded to bf16 for p^ v^' (same
// instruction), the row sum from the unrounded p; belief projection (the query's own fp32 v' row, re-read from global memory), head gate
// and output in fp32.  Head dim 16: the 32-deep contraction of Q K^T is zero-padded (the lanes of k = 16 .. 31 carry a zero q fragment).
//
//   The eight registers of S^T sub-tiles 2 u, 2 u + 1 of a lane, packed to bf16, ARE the A fragment of P V' over the 32 keys of half u — in
//   the key order slot 8 kq + j <-> key 16 (j >> 2) + 4 kq + (j & 3) of the half.  V' is kept transposed in that slot order.
//
// LDS (16 KB at DH 64, static):
//   Ks [64 keys][DH] bf16, natural feature order, in 16-byte chunks (8 features); chunk c of row r sits at chunk c ^ f(r) with
//      f(r) = (r >> 1) & 7 (DH 64: 8 chunks), (-(r >> 2)) & 3 (DH 32: 4 chunks), 0 (DH 16: 2 chunks).
//   Vt [DH features][64 slots] bf16 (128-byte rows = 8 chunks of 8 slots), chunk c of row r at c ^ ((r >> 1) & 7) ^ ((r & 1) << 2).
//   Reads are one ds_read_b128 per fragment: lane (tok, kq) reads chunk 4 s + kq of row 16 kt + tok.  With the 16-lane service groups of
//   ds_read_b128 ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) and the bank (byte / 4) % 64, every group's 16 lanes cover
//   the 16 16-byte slots of the 256-byte bank row exactly once for each DH: conflict-free (computed from the bank rule, not measured).
//   Writes are ds_write_b64 (groups of 16 consecutive lanes, bank (byte / 4) % 32): in Ks two rows share a bank pair at DH 64 and 32 (2-way), four
//   at DH 16 (4-way, one store per tile); Vt's store is 2-way at every DH (computed, not measured).  The value tile is transposed in registers
//   first: the four lanes of a quad (keys 4 g .. 4 g + 3, four features each) exchange bf16 pairs by two DPP quad permutes, after which a
//   lane holds ONE feature of the quad's four keys = four consecutive slots = one 8-byte store.
#include "attn_wide.h"

namespace d4 {

namespace {

typedef __bf16 wb_b8 __attribute__((ext_vector_type(8)));
typedef __bf16 wb_b2 __attribute__((ext_vector_type(2)));
typedef uint32_t wb_u2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {      // (a in the low half): v_cvt_pk_bf16_f32, round to nearest even
    wb_b2 o;
    o[0] = (__bf16)a; o[1] = (__bf16)b;
    return __builtin_bit_cast(uint32_t, o);
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
template <int DH>
__device__ __forceinline__ int ks_swz(int row) {         // Ks: the chunk swizzle f(row) of the header
    return DH == 64 ? ((row >> 1) & 7) : DH == 32 ? ((-(row >> 2)) & 3) : 0;
}

__device__ __forceinline__ int vt_swz(int row) {         // Vt: the same for its 128-byte rows (bit 0 of the row spreads the 8-byte stores over all banks)
    return ((row >> 1) & 7) ^ ((row & 1) << 2);
}

template <int DH>
struct ProdBf16 {
    static constexpr int NS = DH / 16;                   // float4 per operand and lane in staging; 16-feature output tiles
    static constexpr int KS = DH == 64 ? 2 : 1;          // 32-deep contraction steps of Q K^T
    struct __attribute__((aligned(16))) Lds { uint16_t Ks[WIDE_WT * DH], Vt[DH * WIDE_WT]; };
    struct QFrag { wb_b8 qf[KS]; };                      // B fragments of Q K^T: q[i][32 s + 8 kq .. + 7] as bf16 (DH 16: the lanes kq >= 2 pad the contraction with zeros)

    static __device__ __forceinline__ void load_q(QFrag& q, const float* qrow, bool ok, int kq) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const bool qok = ok && (DH > 16 || kq < 2);
        qrow += DH > 16 ? 8 * kq : 8 * (kq & 1);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const f32x4 a = qok ? *reinterpret_cast<const f32x4*>(qrow + 32 * s) : zero;
            const f32x4 b = qok ? *reinterpret_cast<const f32x4*>(qrow + 32 * s + 4) : zero;
#pragma unroll
            for (int e = 0; e < 4; ++e) { q.qf[s][e] = (__bf16)a[e]; q.qf[s][4 + e] = (__bf16)b[e]; }
        }
    }
    static __device__ __forceinline__ void stage(Lds& lds, int jl, int w, int tok, int kq, const f32x4 (&k4)[NS], const f32x4 (&v4)[NS], float nrm, const f32x4 (&gk)[NS]) {
        const int c = tok & 3, tg = tok >> 2;                              // (the whole wave is here: the quad exchanges below see every lane)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            // k': features 16 s + 4 kq .. + 3 of key jl = half (kq & 1) of chunk 2 s + (kq >> 1) of row jl
            wb_u2 kn;
            kn[0] = pk_bf16(k4[s][0] / nrm * gk[s][0], k4[s][1] / nrm * gk[s][1]);
            kn[1] = pk_bf16(k4[s][2] / nrm * gk[s][2], k4[s][3] / nrm * gk[s][3]);
            *reinterpret_cast<wb_u2*>(lds.Ks + jl * DH + 8 * ((2 * s + (kq >> 1)) ^ ks_swz<DH>(jl)) + 4 * (kq & 1)) = kn;
            // v': 4 keys x 4 features of a quad, transposed: lane c ends with feature 16 s + 4 kq + c of keys 4 tg .. 4 tg + 3
            const uint32_t d0 = pk_bf16(v4[s][0], v4[s][1]), d1 = pk_bf16(v4[s][2], v4[s][3]);
            const bool up = (c & 2) != 0, odd = (c & 1) != 0;
            const uint32_t got = dpp_u<0x4E>(up ? d0 : d1);                // quad_perm [2,3,0,1]: lane c ^ 2
            const uint32_t x0 = up ? got : d0, x1 = up ? d1 : got;          // features 2 (c >> 1), + 1 of keys (c & 1), (c & 1) + 2
            const uint32_t lo = (x0 & 0xffffu) | (x1 << 16), hi = (x0 >> 16) | (x1 & 0xffff0000u);
            const uint32_t oth = dpp_u<0xB1>(odd ? lo : hi);                // quad_perm [1,0,3,2]: lane c ^ 1
            wb_u2 vt;                                                       // feature c of keys 0, 1 | 2, 3 of the quad
            vt[0] = odd ? ((oth & 0xffffu) | (x0 & 0xffff0000u)) : ((x0 & 0xffffu) | (oth << 16));
            vt[1] = odd ? ((oth >> 16) | (x1 & 0xffff0000u)) : ((x1 & 0xffffu) | (oth & 0xffff0000u));
            // slots 32 (w >> 1) + 8 tg + 4 (w & 1) .. + 3 = half (w & 1) of chunk 4 (w >> 1) + tg of row 16 s + 4 kq + c
            const int row = 16 * s + 4 * kq + c;
            *reinterpret_cast<wb_u2*>(lds.Vt + row * WIDE_WT + 8 * ((4 * (w >> 1) + tg) ^ vt_swz(row)) + 4 * (w & 1)) = vt;
        }
    }
    static __device__ __forceinline__ f32x4 scores(const Lds& lds, int kt, int tok, int kq, const QFrag& q) {
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
        const int row = 16 * kt + tok;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int ch = DH > 16 ? 4 * s + kq : (kq & 1);
            const wb_b8 kf = *reinterpret_cast<const wb_b8*>(lds.Ks + row * DH + 8 * (ch ^ ks_swz<DH>(row)));
            st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, q.qf[s], st, 0, 0, 0);
        }
        return st;
    }
    static __device__ __forceinline__ void pv(const Lds& lds, const f32x4 (&pr)[4], f32x4 (&o)[NS], int j0, int jmax, int tok, int kq) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (j0 + 32 * u > jmax) continue;               // (wave-uniform; a skipped second sub-tile of a half has p = 0)
            wb_b8 pa;                                       // A fragment: slot 8 kq + e <-> key 4 kq + e of sub-tile 2 u, slot 8 kq + 4 + e of 2 u + 1
#pragma unroll
            for (int e = 0; e < 4; ++e) { pa[e] = (__bf16)pr[2 * u][e]; pa[4 + e] = (__bf16)pr[2 * u + 1][e]; }
#pragma unroll
            for (int t = 0; t < NS; ++t) {
                const int row = 16 * t + tok;
                const wb_b8 vf = *reinterpret_cast<const wb_b8*>(lds.Vt + row * WIDE_WT + 8 * ((4 * u + kq) ^ vt_swz(row)));
                o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vf, o[t], 0, 0, 0);
            }
        }
    }
};

template <int DH>
__global__ __launch_bounds__(256) void wide_attn_bf16_kernel(SmallAttnArgs p) { wide_attn_body<DH, ProdBf16<DH>>(p); }

}  // namespace

// Launches on arguments wide_attn (attn_wide_mfma.hip) has validated; *form names the kernel that ran.  `out_b` (optional) is written by the kernel's epilogue.
int wide_attn_bf16_launch(const SmallAttnArgs& p, hipStream_t stream, const char** form) {
    D4_WIDE_ATTN_LAUNCH(wide_attn_bf16_kernel, p, stream, form);
    return 0;
}

}  // namespace d4
