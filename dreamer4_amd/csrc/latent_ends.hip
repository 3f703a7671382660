// The latent-token ends of a dynamics trunk evaluation, one workgroup per frame.
//
// Both learned-query pools around the trunk work on a few rows per frame (n <= 32 latent tokens, ns <= 16 spatial tokens) and used to be a tiled GEMM
// and a one-wave-per-(frame, head) attention launch each, at their latency floor, with the intermediate (K | V of the latents: 33.5 MB at 256
// frames; the pooled rows: 16.8 MB) written to HBM and read straight back.  Here the pair is one kernel and the intermediate stays on chip:
//
//   lqap_in_kernel    latents [n][dl] of a frame -> K | V of head h on wave h (v_mfma_f32_16x16x4_f32, the weight tile on the row side: the lane that
//                     ends up with out[token l & 15][16 s + 4 (l >> 4) .. + 3] is the lane attn_mfma_unit wants that fragment on) -> the attention of
//                     the ns learned queries over them (attn_mfma_unit with a register operand source)                          D4:7168
//   lqap_out_kernel   attention of the n learned queries over the frame's ns keys (attn_mfma_unit, one head per wave) into LDS -> output projection
//                     [n][512] x [dl][512]^T, every 16 x 16 output tile summed over the whole K on ONE wave                  D4:7251
//
// BIT-IDENTICAL to the launches they replace where those run on the LDS-DMA GEMM family (gemm2.hip): the same MFMA, k = 16 s + 4 kq + e in MFMA e of
// k-step s on one accumulator chain from zero, the folded RMSNorm's row sums in the canonical order (one running sum per 16-byte chunk position of a
// 32-k tile, a0^2 + a1^2 + a2^2 + a3^2 fused from the left, then ((0+1)+(2+3))+((4+5)+(6+7))), the row scale multiplied onto the finished sum.
#include "attn_mfma.h"
#include "prof.h"
#include <hip/hip_ext.h>

namespace d4 {

constexpr int LE_NW = 8;               // waves per workgroup = heads

// K | V rows of one head from the frame's latents, computed where attn_mfma_unit wants them.  The call for key tile 0 computes every tile: the weight
// fragments are loaded once per k-step and feed the KT tiles' independent accumulator chains; the later tiles wait in registers for their call.
template <int KT>
struct LqapInKv {
    const float* lat;                  // this frame's latents [n][ldl]
    const float* w;                    // lin_kv_w [2 * heads * 64][ldw]: K rows then V rows
    int ldl, ldw, dl, h, heads, lane;
    float eps;
    f32x4 kk[KT][4], vv[KT][4];        // tile t's rows, rows past nk as zeros (filled by the call for tile 0)
    __device__ __forceinline__ void operator()(const SmallAttnArgs& p, int, int kt, int, bool, int, f32x4 (&k4)[4], f32x4 (&v4)[4]) {
        if (kt == 0) compute(p.nk);
#pragma unroll
        for (int t = 0; t < KT; ++t)
            if (t == kt) {
#pragma unroll
                for (int s = 0; s < 4; ++s) { k4[s] = kk[t][s]; v4[s] = vv[t][s]; }
            }
    }
    __device__ __forceinline__ void compute(int nk) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const int tok = lane & 15, kq = lane >> 4;
        const float* wk = w + (int64_t)(h * 64 + tok) * ldw + 4 * kq;
        const float* wv = wk + (int64_t)heads * 64 * ldw;
        float ssq[KT][2];                                           // chunk positions kq (even k-steps) and kq + 4 (odd k-steps) of the 32-k tiles
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            ssq[t][0] = 0.f; ssq[t][1] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) { kk[t][s] = zero; vv[t][s] = zero; }
        }
        for (int ks = 0; ks < dl / 16; ks += 2) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int k0 = 16 * (ks + half);
                f32x4 a[KT], bk[4], bv[4];
#pragma unroll
                for (int t = 0; t < KT; ++t) {
                    const int j = 16 * t + tok;
                    a[t] = j < nk ? *reinterpret_cast<const f32x4*>(lat + (int64_t)j * ldl + 4 * kq + k0) : zero;
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    bk[s] = *reinterpret_cast<const f32x4*>(wk + (int64_t)16 * s * ldw + k0);
                    bv[s] = *reinterpret_cast<const f32x4*>(wv + (int64_t)16 * s * ldw + k0);
                }
#pragma unroll
                for (int t = 0; t < KT; ++t)
                    ssq[t][half] = ssq[t][half] + __builtin_fmaf(a[t][3], a[t][3], __builtin_fmaf(a[t][2], a[t][2], __builtin_fmaf(a[t][1], a[t][1], a[t][0] * a[t][0])));
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int t = 0; t < KT; ++t) {
                            kk[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(bk[s][e], a[t][e], kk[t][s], 0, 0, 0);
                            vv[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[s][e], a[t][e], vv[t][s], 0, 0, 0);
                        }
            }
        }
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            // row sum of squares of token 16 t + tok: (0+1)+(2+3) over the lane groups, then (0123) + (4567)
            float s0 = ssq[t][0], s1 = ssq[t][1];
            s0 += __shfl_xor(s0, 16); s0 += __shfl_xor(s0, 32);
            s1 += __shfl_xor(s1, 16); s1 += __shfl_xor(s1, 32);
            const float rs = rsqrtf((s0 + s1) / (float)dl + eps);
            const bool ok = 16 * t + tok < nk;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    kk[t][s][e] = ok ? kk[t][s][e] * rs : 0.f;
                    vv[t][s][e] = ok ? vv[t][s][e] * rs : 0.f;
                }
        }
    }
};

struct LqapInArgs {
    const float* lat; int ldl;         // [frames * n][ldl]
    const float* w; int ldw;           // [2 * heads * 64][ldw]
    int dl;
    float eps;
};

template <int KT>
__global__ __launch_bounds__(LE_NW * 64) void lqap_in_kernel(SmallAttnArgs sa, LqapInArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem_li[];
    float* Vs_all = smem_li;                                        // [waves][KT * 16][SM_LDV]
    float* kinv_all = Vs_all + LE_NW * KT * 16 * SM_LDV;            // [waves][KT * 16]
    float* vinv_all = kinv_all + LE_NW * KT * 16;
    const int lane = threadIdx.x & 63, h = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = blockIdx.x;
    if (h >= sa.heads) return;
    float* op = sa.out + g * sa.o_group_stride + h * 64;
    const int64_t ois = sa.o_item_stride;
    LqapInKv<KT> kv;
    kv.lat = a.lat + (int64_t)g * sa.nk * a.ldl; kv.w = a.w; kv.ldl = a.ldl; kv.ldw = a.ldw; kv.dl = a.dl; kv.h = h; kv.heads = sa.heads; kv.lane = lane; kv.eps = a.eps;
    attn_mfma_unit<1, KT>(sa, g, h, lane, Vs_all + h * KT * 16 * SM_LDV, kinv_all + h * KT * 16, vinv_all + h * KT * 16,
                          [&](int orank, int t, int tok, float v) { op[(int64_t)orank * ois + 16 * t + tok] = v; }, kv);
}

bool lqap_in_applicable(int heads, int dh, int n, int ns, int dl) {
    return heads == LE_NW && dh == 64 && n >= 1 && n <= 32 && ns >= 1 && ns <= 16 && dl >= 32 && dl % 32 == 0 && dl <= 256;
}

int lqap_in(const float* latents, int ldl, const float* w_kv, int ldw, const float* q, const float* gate, const float* k_gamma, float* out, int frames,
            int heads, int n, int ns, int dl, float eps, hipStream_t s) {
    auto al16 = [](const void* p) { return ((uintptr_t)p % 16) == 0; };
    D4_REQUIRE(lqap_in_applicable(heads, 64, n, ns, dl) && frames >= 0 && ldl >= dl && ldw >= dl && ldl % 4 == 0 && ldw % 4 == 0 && al16(latents) && al16(w_kv) &&
               al16(q) && al16(k_gamma) && al16(out) && gate, "lqap_in: call not supported (8 heads x 64, n <= 32, ns <= 16, dl %% 32 == 0, 16-byte aligned rows)");
    if (frames == 0) return 0;
    const int hd = heads * 64;
    SmallAttnArgs sa{};
    sa.q = q; sa.q_group_stride = 0; sa.q_item_stride = hd;
    sa.gate = gate; sa.g_group_stride = 0; sa.g_item_stride = heads;
    sa.k_gamma = k_gamma;
    sa.out = out; sa.o_group_stride = (int64_t)ns * hd; sa.o_item_stride = hd;
    sa.groups = frames; sa.heads = heads; sa.nq = ns; sa.nk = n;
    LqapInArgs a{latents, ldl, w_kv, ldw, dl, eps};
    // algorithmic bytes: the latents read once, the pooled rows written once, queries once (+ the projection weights once per XCD)
    const double bytes = 4.0 * ((double)frames * n * dl + (double)frames * ns * hd + (double)ns * hd + 8.0 * 2.0 * hd * dl);
    const double flops = 2.0 * frames * n * 2.0 * hd * dl;
    const int KT = n <= 16 ? 1 : 2;
    const size_t lds = (size_t)LE_NW * KT * 16 * (SM_LDV + 2) * sizeof(float);
    static DeviceOnce attr_set;
    if (attr_set.need()) {
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lqap_in_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LE_NW * 2 * 16 * (SM_LDV + 2) * sizeof(float))));
        attr_set.done();
    }
    if (KT == 1) D4_GLUE_LAUNCH_F(GL_LATENT_ENDS, bytes, flops, (lqap_in_kernel<1>), dim3(frames), dim3(LE_NW * 64), lds, s, sa, a);
    else D4_GLUE_LAUNCH_F(GL_LATENT_ENDS, bytes, flops, (lqap_in_kernel<2>), dim3(frames), dim3(LE_NW * 64), lds, s, sa, a);
    D4_LAUNCH_CHECK();
    return 0;
}

// ---- spatial tokens -> latent prediction -------------------------------------------------------------------------------------------------
struct LqapOutArgs {
    const float* w; int ldw;           // lout_w [dl][ldw], K = heads * 64
    float* pred; int ldp;              // [frames * n][ldp]
    int dl;
};

template <int QT>
__global__ __launch_bounds__(LE_NW * 64) void lqap_out_kernel(SmallAttnArgs sa, LqapOutArgs a) {
    constexpr int HD = LE_NW * 64, LDA = HD + 4;
    extern __shared__ __attribute__((aligned(16))) float smem_lo[];
    float* As = smem_lo;                                            // [QT * 16][LDA] pooled rows of the frame, all heads
    float* Vs_all = As + QT * 16 * LDA;                             // [waves][16][SM_LDV]
    float* kinv_all = Vs_all + LE_NW * 16 * SM_LDV;                 // [waves][16]
    float* vinv_all = kinv_all + LE_NW * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.x;
    const int tok = lane & 15, kq = lane >> 4;
    // rows past the n queries are never written by the attention: they read as zeros (their products are dropped)
    for (int i = tid; i < (QT * 16 - sa.nq) * LDA; i += LE_NW * 64) As[sa.nq * LDA + i] = 0.f;
    attn_mfma_unit<QT, 1>(sa, g, wave, lane, Vs_all + wave * 16 * SM_LDV, kinv_all + wave * 16, vinv_all + wave * 16,
                          [&](int orank, int t, int tk, float v) { As[orank * LDA + wave * 64 + 16 * t + tk] = v; });
    __syncthreads();

    // output tile (row tile i, column tile j): one wave, the whole K = HD in the GEMM family's k order
    const int nct = (a.dl + 15) / 16, ntile = QT * nct;
    for (int t = wave; t < ntile; t += LE_NW) {
        const int ti = t / nct, tj = t % nct;
        const int wr = 16 * tj + tok;                               // weight row (output column) this lane feeds
        const bool wok = wr < a.dl;
        const float* wp = a.w + (int64_t)(wok ? wr : 0) * a.ldw + 4 * kq;
        const float* ap = As + (16 * ti + tok) * LDA + 4 * kq;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int s = 0; s < HD / 16; ++s) {
            f32x4 b = *reinterpret_cast<const f32x4*>(wp + 16 * s);
            if (!wok) b = f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4 x = *reinterpret_cast<const f32x4*>(ap + 16 * s);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(b[e], x[e], acc, 0, 0, 0);
        }
        // acc[r] = out[row 16 ti + (l & 15)][column 16 tj + 4 kq + r]
        const int row = 16 * ti + tok, col = 16 * tj + 4 * kq;
        if (row < sa.nq && col < a.dl) {
            float* pp = a.pred + ((int64_t)g * sa.nq + row) * a.ldp + col;
            if (col + 3 < a.dl && a.ldp % 4 == 0) *reinterpret_cast<f32x4*>(pp) = acc;
            else {
#pragma unroll
                for (int r = 0; r < 4; ++r) if (col + r < a.dl) pp[r] = acc[r];
            }
        }
    }
}

bool lqap_out_applicable(int heads, int dh, int n, int ns, int dl) {
    return heads == LE_NW && dh == 64 && n >= 1 && n <= 32 && ns >= 1 && ns <= 16 && dl >= 1 && dl <= 256;
}

int lqap_out(const float* kv, int ldkv, const float* q, const float* gate, const float* k_gamma, const float* w_out, int ldw, float* pred, int ldp, int frames,
             int heads, int n, int ns, int dl, hipStream_t s) {
    auto al16 = [](const void* p) { return ((uintptr_t)p % 16) == 0; };
    const int hd = heads * 64;
    D4_REQUIRE(lqap_out_applicable(heads, 64, n, ns, dl) && frames >= 0 && ldkv >= 2 * hd && ldkv % 4 == 0 && ldw >= hd && ldw % 4 == 0 && ldp >= dl && al16(kv) && al16(q) &&
               al16(k_gamma) && al16(w_out) && al16(pred) && gate, "lqap_out: call not supported (8 heads x 64, n <= 32, ns <= 16, dl <= 256, 16-byte aligned rows)");
    if (frames == 0) return 0;
    SmallAttnArgs sa{};
    sa.q = q; sa.q_group_stride = 0; sa.q_item_stride = hd;
    sa.k = kv; sa.k_group_stride = (int64_t)ns * ldkv; sa.k_item_stride = ldkv;
    sa.v = kv + hd; sa.v_group_stride = (int64_t)ns * ldkv; sa.v_item_stride = ldkv;
    sa.gate = gate; sa.g_group_stride = 0; sa.g_item_stride = heads;
    sa.k_gamma = k_gamma;
    sa.groups = frames; sa.heads = heads; sa.nq = n; sa.nk = ns;
    LqapOutArgs a{w_out, ldw, pred, ldp, dl};
    // algorithmic bytes: the frame's keys and values read once, the prediction written once, queries once (+ the projection weights once per XCD)
    const double bytes = 4.0 * ((double)frames * ns * 2.0 * hd + (double)frames * n * dl + (double)n * hd + 8.0 * dl * hd);
    const double flops = 2.0 * frames * n * (double)dl * hd;
    const int QT = n <= 16 ? 1 : 2;
    auto lds_of = [&](int qt) { return (size_t)(qt * 16 * (hd + 4) + LE_NW * 16 * (SM_LDV + 2)) * sizeof(float); };
    static DeviceOnce attr_set;
    if (attr_set.need()) {
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lqap_out_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of(1)));
        D4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lqap_out_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_of(2)));
        attr_set.done();
    }
    if (QT == 1) D4_GLUE_LAUNCH_F(GL_LATENT_ENDS, bytes, flops, (lqap_out_kernel<1>), dim3(frames), dim3(LE_NW * 64), lds_of(1), s, sa, a);
    else D4_GLUE_LAUNCH_F(GL_LATENT_ENDS, bytes, flops, (lqap_out_kernel<2>), dim3(frames), dim3(LE_NW * 64), lds_of(2), s, sa, a);
    D4_LAUNCH_CHECK();
    return 0;
}

}  // namespace d4
