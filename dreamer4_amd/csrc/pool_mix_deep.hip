// AttentionPool core (D4:2143-2177, value side restructured: see PoolMixArgs in kernels.h) over MORE than 64 layer hiddens: the pools of a trunk
// of depth >= 32 in the inference engine (wide_frames option), up to POOL_DEEP_MAX hiddens.
//
// The arithmetic is pool_mix_row's (pool_mix_row.h), expression for expression: key l2-norm with 1 / max(|k|, 1e-12), key gain (gamma + 1) * 8 and
// the 0.125 score scale, per-head softmax over the L hiddens, RMS-normalised hidden rows mixed per head, the head gate sigmoid(RMSNorm(x) . gate_w[h])
// applied once after the mix, x recognised as the last hidden row.  What differs is that nothing of size L lives in LDS or registers: the hiddens
// are walked in chunks of POOL_DEEP_CHUNK = 64, a chunk is scored as pool_mix_row scores its whole pool (four heads at once by 16-lane row
// reductions, the 64 x 4 scores parked in the wave's LDS, the exponentials once per (hidden, head) spread over the lanes), and between chunks the
// running maximum, the denominator and the unnormalised mixes acc[4][ITER] are carried by the online-softmax rescale; the division by the
// denominator happens once, after the last chunk.  Hidden 0 is in the first chunk, so the running maximum is finite from then on.  Every sum has a
// fixed order and there are no atomics: two runs give the same bits.
//
// Two forms, chosen by M and D alone (the rule of pool_mix):
//   pool_mix_deep_rows_kernel  (M <= 2048 && D <= 512)  one BLOCK per token row: wave w owns the hiddens l = w, w + 4, ... and walks ITS hiddens in
//                              chunks of 64, four key rows / four hidden rows per round with every load of a round issued before anything is
//                              computed; the four partial (maximum, denominator, mix) are merged through LDS in wave order.
//   pool_mix_deep_kernel       one wave per token row, the hidden rows one ahead.
#include "common.h"
#include "kernels.h"
#include "pool_mix_row.h"
#include <float.h>

namespace d4 {

int g_pool_mix_deep = 0;              // test hook d4_debug_switch("pool_mix_deep"): 1 = the engine's pools of <= 64 hiddens take this launcher too

namespace {

constexpr int PH = 4, CH = POOL_DEEP_CHUNK;

__device__ __forceinline__ f32x4 bf16x4_to_f32(const uint2 raw) {
    return f32x4{__builtin_bit_cast(float, raw.x << 16), __builtin_bit_cast(float, raw.x & 0xFFFF0000u),
                 __builtin_bit_cast(float, raw.y << 16), __builtin_bit_cast(float, raw.y & 0xFFFF0000u)};
}

template <bool KB16>
__device__ __forceinline__ f32x4 deep_key4(const PoolMixArgs& p, int l, int m, int lane) {
    if constexpr (KB16) return bf16x4_to_f32(*reinterpret_cast<const uint2*>(p.k_b + ((int64_t)l * p.M + m) * p.ldk + lane * 4));
    else return *reinterpret_cast<const f32x4*>(p.k + ((int64_t)l * p.M + m) * p.ldk + lane * 4);
}

// a value every lane of the wave holds alike (the running maximum, denominator and rescale factor): kept in a scalar register across the chunk loop
__device__ __forceinline__ float uniform_f(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

// the scores of the four heads against one key row (head = lane / 16): every lane of a 16-lane row ends up with its head's score
__device__ __forceinline__ float deep_score(const f32x4& kv, const f32x4& q4, const f32x4& g4) {
    const float nrm = sqrtf(row_sum16(kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2] + kv[3] * kv[3]));
    const float inv = 1.f / fmaxf(nrm, 1e-12f);
    return row_sum16(q4[0] * (kv[0] * inv * g4[0]) + q4[1] * (kv[1] * inv * g4[1]) + q4[2] * (kv[2] * inv * g4[2]) + q4[3] * (kv[3] * inv * g4[3])) * 0.125f;
}

// One chunk's softmax step on the wave's parked scores ps[n][4] (mxl: the chunk's per-head maximum in the head's lanes): folds the chunk maximum
// into the running one, turns ps into exp(s - new maximum), and rescales the running denominator; returns through `scale` the factor the mixes
// accumulated so far must be multiplied by.  `first`: nothing accumulated yet (the factor is an exact 0 instead of exp(-FLT_MAX - max)).
__device__ __forceinline__ void deep_chunk_softmax(float* ps, int n, int lane, float mxl, bool first, float (&mrun)[PH], float (&den)[PH], float (&scale)[PH]) {
#pragma unroll
    for (int h = 0; h < PH; ++h) {
        const float mn = uniform_f(fmaxf(mrun[h], readlane_f(mxl, h * 16)));
        scale[h] = first ? 0.f : uniform_f(expf(mrun[h] - mn));
        mrun[h] = mn;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int idx = lane; idx < n * PH; idx += 64) ps[idx] = expf(ps[idx] - mrun[idx & (PH - 1)]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    f32x4 cs = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int j = 0; j < n; ++j) cs += reinterpret_cast<const f32x4*>(ps)[j];
#pragma unroll
    for (int h = 0; h < PH; ++h) den[h] = uniform_f(den[h] * scale[h] + cs[h]);
}

template <int ITER>
__device__ __forceinline__ float deep_sumsq(const f32x4 (&v)[ITER]) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < ITER; ++i) ss += v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3];
    return ss;
}

// ---------------------------------------------------------------------------------------------- one wave per token row
template <int ITER, bool KB16>
__global__ __launch_bounds__(256) void pool_mix_deep_kernel(PoolMixArgs p) {
    __shared__ __attribute__((aligned(16))) float psh[4][CH * PH];
    __shared__ f32x4 gws[PH * ITER * 64];                 // head-gate weights [PH][D] of the pool (norm gamma folded; columns past D zero)
    const int L = p.L, D = p.D, nf4 = D / 4;
    for (int i = threadIdx.x; i < PH * ITER * 64; i += 256) {
        const int h = i / (ITER * 64), c4 = i % (ITER * 64);
        gws[i] = c4 < nf4 ? reinterpret_cast<const f32x4*>(p.gate_w)[h * nf4 + c4] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    const int wslot = threadIdx.x >> 6, lane = threadIdx.x & 63, hh = lane >> 4;
    const int m = blockIdx.x * 4 + wslot;
    if (m >= p.M) return;
    float* ps = psh[wslot];
    const bool x_is_last_hidden = p.x == p.hid + (int64_t)(L - 1) * p.M * D && p.ldx == D;
    float glog[PH] = {0.f, 0.f, 0.f, 0.f};
    const f32x4 q4 = pool_query4<KB16>(p, m, lane);
    f32x4 g4 = *reinterpret_cast<const f32x4*>(p.k_gamma + lane * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) g4[e] = (g4[e] + 1.f) * 8.f;

    auto load_row = [&](int l, f32x4 (&dst)[ITER]) {
        if (p.hid_b) {                                   // bf16 image of the hiddens: 8 bytes per lane and group
            const uint2* hb = reinterpret_cast<const uint2*>(p.hid_b + ((int64_t)l * p.M + m) * D);
#pragma unroll
            for (int i = 0; i < ITER; ++i) {
                const int c4 = lane + 64 * i;
                dst[i] = bf16x4_to_f32(c4 < nf4 ? hb[c4] : uint2{0u, 0u});
            }
            return;
        }
        const f32x4* hr = reinterpret_cast<const f32x4*>(p.hid + ((int64_t)l * p.M + m) * D);
#pragma unroll
        for (int i = 0; i < ITER; ++i) {
            const int c4 = lane + 64 * i;
            dst[i] = c4 < nf4 ? hr[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto gate_logits = [&](const f32x4 (&r)[ITER], float rstd) {
#pragma unroll
        for (int h = 0; h < PH; ++h) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < ITER; ++i) { const f32x4 g = gws[h * (ITER * 64) + lane + 64 * i]; d += r[i][0] * g[0] + r[i][1] * g[1] + r[i][2] * g[2] + r[i][3] * g[3]; }
            glog[h] = wave_sum(d) * rstd;
        }
    };

    float mrun[PH], den[PH];
    f32x4 acc[PH][ITER];
#pragma unroll
    for (int h = 0; h < PH; ++h) {
        mrun[h] = -FLT_MAX; den[h] = 0.f;
#pragma unroll
        for (int i = 0; i < ITER; ++i) acc[h][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 vn[ITER];                                       // the hidden row one ahead (across chunk edges too)
    load_row(0, vn);
#pragma unroll 1
    for (int c0 = 0; c0 < L; c0 += CH) {
        const int n = L - c0 < CH ? L - c0 : CH;          // a ragged last chunk: entries past n are neither written nor read
        float mxl = -FLT_MAX;
#pragma unroll 1
        for (int j = 0; j < n; ++j) {
            const float sc = deep_score(deep_key4<KB16>(p, c0 + j, m, lane), q4, g4);
            mxl = fmaxf(mxl, sc);
            if ((lane & 15) == 0) ps[j * PH + hh] = sc;
        }
        float scale[PH];
        deep_chunk_softmax(ps, n, lane, mxl, c0 == 0, mrun, den, scale);
#pragma unroll
        for (int h = 0; h < PH; ++h)
#pragma unroll
            for (int i = 0; i < ITER; ++i) acc[h][i] = acc[h][i] * scale[h];
#pragma unroll 1
        for (int j = 0; j < n; ++j) {
            const int l = c0 + j;
            f32x4 v[ITER];
#pragma unroll
            for (int i = 0; i < ITER; ++i) v[i] = vn[i];
            const float ss = deep_sumsq<ITER>(v);
            if (l + 1 < L) load_row(l + 1, vn);
            const float rstd = rsqrtf(wave_sum(ss) / (float)D + p.eps);
            const f32x4 e4 = reinterpret_cast<const f32x4*>(ps)[j];
#pragma unroll
            for (int h = 0; h < PH; ++h) {
                const float w = e4[h] * rstd;
#pragma unroll
                for (int i = 0; i < ITER; ++i) acc[h][i] += v[i] * w;
            }
            if (l == L - 1 && x_is_last_hidden) gate_logits(v, rstd);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the next chunk's scores overwrite ps
        __builtin_amdgcn_wave_barrier();
    }
    if (!x_is_last_hidden) {
        const f32x4* xr = reinterpret_cast<const f32x4*>(p.x + (int64_t)m * p.ldx);
        f32x4 xv[ITER];
#pragma unroll
        for (int i = 0; i < ITER; ++i) {
            const int c4 = lane + 64 * i;
            xv[i] = c4 < nf4 ? xr[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        gate_logits(xv, rsqrtf(wave_sum(deep_sumsq<ITER>(xv)) / (float)D + p.eps));
    }
#pragma unroll
    for (int h = 0; h < PH; ++h) {
        const float f = 1.f / den[h], gate = sigmoidf(glog[h]);
#pragma unroll
        for (int i = 0; i < ITER; ++i) {
            const int c4 = lane + 64 * i;
            if (c4 >= nf4) continue;
            const f32x4 o = acc[h][i] * f * gate;
            if (p.u) reinterpret_cast<f32x4*>(p.u + ((int64_t)m * PH + h) * D)[c4] = o;
            if (p.u_b) store_bf16x4(p.u_b + ((int64_t)m * PH + h) * D + 4 * c4, o);
        }
    }
}

// ---------------------------------------------------------------------------------------------- one block per token row
// Wave w owns the hiddens l = w + 4 t, t = 0 .. nw - 1, and runs the chunked walk above over ITS hiddens (a chunk = 64 of them = 256 of the pool's),
// four per round.  Merge buffer: accs [wave][head][D / 4] float4 — lane c4 writes and reads float4 c4, consecutive 16-byte slots, so both the
// ds_write_b128 and the ds_read_b128 of the merge are conflict-free; the per-wave maxima / denominators are 2 x 16 floats next to it.
template <int ITER, bool KB16>
__global__ __launch_bounds__(256) void pool_mix_deep_rows_kernel(PoolMixArgs p) {
    __shared__ __attribute__((aligned(16))) float psh[4][CH * PH];
    __shared__ float msh[4][PH], dsh[4][PH], gsh[PH];
    __shared__ f32x4 accs[4][PH][ITER * 64];
    const int L = p.L, D = p.D, nf4 = D / 4;
    const int m = blockIdx.x;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, hh = lane >> 4;
    float* ps = psh[w];
    const int nw = w < L ? (L - w + 3) / 4 : 0;            // this wave's hiddens
    const f32x4 q4 = pool_query4<KB16>(p, m, lane);
    f32x4 g4 = *reinterpret_cast<const f32x4*>(p.k_gamma + lane * 4);
    auto load_keys = [&](int t0, f32x4 (&kv)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) kv[j] = t0 + j < nw ? deep_key4<KB16>(p, w + 4 * (t0 + j), m, lane) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto load_hid = [&](int t0, f32x4 (&v)[4][ITER]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = t0 + j < nw;
            const f32x4* hr = reinterpret_cast<const f32x4*>(p.hid + ((int64_t)(on ? w + 4 * (t0 + j) : 0) * p.M + m) * D);
#pragma unroll
            for (int i = 0; i < ITER; ++i) {
                const int c4 = lane + 64 * i;
                v[j][i] = (on && c4 < nf4) ? hr[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    const bool x_is_last_hidden = p.x == p.hid + (int64_t)(L - 1) * p.M * D && p.ldx == D;
    const bool gating_wave = w == (x_is_last_hidden ? ((L - 1) & 3) : 0);          // l = w (mod 4): the wave that meets hidden L - 1
    // every global load of the first round is issued before anything is computed: query, key rows, hidden rows, and for the gating wave the gate
    // weights (and x when it is not the last hidden)
    f32x4 kv[4], v[4][ITER], gwv[PH][ITER], xv[ITER];
    load_keys(0, kv);
    load_hid(0, v);
    if (gating_wave) {
        const f32x4* gw = reinterpret_cast<const f32x4*>(p.gate_w);
        const f32x4* xr = reinterpret_cast<const f32x4*>(p.x + (int64_t)m * p.ldx);
#pragma unroll
        for (int i = 0; i < ITER; ++i) {
            const int c4 = lane + 64 * i;
#pragma unroll
            for (int h = 0; h < PH; ++h) gwv[h][i] = c4 < nf4 ? gw[h * nf4 + c4] : f32x4{0.f, 0.f, 0.f, 0.f};
            xv[i] = (!x_is_last_hidden && c4 < nf4) ? xr[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) g4[e] = (g4[e] + 1.f) * 8.f;
    auto gate_logits = [&](const f32x4 (&r)[ITER], float rstd) {       // gate_h = sigmoid(RMSNorm(x) . gate_w[h])
#pragma unroll
        for (int h = 0; h < PH; ++h) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < ITER; ++i) d += r[i][0] * gwv[h][i][0] + r[i][1] * gwv[h][i][1] + r[i][2] * gwv[h][i][2] + r[i][3] * gwv[h][i][3];
            d = wave_sum(d) * rstd;
            if (lane == 0) gsh[h] = d;
        }
    };
    float mrun[PH], den[PH];
    f32x4 acc[PH][ITER];
#pragma unroll
    for (int h = 0; h < PH; ++h) {
        mrun[h] = -FLT_MAX; den[h] = 0.f;
#pragma unroll
        for (int i = 0; i < ITER; ++i) acc[h][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1
    for (int tc = 0; tc < nw; tc += CH) {
        const int n = nw - tc < CH ? nw - tc : CH;
        if (tc != 0) load_hid(tc, v);                     // the chunk's first four hidden rows travel while its keys are scored
        float mxl = -FLT_MAX;
#pragma unroll 1
        for (int r = 0; r < n; r += 4) {
            if (tc + r != 0) load_keys(tc + r, kv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float sc = deep_score(kv[j], q4, g4);           // (a key row past the wave's last is zeros: score 0, not stored, not in the maximum)
                if (r + j < n) {
                    mxl = fmaxf(mxl, sc);
                    if ((lane & 15) == 0) ps[(r + j) * PH + hh] = sc;
                }
            }
        }
        float scale[PH];
        deep_chunk_softmax(ps, n, lane, mxl, tc == 0, mrun, den, scale);
#pragma unroll
        for (int h = 0; h < PH; ++h)
#pragma unroll
            for (int i = 0; i < ITER; ++i) acc[h][i] = acc[h][i] * scale[h];
#pragma unroll 1
        for (int r = 0; r < n; r += 4) {
            if (r != 0) load_hid(tc + r, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (r + j >= n) break;
                const int l = w + 4 * (tc + r + j);
                const float rstd = rsqrtf(wave_sum(deep_sumsq<ITER>(v[j])) / (float)D + p.eps);
                const f32x4 e4 = reinterpret_cast<const f32x4*>(ps)[r + j];
#pragma unroll
                for (int h = 0; h < PH; ++h) {
                    const float wt = e4[h] * rstd;
#pragma unroll
                    for (int i = 0; i < ITER; ++i) acc[h][i] += v[j][i] * wt;
                }
                if (l == L - 1 && x_is_last_hidden) gate_logits(v[j], rstd);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the next chunk's scores overwrite ps
        __builtin_amdgcn_wave_barrier();
    }
    if (!x_is_last_hidden && w == 0) gate_logits(xv, rsqrtf(wave_sum(deep_sumsq<ITER>(xv)) / (float)D + p.eps));
#pragma unroll
    for (int h = 0; h < PH; ++h) {
        if (lane == 0) { msh[w][h] = mrun[h]; dsh[w][h] = den[h]; }
#pragma unroll
        for (int i = 0; i < ITER; ++i) accs[w][h][lane + 64 * i] = acc[h][i];
    }
    __syncthreads();
    // merge in wave order: maximum over the waves, each partial rescaled to it (a wave without a hidden has denominator 0: factor an exact 0)
    for (int idx = threadIdx.x; idx < PH * ITER * 64; idx += 256) {
        const int h = idx / (ITER * 64), c4 = idx % (ITER * 64);
        if (c4 >= nf4) continue;
        const float mx = fmaxf(fmaxf(msh[0][h], msh[1][h]), fmaxf(msh[2][h], msh[3][h]));
        float s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = dsh[k][h] > 0.f ? expf(msh[k][h] - mx) : 0.f;
        const float dn = ((dsh[0][h] * s[0] + dsh[1][h] * s[1]) + dsh[2][h] * s[2]) + dsh[3][h] * s[3];
        const f32x4 sum = ((accs[0][h][c4] * s[0] + accs[1][h][c4] * s[1]) + accs[2][h][c4] * s[2]) + accs[3][h][c4] * s[3];
        const f32x4 gated = sum * (1.f / dn) * sigmoidf(gsh[h]);
        if (p.u) reinterpret_cast<f32x4*>(p.u + ((int64_t)m * PH + h) * D)[c4] = gated;
        if (p.u_b) store_bf16x4(p.u_b + ((int64_t)m * PH + h) * D + 4 * c4, gated);
    }
}

}  // namespace

int pool_mix_deep(const PoolMixArgs& p, hipStream_t stream) {
    D4_REQUIRE(p.heads == 4, "pool_mix_deep: heads=%d, 4 pool heads expected (AttentionPool default, D4:2147)", p.heads);
    D4_REQUIRE(p.L >= 1 && p.L <= POOL_DEEP_MAX, "pool_mix_deep: L=%d out of range [1,%d]", p.L, POOL_DEEP_MAX);
    D4_REQUIRE(p.D >= 4 && p.D % 4 == 0 && p.D <= 1024, "pool_mix_deep: D=%d: a multiple of 4 up to 1024 expected", p.D);
    D4_REQUIRE(p.k_b ? (p.q != nullptr || p.q_b != nullptr) : (p.k != nullptr && p.q != nullptr && p.q_b == nullptr),
               "pool_mix_deep: keys / queries: fp32 (k, q) or the bf16 images (k_b with q or q_b)");
    D4_REQUIRE(p.u != nullptr || p.u_b != nullptr, "pool_mix_deep: no output");
    if (p.M == 0) return 0;
    const bool kb = p.k_b != nullptr;
    const dim3 block(256);
    if ((p.rule_M > 0 ? p.rule_M : p.M) <= 2048 && p.D <= 512) {      // the rule of pool_mix: by M and D alone, so a shape always takes the same arithmetic path
        const dim3 grid(p.M);
        if (p.D <= 256) {
            note_pool_deep_form(kb ? "pool_mix_deep_rows_kernel<1,bf16>" : "pool_mix_deep_rows_kernel<1>");
            if (kb) hipLaunchKernelGGL((pool_mix_deep_rows_kernel<1, true>), grid, block, 0, stream, p);
            else hipLaunchKernelGGL((pool_mix_deep_rows_kernel<1, false>), grid, block, 0, stream, p);
        } else {
            note_pool_deep_form(kb ? "pool_mix_deep_rows_kernel<2,bf16>" : "pool_mix_deep_rows_kernel<2>");
            if (kb) hipLaunchKernelGGL((pool_mix_deep_rows_kernel<2, true>), grid, block, 0, stream, p);
            else hipLaunchKernelGGL((pool_mix_deep_rows_kernel<2, false>), grid, block, 0, stream, p);
        }
        D4_LAUNCH_CHECK();
        return 0;
    }
    const dim3 grid(cdiv(p.M, 4));
    if (p.D <= 256) {
        note_pool_deep_form(kb ? "pool_mix_deep_kernel<1,bf16>" : "pool_mix_deep_kernel<1>");
        if (kb) hipLaunchKernelGGL((pool_mix_deep_kernel<1, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((pool_mix_deep_kernel<1, false>), grid, block, 0, stream, p);
    } else if (p.D <= 512) {
        note_pool_deep_form(kb ? "pool_mix_deep_kernel<2,bf16>" : "pool_mix_deep_kernel<2>");
        if (kb) hipLaunchKernelGGL((pool_mix_deep_kernel<2, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((pool_mix_deep_kernel<2, false>), grid, block, 0, stream, p);
    } else {
        note_pool_deep_form(kb ? "pool_mix_deep_kernel<4,bf16>" : "pool_mix_deep_kernel<4>");
        if (kb) hipLaunchKernelGGL((pool_mix_deep_kernel<4, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((pool_mix_deep_kernel<4, false>), grid, block, 0, stream, p);
    }
    D4_LAUNCH_CHECK();
    return 0;
}

}  // namespace d4
