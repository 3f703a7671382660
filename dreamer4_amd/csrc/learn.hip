// Actor / critic learner: reference DynamicsWorldModel.learn_from_experience with
// only_learn_policy_value_heads=True and stored agent embeddings (D4:5893-6305), forward AND
// backward, plus the clipped AdamW step DreamTrainer applies (trainers.py:1436-1452).
//
//   calc_gae (D4:1566-1600) -> masked z-score (D4:404-410, 6024) -> policy MLP + unembed head 0 ->
//   log-prob / entropy (D4:1422-1426) -> PPO / SPO / PMPO surrogate with delight gating
//   (D4:6119-6242) ;  value MLP -> HL-Gauss cross entropy against transform_to_probs(returns)
//   (D4:6268-6295).
//
// The reference builds these losses from ~40 elementwise ATen ops and lets autograd derive the
// gradients; here each loss has one fused forward+backward kernel and the MLP backward is explicit
// (GEMMs on the MFMA kernel in its transposed-operand modes, deterministic column reductions).
// Every reduction has a fixed order: results are bitwise reproducible run to run.
#include "common.h"
#include "engine.h"
#include "beta.h"
#include <float.h>
#include <math.h>

namespace d4 {

static constexpr float RMS_EPS_L = 1.1920928955078125e-07f;

// ------------------------------------------------------------------------------------ GAE
// one thread per trajectory: masks (D4:5943-5967) + reverse recurrence
__global__ void gae_kernel(const float* rewards, const float* values, const int64_t* lens, const uint8_t* is_truncated,
                           const uint8_t* terminals, float gamma, float lam, int B, int T,
                           float* returns, float* adv, float* mask) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int len = lens ? (int)lens[b] : T;
    const int trunc = is_truncated ? (is_truncated[b] != 0) : 1;
    const int term = terminals ? (terminals[b] != 0) : 0;
    const int learn_len = len - trunc;
    const int last = len - 1 > 0 ? len - 1 : 0;
    float g = 0.f, v_next = 0.f;
    for (int t = T - 1; t >= 0; --t) {
        const bool in_len = t < len;
        const float r = in_len ? rewards[(int64_t)b * T + t] : 0.f;
        const float v = in_len ? values[(int64_t)b * T + t] : 0.f;
        bool cont = t < last;
        if (term && t == last) cont = false;
        const float m = cont ? 1.f : 0.f;
        const bool learn = t < learn_len;
        float delta = r + gamma * v_next * m - v;
        if (!learn) delta = 0.f;
        g = (gamma * lam * m) * g + delta;
        const float ret = g + v;
        returns[(int64_t)b * T + t] = ret;
        if (adv) adv[(int64_t)b * T + t] = ret - v;
        if (mask) mask[(int64_t)b * T + t] = learn ? 1.f : 0.f;
        v_next = v;
    }
}

// old values with 0 past `len`, as gae_kernel reads them (D4:5950): the input of the return statistics and of the value clipping
__global__ void masked_old_values_kernel(const float* values, const int64_t* lens, int B, int T, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * T) return;
    const int b = i / T, t = i - b * T;
    out[i] = (!lens || t < (int)lens[b]) ? values[i] : 0.f;
}

// ------------------------------------------------------------------------------------ deterministic reductions
// out[slot] = sum_i f(a[i], b[i]) with one 1024-thread block (fixed tree order).
enum { RED_PROD = 0, RED_SQDIFF_MASKED = 1, RED_SUM = 2 };
template <int MODE>
__global__ __launch_bounds__(1024) void reduce1_kernel(const float* a, const float* b, const float* scal, int64_t n, float* out) {
    __shared__ float sh[1024];
    float s = 0.f;
    float mean = 0.f;
    if (MODE == RED_SQDIFF_MASKED) mean = scal[0] / fmaxf(scal[1], 1.f);
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        if (MODE == RED_PROD) s += a[i] * b[i];
        else if (MODE == RED_SUM) s += a[i];
        else { float d = a[i] - mean; s += d * d * b[i]; }
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

// column sums: out[c] = sum_r x[r][c]; block = 16 columns x 64 row lanes (4x more blocks than a 64-column block: the
// [4096][2048] bias-gradient reductions are latency bound, not bandwidth bound), 16 loads in flight per thread (a 3840-row reduction is
// four round trips to memory instead of eight: 14.7 -> ~8 us), fixed order
__device__ __forceinline__ void colsum_block(const float* x, int ld, int rows, int cols, float* out, int bx) {
    __shared__ float sh[64][17];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = bx * 16 + cl;
    float s = 0.f;
    if (c < cols) {
        for (int r = rl; r < rows; r += 16 * 64) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int rr = r + u * 64;
                v[u] = rr < rows ? x[(int64_t)rr * ld + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) s += v[u];
        }
    }
    sh[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < cols) {
        float t = 0.f;
        for (int i = 0; i < 64; ++i) t += sh[i][cl];
        out[c] = t;
    }
}
__global__ __launch_bounds__(1024) void colsum_kernel(const float* x, int ld, int rows_all, int cols, float* out_all, int chunk) {
    // blockIdx.y: row chunk [y * chunk, (y + 1) * chunk) summed into row y of out (one chunk = the whole matrix in the plain form)
    const int r_lo = blockIdx.y * chunk, rows = min(rows_all, r_lo + chunk) - r_lo;
    colsum_block(x + (int64_t)r_lo * ld, ld, rows, cols, out_all + (int64_t)blockIdx.y * cols, blockIdx.x);
}
// several independent column sums in ONE launch (a block backward has three or four: bias, norm-gain and key-gain gradients — each alone is a
// 32-block, latency-bound launch of ~14 us); same per-column arithmetic and order as colsum_kernel
__global__ __launch_bounds__(1024) void colsum_batch_kernel(ColsumBatch b) {
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.first[i + 1]) ++i;
    colsum_block(b.x[i], b.ld[i], b.rows[i], b.cols[i], b.out[i], blockIdx.x - b.first[i]);
}
int colsum_batch(ColsumBatch& b, hipStream_t s) {
    if (b.n == 0) return 0;
    int nb = 0;
    for (int i = 0; i < b.n; ++i) { b.first[i] = nb; nb += cdiv(b.cols[i], 16); }
    hipLaunchKernelGGL(colsum_batch_kernel, dim3(nb), dim3(1024), 0, s, b);
    D4_LAUNCH_CHECK();
    return 0;
}
// scratch (optional, >= 16 * cols floats): tall matrices (the attention pools' context gradients: up to 13 x the token rows) are summed in 16
// row chunks over 16 x the blocks, then the 16 partial rows in a second, tiny launch — fixed order either way
int colsum(const float* x, int ld, int rows, int cols, float* out, hipStream_t s, float* scratch, size_t scratch_floats) {
    constexpr int SY = 16;
    if (scratch && rows >= 8192 && scratch_floats >= (size_t)SY * cols) {
        const int chunk = cdiv(cdiv(rows, SY), 64) * 64;
        const int ny = cdiv(rows, chunk);
        hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(cols, 16), ny), dim3(1024), 0, s, x, ld, rows, cols, scratch, chunk);
        hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(cols, 16)), dim3(1024), 0, s, scratch, cols, ny, cols, out, ny);
        D4_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(cols, 16)), dim3(1024), 0, s, x, ld, rows, cols, out, rows);
    D4_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------ policy loss fwd + bwd
struct PolicyLossArgs {
    const float* logits; int ld;        // [R][Apad]
    const int64_t* actions;             // [R][na]
    const float* old_lp;                // [R][na]
    const float* old_logits; int ldo;   // [R][A] (pmpo) or null
    const float* adv_raw;               // [R]
    const float* mask;                  // [R]
    const float* scal;                  // stats: [0] sum adv*mask, [1] count, [2] sum sq diff
    const int32_t* action_sizes;
    float* dlogits;                     // [R][Apad]
    float* row_pl; float* row_ent; float* row_aux;   // per-row masked terms
    // continuous actions (Beta head): raw parameters [R][ldc] (2 per action), targets, old log-probs, old parameters (pmpo KL)
    const float* cparams; int ldc;
    const float* actions_cont; const float* old_lp_cont; const float* old_cparams;
    float* dcparams;                    // [R][ldc]
    int beta_param;                     // d4_config.continuous_beta_param
    int nc;
    int R, na, A, objective, normalize, use_gate, reverse_kl;
    float eps, clip, ent_w, gate_temp, pmpo_alpha, kl_w;
};

__global__ void policy_loss_kernel(PolicyLossArgs p) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.R) return;
    const float count = fmaxf(p.scal[1], 1.f);
    const float mk = p.mask[r];
    float adv = p.adv_raw[r];
    if (p.normalize) {
        const float mean = p.scal[0] / count;
        const float var = p.scal[2] / count;
        adv = (adv - mean) / sqrtf(fmaxf(var, p.eps));
    }
    const float* lg = p.logits + (int64_t)r * p.ld;
    float* dl = p.dlogits + (int64_t)r * p.ld;
    // pass 1: joint log-prob, entropy
    float lp = 0.f, old = 0.f, ent = 0.f;
    int o = 0;
    for (int a = 0; a < p.na; ++a) {
        const int n = p.action_sizes[a];
        float mx = -FLT_MAX;
        for (int j = 0; j < n; ++j) mx = fmaxf(mx, lg[o + j]);
        float se = 0.f;
        for (int j = 0; j < n; ++j) se += expf(lg[o + j] - mx);
        const float lse = mx + logf(se);
        const int act = (int)p.actions[(int64_t)r * p.na + a];
        lp += lg[o + act] - lse;
        old += p.old_lp[(int64_t)r * p.na + a];
        float h = 0.f;
        for (int j = 0; j < n; ++j) { const float l = lg[o + j] - lse; h -= expf(l) * l; }
        ent += h;
        o += n;
    }
    // continuous actions: log-prob of the stored action and entropy of each Beta join the same sums  D4:6090-6111
    for (int c = 0; c < p.nc; ++c) {
        const float* raw = p.cparams + (int64_t)r * p.ldc + 2 * c;
        const BetaAB ab = beta_ab(raw[0], raw[1], p.beta_param);
        lp += beta_log_prob(ab.a, ab.b, p.actions_cont[(int64_t)r * p.nc + c]);
        old += p.old_lp_cont[(int64_t)r * p.nc + c];
        ent += lbetaf(ab.a, ab.b) - (ab.a - 1.f) * digammaf(ab.a) - (ab.b - 1.f) * digammaf(ab.b) + (ab.a + ab.b - 2.f) * digammaf(ab.a + ab.b);
    }
    const float gate = p.use_gate ? sigmoidf(-lp * adv / p.gate_temp) : 1.f;
    float pl = 0.f, dpl_dlp = 0.f, aux = 0.f;
    if (p.objective == 0) {             // ppo  D4:6204-6212
        const float ratio = expf(lp - old);
        const float cr = fminf(fmaxf(ratio, 1.f - p.clip), 1.f + p.clip);
        const float s1 = ratio * adv, s2 = cr * adv;
        pl = -fminf(s1, s2) * gate;
        const bool inside = ratio >= 1.f - p.clip && ratio <= 1.f + p.clip;
        const float dmin = (s1 < s2 || (s1 == s2 && inside)) ? s1 : ((s1 == s2) ? 0.5f * s1 : 0.f);
        dpl_dlp = -dmin * gate;
    } else if (p.objective == 1) {      // spo  D4:6188-6198
        const float ratio = expf(lp - old);
        const float q = fabsf(adv) * (ratio - 1.f) / p.clip;
        pl = -(ratio * adv - fabsf(adv) * (ratio - 1.f) * (ratio - 1.f) / (2.f * p.clip)) * gate;
        dpl_dlp = -(ratio * adv - q * ratio) * gate;
    } else {                            // pmpo D4:6127-6154
        const float w = fabsf(tanhf(adv)) * gate;
        const float sgn = adv >= 0.f ? 1.f : -1.f;
        pl = -p.pmpo_alpha * sgn * lp * w;              // summed / num below (mask applied there)
        dpl_dlp = -p.pmpo_alpha * sgn * w;
    }
    // pass 2: gradients wrt logits
    const float scale = mk / count;
    o = 0;
    for (int a = 0; a < p.na; ++a) {
        const int n = p.action_sizes[a];
        float mx = -FLT_MAX;
        for (int j = 0; j < n; ++j) mx = fmaxf(mx, lg[o + j]);
        float se = 0.f;
        for (int j = 0; j < n; ++j) se += expf(lg[o + j] - mx);
        const float lse = mx + logf(se);
        const int act = (int)p.actions[(int64_t)r * p.na + a];
        float h = 0.f;
        for (int j = 0; j < n; ++j) { const float l = lg[o + j] - lse; h -= expf(l) * l; }
        float kl = 0.f, lse_o = 0.f;
        if (p.objective == 2 && p.kl_w > 0.f && p.old_logits) {
            const float* og = p.old_logits + (int64_t)r * p.ldo;
            float mo = -FLT_MAX;
            for (int j = 0; j < n; ++j) mo = fmaxf(mo, og[o + j]);
            float so = 0.f;
            for (int j = 0; j < n; ++j) so += expf(og[o + j] - mo);
            lse_o = mo + logf(so);
            for (int j = 0; j < n; ++j) {
                const float ln = lg[o + j] - lse, lo = og[o + j] - lse_o;
                kl += p.reverse_kl ? expf(lo) * (lo - ln) : expf(ln) * (ln - lo);
            }
            aux += kl;
        }
        for (int j = 0; j < n; ++j) {
            const float l = lg[o + j] - lse;
            const float pj = expf(l);
            float g = dpl_dlp * ((j == act ? 1.f : 0.f) - pj);          // d lp / d logit
            g += p.ent_w * pj * (l + h);                                  // d(-H)/d logit
            if (p.objective == 2 && p.kl_w > 0.f && p.old_logits) {
                const float lo = p.old_logits[(int64_t)r * p.ldo + o + j] - lse_o;
                g += p.kl_w * (p.reverse_kl ? (pj - expf(lo)) : pj * ((l - lo) - kl));
            }
            dl[o + j] = g * scale;
        }
        o += n;
    }
    for (int j = p.A; j < p.ld; ++j) dl[j] = 0.f;
    // gradients wrt the raw Beta parameters: d lp, d(-H) and (pmpo) the KL against the behaviour parameters
    for (int c = 0; c < p.nc; ++c) {
        const float* raw = p.cparams + (int64_t)r * p.ldc + 2 * c;
        const BetaAB ab = beta_ab(raw[0], raw[1], p.beta_param);
        const float a = ab.a, b = ab.b, x = p.actions_cont[(int64_t)r * p.nc + c];
        const float psi_a = digammaf(a), psi_b = digammaf(b), psi_ab = digammaf(a + b);
        const float tri_ab = trigammaf(a + b);
        float ga = dpl_dlp * (logf(x) - psi_a + psi_ab);                              // d lp / d alpha
        float gb = dpl_dlp * (log1pf(-x) - psi_b + psi_ab);
        // H = lbeta - (a-1) psi(a) - (b-1) psi(b) + (a+b-2) psi(a+b);  dH/da = -(a-1) psi'(a) + (a+b-2) psi'(a+b)
        ga += p.ent_w * ((a - 1.f) * trigammaf(a) - (a + b - 2.f) * tri_ab);          // d(-H) / d alpha
        gb += p.ent_w * ((b - 1.f) * trigammaf(b) - (a + b - 2.f) * tri_ab);
        if (p.objective == 2 && p.kl_w > 0.f && p.old_cparams) {
            const float* oraw = p.old_cparams + ((int64_t)r * p.nc + c) * 2;
            const BetaAB ob = beta_ab(oraw[0], oraw[1], p.beta_param);
            const float a2 = ob.a, b2 = ob.b;
            float kl, ka, kb;
            if (p.reverse_kl) {
                // KL(old || new): lbeta(a,b) - lbeta(a2,b2) + (a2-a) psi(a2) + (b2-b) psi(b2) + (a-a2+b-b2) psi(a2+b2)
                const float q_a = digammaf(a2), q_b = digammaf(b2), q_ab = digammaf(a2 + b2);
                kl = lbetaf(a, b) - lbetaf(a2, b2) + (a2 - a) * q_a + (b2 - b) * q_b + (a - a2 + b - b2) * q_ab;
                ka = (psi_a - psi_ab) - q_a + q_ab;
                kb = (psi_b - psi_ab) - q_b + q_ab;
            } else {
                // KL(new || old): lbeta(a2,b2) - lbeta(a,b) + (a-a2) psi(a) + (b-b2) psi(b) + (a2-a+b2-b) psi(a+b)
                kl = lbetaf(a2, b2) - lbetaf(a, b) + (a - a2) * psi_a + (b - b2) * psi_b + (a2 - a + b2 - b) * psi_ab;
                ka = -(psi_a - psi_ab) + psi_a + (a - a2) * trigammaf(a) - psi_ab + (a2 - a + b2 - b) * tri_ab;
                kb = -(psi_b - psi_ab) + psi_b + (b - b2) * trigammaf(b) - psi_ab + (a2 - a + b2 - b) * tri_ab;
            }
            aux += kl;
            ga += p.kl_w * ka; gb += p.kl_w * kb;
        }
        float* dc = p.dcparams + (int64_t)r * p.ldc + 2 * c;
        dc[0] = ga * ab.da * scale;
        dc[1] = gb * ab.db * scale;
    }
    for (int j = 2 * p.nc; j < p.ldc; ++j) p.dcparams[(int64_t)r * p.ldc + j] = 0.f;
    p.row_pl[r] = pl * mk;
    p.row_ent[r] = -ent * mk;
    p.row_aux[r] = aux * mk;
}

// ------------------------------------------------------------------------------------ value loss fwd + bwd
// one wave per row: HL-Gauss target probs (erf), CE against log_softmax(value bins)
// (TWO_HOT: SymExpTwoHot.forward D4:1001-1040 — `support` holds the `bins` bin values; the target puts (right - v) / (right - left) on the
//  bin to the left of v and the rest on its right neighbour)
template <bool TWO_HOT>
__global__ __launch_bounds__(256) void value_loss_kernel(const float* vbins, int ld, const float* returns, const float* mask,
                                                         const float* scal, const float* support, int R, int bins,
                                                         float sigma_sqrt2, float hl_eps, float vmin, float vmax,
                                                         float* dv, float* row_loss) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    const float count = fmaxf(scal[1], 1.f);
    const float mk = mask[r];
    const float* v = vbins + (int64_t)r * ld;
    float ret = fminf(fmaxf(returns[r], TWO_HOT ? support[0] : vmin), TWO_HOT ? support[bins - 1] : vmax);
    int li = 0, ri = 0;
    float wl = 0.f;
    if (TWO_HOT) {
        // torch.searchsorted(bin_values, v): first index with bin_values[i] >= v (binary search, wave-uniform)
        int lo = 0, hi = bins;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (support[mid] < ret) lo = mid + 1; else hi = mid; }
        li = lo - 1 > 0 ? lo - 1 : 0;
        ri = li + 1 < bins - 1 ? li + 1 : bins - 1;
        wl = (support[ri] - ret) / (support[ri] - support[li]);
    }
    const float z = TWO_HOT ? 1.f : erff((support[bins] - ret) / sigma_sqrt2) - erff((support[0] - ret) / sigma_sqrt2);
    const float zc = fmaxf(z, hl_eps);
    auto target = [&](int c) -> float {
        if (TWO_HOT) return c == ri ? 1.f - wl : (c == li ? wl : 0.f);            // (scatter order of the reference: right written last)
        return (erff((support[c + 1] - ret) / sigma_sqrt2) - erff((support[c] - ret) / sigma_sqrt2)) / zc;
    };
    float mx = -FLT_MAX;
    for (int c = lane; c < bins; c += 64) mx = fmaxf(mx, v[c]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int c = lane; c < bins; c += 64) se += expf(v[c] - mx);
    const float lse = mx + logf(wave_sum(se));
    float loss = 0.f, psum = 0.f;
    for (int c = lane; c < bins; c += 64) {
        const float pr = target(c);
        loss -= pr * (v[c] - lse);
        psum += pr;
    }
    loss = wave_sum(loss);
    psum = wave_sum(psum);
    const float scale = mk / count;
    for (int c = lane; c < bins; c += 64) {
        const float pr = target(c);
        dv[(int64_t)r * ld + c] = (expf(v[c] - lse) * psum - pr) * scale;
    }
    for (int c = bins + lane; c < ld; c += 64) dv[(int64_t)r * ld + c] = 0.f;
    if (lane == 0) row_loss[r] = loss * mk;
}

// ------------------------------------------------------------------------------------ value loss with PPO value clipping, fwd + bwd
// D4:6283-6291 on top of value_loss_kernel (same targets, same CE, one wave per row):
//   values  = sum_c softmax(v)_c * centre_c            (HL-Gauss: centres of the bin edges; TWO_HOT: the bin values)
//   clipped = old + clamp(values - old, -clip, clip);  q = encoder(clipped), the encoder and range clamp of the returns
//   loss    = max(CE, -sum_c p_c log max(q_c, 1e-20))
// Gradient: where the clipped branch wins, d loss / d clipped goes through q (HL-Gauss: the erf differences and the normaliser; two-hot: the two
// weights) and, where neither the +-clip clamp nor the range clamp is active (autograd's clamp: inclusive ends), on through values into the
// logits: d values / d v_j = softmax_j (centre_j - values).  A q_c below 1e-20 passes nothing (clamp(min)).  A tie of the two losses halves both.
template <bool TWO_HOT>
__global__ __launch_bounds__(256) void value_loss_clip_kernel(const float* vbins, int ld, const float* returns, const float* old_values, const float* mask,
                                                              const float* scal, const float* support, int R, int bins,
                                                              float sigma_sqrt2, float hl_eps, float vmin, float vmax, float clip,
                                                              float* dv, float* row_loss) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    const float count = fmaxf(scal[1], 1.f);
    const float mk = mask[r];
    const float* v = vbins + (int64_t)r * ld;
    const float rlo = TWO_HOT ? support[0] : vmin, rhi = TWO_HOT ? support[bins - 1] : vmax;
    // encoder of a scalar x already clamped into the range: two-hot indices and left weight, or the HL-Gauss normaliser
    auto two_hot_of = [&](float x, int& li, int& ri, float& wl) {
        int lo = 0, hi = bins;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (support[mid] < x) lo = mid + 1; else hi = mid; }
        li = lo - 1 > 0 ? lo - 1 : 0;
        ri = li + 1 < bins - 1 ? li + 1 : bins - 1;
        wl = (support[ri] - x) / (support[ri] - support[li]);
    };
    const float ret = fminf(fmaxf(returns[r], rlo), rhi);
    int li = 0, ri = 0;
    float wl = 0.f;
    if (TWO_HOT) two_hot_of(ret, li, ri, wl);
    const float z = TWO_HOT ? 1.f : erff((support[bins] - ret) / sigma_sqrt2) - erff((support[0] - ret) / sigma_sqrt2);
    const float zc = fmaxf(z, hl_eps);
    auto target = [&](int c) -> float {
        if (TWO_HOT) return c == ri ? 1.f - wl : (c == li ? wl : 0.f);
        return (erff((support[c + 1] - ret) / sigma_sqrt2) - erff((support[c] - ret) / sigma_sqrt2)) / zc;
    };
    auto centre = [&](int c) -> float { return TWO_HOT ? support[c] : (support[c] + support[c + 1]) / 2.f; };
    float mx = -FLT_MAX;
    for (int c = lane; c < bins; c += 64) mx = fmaxf(mx, v[c]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int c = lane; c < bins; c += 64) se += expf(v[c] - mx);
    const float lse = mx + logf(wave_sum(se));
    float loss1 = 0.f, psum = 0.f, values = 0.f;
    for (int c = lane; c < bins; c += 64) {
        const float pr = target(c);
        loss1 -= pr * (v[c] - lse);
        psum += pr;
        values += expf(v[c] - lse) * centre(c);
    }
    loss1 = wave_sum(loss1);
    psum = wave_sum(psum);
    values = wave_sum(values);
    // the clipped prediction and its encoding
    const float old = old_values[r];
    const float diff = values - old;
    const float clipped = old + fminf(fmaxf(diff, -clip), clip);
    const bool through = diff >= -clip && diff <= clip && clipped >= rlo && clipped <= rhi;       // d x / d values = 1
    const float x = fminf(fmaxf(clipped, rlo), rhi);
    int li2 = 0, ri2 = 0;
    float wl2 = 0.f;
    if (TWO_HOT) two_hot_of(x, li2, ri2, wl2);
    const float z2 = TWO_HOT ? 1.f : erff((support[bins] - x) / sigma_sqrt2) - erff((support[0] - x) / sigma_sqrt2);
    const float zc2 = fmaxf(z2, hl_eps);
    // d erf((s - x) / a) / dx = -k exp(-((s - x) / a)^2),  k = 2 / (a sqrt(pi))
    const float k = 1.1283791670955126f / sigma_sqrt2;
    auto gauss = [&](int c) -> float { const float u = (support[c] - x) / sigma_sqrt2; return expf(-u * u); };
    const float dz2 = (TWO_HOT || z2 < hl_eps) ? 0.f : -k * (gauss(bins) - gauss(0));
    float loss2 = 0.f, dl2 = 0.f;                                                                 // loss2 and d loss2 / d x
    for (int c = lane; c < bins; c += 64) {
        const float pr = target(c);
        float q, dq;
        if (TWO_HOT) {
            const float inv = 1.f / (support[ri2] - support[li2]);
            q = c == ri2 ? 1.f - wl2 : (c == li2 ? wl2 : 0.f);
            dq = c == ri2 ? inv : (c == li2 ? -inv : 0.f);
        } else {
            const float num = erff((support[c + 1] - x) / sigma_sqrt2) - erff((support[c] - x) / sigma_sqrt2);
            q = num / zc2;
            dq = -k * (gauss(c + 1) - gauss(c)) / zc2 - num * dz2 / (zc2 * zc2);
        }
        loss2 -= pr * logf(fmaxf(q, 1e-20f));
        if (q >= 1e-20f) dl2 -= pr * dq / q;
    }
    loss2 = wave_sum(loss2);
    dl2 = wave_sum(dl2);
    const float w2 = loss2 > loss1 ? 1.f : (loss2 == loss1 ? 0.5f : 0.f), w1 = 1.f - w2;
    const float g2 = through ? w2 * dl2 : 0.f;                                                    // d loss / d values
    const float scale = mk / count;
    for (int c = lane; c < bins; c += 64) {
        const float pr = target(c);
        const float pc = expf(v[c] - lse);
        dv[(int64_t)r * ld + c] = (w1 * (pc * psum - pr) + g2 * pc * (centre(c) - values)) * scale;
    }
    for (int c = bins + lane; c < ld; c += 64) dv[(int64_t)r * ld + c] = 0.f;
    if (lane == 0) row_loss[r] = fmaxf(loss1, loss2) * mk;
}

// ------------------------------------------------------------------------------------ return statistics (keep_reward_ema_stats)
// D4:5985-6015 in ONE workgroup, nothing read back by the host.  The quantiles are exact order statistics of the kept returns: each float is
// mapped to an unsigned key of the same order (sign bit flipped for positives, all bits for negatives) and the element of rank k is found
// digit by digit, 8 bits per pass: a 256-bin histogram (LDS integer atomics) of the keys that share the digits found so far, a scan, the bin that
// holds rank k.  The four ranks (floor and ceil of both positions) go through the four passes together, one histogram each: 1024 threads = 4 x
// 256 bins for the scan.  Counts are integers and the float sums have a fixed tree order: equal inputs give equal bits.
__device__ __forceinline__ uint32_t order_key(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_key_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float block_sum_1024(float s, float* sh) {
    __syncthreads();
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(1024) void return_stats_kernel(const float* returns, const float* old_values, const float* mask, int64_t n, float* ema,
                                                            float ema_w, float q_lo, float q_hi, float* adv, float* stats) {
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t scan[2][1024];
    __shared__ float shf[1024];
    __shared__ uint32_t s_prefix[4], s_rank[4];
    __shared__ uint32_t s_count;
    const int tid = threadIdx.x;
    if (tid == 0) s_count = 0;
    __syncthreads();
    uint32_t cnt = 0;
    for (int64_t i = tid; i < n; i += 1024) cnt += (!mask || mask[i] != 0.f) ? 1u : 0u;
    atomicAdd(&s_count, cnt);
    __syncthreads();
    const uint32_t N = s_count;
    float mean_e = ema[0], var_e = ema[1];
    if (N > 0) {
        // positions q (N - 1) in double: a float position loses the fraction beyond 2^24 / N
        const double pos_lo = (double)q_lo * (double)(N - 1), pos_hi = (double)q_hi * (double)(N - 1);
        const double fl_lo = floor(pos_lo), fl_hi = floor(pos_hi);
        if (tid == 0) {
            s_rank[0] = (uint32_t)fl_lo; s_rank[1] = (uint32_t)ceil(pos_lo); s_rank[2] = (uint32_t)fl_hi; s_rank[3] = (uint32_t)ceil(pos_hi);
            for (int j = 0; j < 4; ++j) s_prefix[j] = 0;
        }
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t pmask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
            (&hist[0][0])[tid] = 0;
            __syncthreads();
            const uint32_t p0 = s_prefix[0], p1 = s_prefix[1], p2 = s_prefix[2], p3 = s_prefix[3];
            for (int64_t i = tid; i < n; i += 1024) {
                if (mask && mask[i] == 0.f) continue;
                const uint32_t key = order_key(returns[i]), hi = key & pmask, d = (key >> shift) & 255u;
                if (hi == p0) atomicAdd(&hist[0][d], 1u);
                if (hi == p1) atomicAdd(&hist[1][d], 1u);
                if (hi == p2) atomicAdd(&hist[2][d], 1u);
                if (hi == p3) atomicAdd(&hist[3][d], 1u);
            }
            __syncthreads();
            // inclusive scan of each histogram: thread = (rank j, bin b)
            const int b = tid & 255, j = tid >> 8;
            const uint32_t own = (&hist[0][0])[tid];
            int cur = 0;
            scan[0][tid] = own;
            __syncthreads();
            for (int w = 1; w < 256; w <<= 1) {
                const uint32_t t = scan[cur][tid] + (b >= w ? scan[cur][tid - w] : 0u);
                scan[cur ^ 1][tid] = t;
                cur ^= 1;
                __syncthreads();
            }
            const uint32_t incl = scan[cur][tid], excl = incl - own, kj = s_rank[j];
            __syncthreads();
            if (kj >= excl && kj < incl) { s_rank[j] = kj - excl; s_prefix[j] |= (uint32_t)b << shift; }
            __syncthreads();
        }
        const float x0 = order_key_inv(s_prefix[0]), x1 = order_key_inv(s_prefix[1]), x2 = order_key_inv(s_prefix[2]), x3 = order_key_inv(s_prefix[3]);
        // torch.lerp(a, b, w): a + w (b - a) below one half, b - (b - a)(1 - w) from there
        const float w_lo = (float)(pos_lo - fl_lo), w_hi = (float)(pos_hi - fl_hi);
        const float lo = w_lo < 0.5f ? x0 + w_lo * (x1 - x0) : x1 - (x1 - x0) * (1.f - w_lo);
        const float hi = w_hi < 0.5f ? x2 + w_hi * (x3 - x2) : x3 - (x3 - x2) * (1.f - w_hi);
        float s = 0.f;
        for (int64_t i = tid; i < n; i += 1024)
            if (!mask || mask[i] != 0.f) s += fminf(fmaxf(returns[i], lo), hi);
        const float mean = block_sum_1024(s, shf) / (float)N;
        s = 0.f;
        for (int64_t i = tid; i < n; i += 1024)
            if (!mask || mask[i] != 0.f) { const float d = fminf(fmaxf(returns[i], lo), hi) - mean; s += d * d; }
        const float var = block_sum_1024(s, shf) / (float)N;
        mean_e = mean_e + ema_w * (mean - mean_e);                       // lerp_ (weight below one half)
        var_e = var_e + ema_w * (var - var_e);
        __syncthreads();                                                 // every thread has read ema[] before it is written
        if (tid == 0) { ema[0] = mean_e; ema[1] = var_e; stats[0] = lo; stats[1] = hi; stats[2] = mean; stats[3] = var; }
    } else if (tid == 0) {
        stats[0] = stats[1] = stats[2] = stats[3] = 0.f;
    }
    const float sd = sqrtf(fmaxf(var_e, 1e-5f));
    for (int64_t i = tid; i < n; i += 1024) adv[i] = (returns[i] - mean_e) / sd - (old_values[i] - mean_e) / sd;
}

int return_stats(const float* returns, const float* old_values, const float* mask, int64_t n, float* ema, double reward_ema_decay, float q_lo, float q_hi,
                 float* adv, float* stats, hipStream_t s) {
    float w = (float)(1. - reward_ema_decay);
    // torch's lerp takes its other branch from one half on; the kernel has the lower one only (a decay above one half, as any EMA has)
    D4_REQUIRE(w < 0.5f, "return statistics: reward_ema_decay must exceed 0.5");
    hipLaunchKernelGGL(return_stats_kernel, dim3(1), dim3(1024), 0, s, returns, old_values, mask, n, ema, w, q_lo, q_hi, adv, stats);
    D4_LAUNCH_CHECK();
    return 0;
}

__global__ void masked_mean_final_kernel(const float* scal, float* out) { out[0] = scal[7] / fmaxf(scal[1], 1.f); }

__global__ void finalize_losses_kernel(const float* scal, float* losses, int objective, float ent_w, float kl_w) {
    // scal: [1] count, [4] sum pl, [5] sum ent, [6] sum aux(kl), [7] sum value loss
    const float count = fmaxf(scal[1], 1.f);
    float pl = scal[4] / count;
    if (objective == 2) pl += kl_w * scal[6] / count;
    losses[0] = pl + ent_w * scal[5] / count;
    losses[1] = scal[7] / count;
}

// The policy branch's loss as one sequence (learn() and the stateless entry d4_policy_loss both run it, so the two cannot drift): the masked
// advantage statistics scal[0..2] (sum adv * mask, count, sum of squared differences; each all-reduced where a callback is given), the fused
// forward + backward kernel, and the row sums scal[4..6].  scal is zeroed by the caller, who also finalises (learn() adds the value branch's
// sum first).
static int policy_loss_run(const PolicyLossArgs& p, float* scal, int (*allreduce_sum)(float*, int, void*), void* allreduce_user, hipStream_t s) {
    int rc;
    const int64_t R = p.R;
    hipLaunchKernelGGL(reduce1_kernel<RED_PROD>, dim3(1), dim3(1024), 0, s, p.adv_raw, p.mask, scal, R, scal + 0);
    hipLaunchKernelGGL(reduce1_kernel<RED_SUM>, dim3(1), dim3(1024), 0, s, p.mask, nullptr, scal, R, scal + 1);
    D4_LAUNCH_CHECK();
    if (allreduce_sum && (rc = allreduce_sum(scal, 2, allreduce_user))) { set_error("allreduce callback failed (%d)", rc); return 5; }
    hipLaunchKernelGGL(reduce1_kernel<RED_SQDIFF_MASKED>, dim3(1), dim3(1024), 0, s, p.adv_raw, p.mask, scal, R, scal + 2);
    D4_LAUNCH_CHECK();
    if (allreduce_sum && (rc = allreduce_sum(scal + 2, 1, allreduce_user))) { set_error("allreduce callback failed (%d)", rc); return 5; }
    hipLaunchKernelGGL(policy_loss_kernel, dim3(cdiv(p.R, 128)), dim3(128), 0, s, p);
    D4_LAUNCH_CHECK();
    hipLaunchKernelGGL(reduce1_kernel<RED_SUM>, dim3(1), dim3(1024), 0, s, p.row_pl, nullptr, scal, R, scal + 4);
    hipLaunchKernelGGL(reduce1_kernel<RED_SUM>, dim3(1), dim3(1024), 0, s, p.row_ent, nullptr, scal, R, scal + 5);
    hipLaunchKernelGGL(reduce1_kernel<RED_SUM>, dim3(1), dim3(1024), 0, s, p.row_aux, nullptr, scal, R, scal + 6);
    D4_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------ MLP backward pieces
__global__ void silu_bwd_kernel(const float* dy, const float* z, float* dz, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float s = sigmoidf(z[i]);
        dz[i] = dy[i] * s * (1.f + z[i] * (1.f - s));
    }
}

// RMSNorm backward, one wave per row:  xhat = x * rstd * gamma
//   tg[r][k] = dxhat * x * rstd   (column-summed afterwards -> dgamma)
//   dx[r][k] = rstd * (gamma * dxhat - x * rstd^2 * mean_k(gamma * dxhat * x))
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const float* x, const float* dxhat, const float* gamma, float* tg, float* dx,
                                                          int rows, int d, float eps) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* xr = x + (int64_t)r * d;
    const float* gr = dxhat + (int64_t)r * d;
    float ss = 0.f, dot = 0.f;
    for (int c = lane; c < d; c += 64) { const float v = xr[c]; ss += v * v; dot += gamma[c] * gr[c] * v; }
    const float rstd = rsqrtf(wave_sum(ss) / (float)d + eps);
    dot = wave_sum(dot) / (float)d;
    for (int c = lane; c < d; c += 64) {
        const float v = xr[c], g = gr[c];
        tg[(int64_t)r * d + c] = g * v * rstd;
        if (dx) dx[(int64_t)r * d + c] = rstd * (gamma[c] * g - v * rstd * rstd * dot);
    }
}

int rmsnorm_bwd(const float* x, const float* dxhat, const float* gamma, float* tg, float* dx, int rows, int d, float eps, hipStream_t s) {
    if (rows == 0) return 0;
    hipLaunchKernelGGL(rmsnorm_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, x, dxhat, gamma, tg, dx, rows, d, eps);
    D4_LAUNCH_CHECK();
    return 0;
}

// Backward through a = silu(y), y = LayerNorm(z) * g + b (one wave per row, z recomputed into zhat):
//   dy = da * silu'(y);  tg = dy * zhat, tb = dy (column-summed afterwards -> dg, db_norm)
//   dz = rstd * (g dy - mean(g dy) - zhat * mean(g dy zhat))
__global__ __launch_bounds__(256) void layernorm_silu_bwd_kernel(const float* z, int ldz, const float* da, const float* g, const float* b,
                                                                 float* tg, float* tb, float* dz, int rows, int d, float eps) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* zr = z + (int64_t)r * ldz;
    float sum = 0.f;
    for (int c = lane; c < d; c += 64) sum += zr[c];
    const float mean = wave_sum(sum) / (float)d;
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) { const float t = zr[c] - mean; ss += t * t; }
    const float rstd = rsqrtf(wave_sum(ss) / (float)d + eps);
    float m1 = 0.f, m2 = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float zh = (zr[c] - mean) * rstd;
        const float y = zh * g[c] + b[c];
        const float sg = sigmoidf(y);
        const float dy = da[(int64_t)r * d + c] * sg * (1.f + y * (1.f - sg));
        tg[(int64_t)r * d + c] = dy * zh;
        tb[(int64_t)r * d + c] = dy;
        const float gd = g[c] * dy;
        m1 += gd; m2 += gd * zh;
    }
    m1 = wave_sum(m1) / (float)d; m2 = wave_sum(m2) / (float)d;
    for (int c = lane; c < d; c += 64) {
        const float zh = (zr[c] - mean) * rstd;
        const float gd = g[c] * tb[(int64_t)r * d + c];
        dz[(int64_t)r * ldz + c] = rstd * (gd - m1 - zh * m2);
    }
}

static inline dim3 grid1d(int64_t n) {
    int64_t g = (n + 255) / 256;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return dim3((unsigned)g);
}
static int silu_bwd(const float* dy, const float* z, float* dz, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(silu_bwd_kernel, grid1d(n), dim3(256), 0, s, dy, z, dz, n);
    D4_LAUNCH_CHECK();
    return 0;
}
static int layernorm_silu_bwd(const float* z, int ldz, const float* da, const float* g, const float* b, float* tg, float* tb, float* dz, int rows, int d,
                              float eps, hipStream_t s) {
    hipLaunchKernelGGL(layernorm_silu_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, z, ldz, da, g, b, tg, tb, dz, rows, d, eps);
    D4_LAUNCH_CHECK();
    return 0;
}

// dW[M][N] = A^T B over R rows (weight gradient of a head Linear)
static int gemm_dw_l(d4_engine* e, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int R, hipStream_t s) {
    if (gemm_tn_applicable(A, lda, B, ldb, C, ldc, M, N, R)) return gemm_tn(A, lda, B, ldb, C, ldc, M, N, R, e->l_dwpart, e->l_dwpart ? L_DWPART_FLOATS : 0, s);
    GemmArgs g{A, lda, B, ldb, C, ldc, nullptr, nullptr, 0, M, N, R, GEMM_TRANS_A | GEMM_TRANS_B, 0.f};
    return gemm(g, s);
}

static int gemm_l(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K, int flags, hipStream_t s) {
    GemmArgs g{A, lda, W, ldw, C, ldc, nullptr, nullptr, 0, M, N, K, flags, 0.f};
    return gemm(g, s);
}

// Backward of mlp_forward(save=...).  dout: [R][dims[nl]] gradient of the (un-activated) output.
// dx0 (optional, [R][dims[0]]): gradient with respect to the MLP's INPUT (the agent embeddings), for fine-tuning the whole world model
static int mlp_backward(d4_engine* e, const Mlp& m, const float* save, int R, const float* dout, int ld_dout, hipStream_t s, float* dx0 = nullptr) {
    int rc;
    float* sx[9]; float* sxh[9]; float* sz[9];
    for (int i = 0; i < m.nl; ++i) m.save_ptrs(const_cast<float*>(save), R, i, &sx[i], &sxh[i], &sz[i]);
    float* dy = e->l_tmp[0]; float* dz = e->l_tmp[1]; float* dxh = e->l_tmp[2];
    const float* cur = dout;
    const bool pre = m.recipe == D4_MLP_PRE_RMS;
    for (int i = m.nl - 1; i >= 0; --i) {
        const int din = m.dims[i], dout_i = m.dims[i + 1];
        const float* dzp;
        int ldd = dout_i;
        D4_REQUIRE(m.db[i] && m.dw[i], "learner: head parameters were bound without gradient buffers");
        if (i == m.nl - 1) { dzp = cur; ldd = ld_dout; }
        else if (m.post_norm(i)) {
            // through silu and the LayerNorm: tg / tb (per-row terms of the norm's weight / bias gradients) use dxh and dy's buffers
            D4_REQUIRE(m.dg[i] && m.dnb[i], "learner: head parameters were bound without gradient buffers");
            const int ldz = m.ldz(i);
            float* tg = dxh; float* tb = dz; float* dzo = e->l_tmp[3];        // cur (= dy, the incoming gradient) stays intact while it is read
            if ((rc = layernorm_silu_bwd(sz[i], ldz, cur, m.g[i], m.nb[i], tg, tb, dzo, R, dout_i, 1e-5f, s))) return rc;
            if ((rc = colsum(tg, dout_i, R, dout_i, m.dg[i], s))) return rc;
            if ((rc = colsum(tb, dout_i, R, dout_i, m.dnb[i], s))) return rc;
            dzp = dzo; ldd = ldz;
        } else {
            if ((rc = silu_bwd(cur, sz[i], dz, (int64_t)R * dout_i, s))) return rc;
            dzp = dz;
        }
        if ((rc = colsum(dzp, ldd, R, dout_i, m.db[i], s))) return rc;
        const float* lin_in = pre ? sxh[i] : sx[i];
        // input gradients go through a transposed image of the weight (gemm_dx; scratch shared with the weight gradient's partial products,
        // used one after the other on the stream)
        float* wt = (e->l_dwpart && (size_t)dout_i * din <= L_DWPART_FLOATS) ? e->l_dwpart : nullptr;
        // dW[n][k] = sum_r dz[r][n] * lin_in[r][k]
        if ((rc = gemm_dw_l(e, dzp, ldd, lin_in, din, m.dw[i], din, dout_i, din, R, s))) return rc;
        if (!pre) {
            // dx[r][k] = sum_n dz[r][n] * W[n][k] is the previous layer's activation gradient directly
            if (i > 0 && (rc = gemm_dx(dzp, ldd, m.w[i], din, dy, din, R, din, dout_i, wt, s))) return rc;
            if (i == 0 && dx0 && (rc = gemm_dx(dzp, ldd, m.w[i], din, dx0, din, R, din, dout_i, wt, s))) return rc;
            cur = dy;
            continue;
        }
        D4_REQUIRE(m.dg[i], "learner: head parameters were bound without gradient buffers");
        // dxhat[r][k] = sum_n dz[r][n] * W[n][k]
        if ((rc = gemm_dx(dzp, ldd, m.w[i], din, dxh, din, R, din, dout_i, wt, s))) return rc;
        // through the RMSNorm; dy of the previous layer overwrites e->l_tmp[0]; tg reuses dz (dz is dead after the GEMMs)
        float* tg = dz;
        hipLaunchKernelGGL(rmsnorm_bwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, sx[i], dxh, m.g[i], tg, i > 0 ? dy : dx0, R, din, RMS_EPS_L);
        D4_LAUNCH_CHECK();
        if ((rc = colsum(tg, din, R, din, m.dg[i], s))) return rc;
        cur = dy;
    }
    return 0;
}

// A rank whose trajectory shard is EMPTY (a global batch smaller than the number of ranks, or an uneven split): it has nothing to learn from but must
// take part in every collective of the step with a zero contribution, in the order the other ranks issue them (three statistics all-reduces here, the
// gradient all-reduce of each head in the caller), and ends up with the global losses and zero local gradients.
static int learn_empty_shard(d4_engine* e, const d4_learn_io* io, hipStream_t s) {
    const d4_config& c = e->c;
    int rc;
    float* scal = e->l_scal;
    D4_REQUIRE(e->LR > 0 && scal, "learn: an empty shard still needs an engine created with max_learn_rows >= 1 (the learner's scalar workspace)");
    D4_HIP(hipMemsetAsync(scal, 0, 64 * sizeof(float), s));
    if ((rc = io->allreduce_sum(scal, 2, io->allreduce_user)) || (rc = io->allreduce_sum(scal + 2, 1, io->allreduce_user)) ||
        (rc = io->allreduce_sum(scal + 4, 4, io->allreduce_user))) { set_error("allreduce callback failed (%d)", rc); return 5; }
    hipLaunchKernelGGL(finalize_losses_kernel, dim3(1), dim3(1), 0, s, scal, io->losses, io->objective, c.policy_entropy_weight,
                       io->objective == 2 ? c.pmpo_kl_div_loss_weight : 0.f);
    D4_LAUNCH_CHECK();
    for (const Mlp* m : {&e->policy, &e->value})
        for (int i = 0; i < m->nl; ++i) {
            const int din = m->dims[i], dout = m->dims[i + 1];
            D4_REQUIRE(m->db[i] && m->dw[i], "learner: head parameters were bound without gradient buffers");
            if ((rc = fill_f32(m->dw[i], 0.f, (int64_t)dout * din, s)) || (rc = fill_f32(m->db[i], 0.f, dout, s))) return rc;
            if (m->dg[i] && (rc = fill_f32(m->dg[i], 0.f, m->post_norm(i) ? dout : din, s))) return rc;
            if (m->dnb[i] && (rc = fill_f32(m->dnb[i], 0.f, dout, s))) return rc;
        }
    const int64_t mtp4d = (int64_t)c.multi_token_pred_len * 4 * e->D;
    if (e->na > 0 && e->action_unembed_grad && (rc = fill_f32(e->action_unembed_grad, 0.f, e->A * mtp4d, s))) return rc;
    if (e->nc > 0 && e->cont_unembed_grad && (rc = fill_f32(e->cont_unembed_grad, 0.f, 2 * e->nc * mtp4d, s))) return rc;
    return 0;
}

int learn(d4_engine* e, const d4_learn_io* io, hipStream_t s) {
    const d4_config& c = e->c;
    D4_REQUIRE(e->prepared, "engine not prepared");
    const int B = io->batch, T = io->time, R = B * T;
    D4_REQUIRE(io->objective >= 0 && io->objective <= 2, "unknown objective %d  [D4:6215]", io->objective);
    if (R == 0 && io->allreduce_sum && io->losses) return learn_empty_shard(e, io, s);
    D4_REQUIRE(R > 0 && R <= e->LR, "learn: %d rows exceed max_learn_rows %d", R, e->LR);
    D4_REQUIRE(io->agent_embed && io->old_values && io->rewards && io->losses && (e->na == 0 || (io->actions && io->old_log_probs)) &&
               (e->nc == 0 || (io->actions_cont && io->old_log_probs_cont)),
               "the generations need to contain the log probs, values, and rewards for policy optimization  [D4:5935]");
    D4_REQUIRE(io->objective >= 0 && io->objective <= 2, "unknown objective %d  [D4:6215]", io->objective);
    const int D = e->D, A = e->A, Apad = (A + 3) / 4 * 4 + (A == 0 ? 4 : 0), na = e->na, nc = e->nc, Cpad = (2 * nc + 3) / 4 * 4 + (nc == 0 ? 4 : 0);
    int rc;
    float* scal = e->l_scal;
    const bool need_vold = io->ema_returns || io->clip_values;
    D4_REQUIRE(!(io->ema_returns && io->allreduce_sum), "learn: keep_reward_ema_stats is single-process only (the return quantiles are not reduced over ranks)  [D4:5999]");
    D4_REQUIRE(!io->ema_returns || (io->q_lo >= 0.f && io->q_lo <= io->q_hi && io->q_hi <= 1.f && io->reward_ema_decay > 0.5 && io->reward_ema_decay <= 1.),
               "learn: 0 <= q_lo <= q_hi <= 1 and 0.5 < reward_ema_decay <= 1");
    D4_REQUIRE(!io->clip_values || io->value_clip >= 0.f, "learn: value_clip >= 0");
    D4_REQUIRE(!need_vold || e->l_oldv, "learn: no workspace for the old values");
    D4_HIP(hipMemsetAsync(scal, 0, 64 * sizeof(float), s));

    // ---- returns, advantages, masks
    float* row_a = e->l_adv;                        // raw advantage [R]
    float* mask_keep = e->l_mask;                   // learnable-step mask [R]
    hipLaunchKernelGGL(gae_kernel, dim3(cdiv(B, 128)), dim3(128), 0, s, io->rewards, io->old_values, io->lens, io->is_truncated,
                       io->terminals, c.gae_discount_factor, c.gae_lambda, B, T, e->l_returns, row_a, mask_keep);
    D4_LAUNCH_CHECK();
    if (need_vold) {      // the old values as the reference's later steps see them: 0 past `len` (D4:5950); launched with an option on only
        hipLaunchKernelGGL(masked_old_values_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, io->old_values, io->lens, B, T, e->l_oldv);
        D4_LAUNCH_CHECK();
    }
    if (io->returns) D4_HIP(hipMemcpyAsync(io->returns, e->l_returns, sizeof(float) * R, hipMemcpyDeviceToDevice, s));
    // keep_reward_ema_stats: the EMA pair is updated on the stream and the advantage is formed from the normalised returns and old values
    // (D4:5985-6015); scal[40..43] = lo, hi, mean, var
    if (io->ema_returns && (rc = return_stats(e->l_returns, e->l_oldv, mask_keep, R, io->ema_returns, io->reward_ema_decay, io->q_lo, io->q_hi, row_a, scal + 40, s))) return rc;

    const int normalize = io->normalize_advantages < 0 ? (io->objective != 2) : io->normalize_advantages;

    // ---- policy head forward (saved), logits of prediction head 0
    float* save_p = e->l_save;
    float* save_v = e->l_save + e->policy.save_floats(R);
    float* pe = e->l_tmp[0];
    if ((rc = mlp_forward(e, e->policy, io->agent_embed, D, R, pe, 4 * D, save_p, s))) return rc;
    if ((rc = fill_f32(e->l_logits, 0.f, (int64_t)R * Apad, s))) return rc;
    if (na > 0) {
        GemmArgs g{pe, 4 * D, e->action_unembed, c.multi_token_pred_len * 4 * D, e->l_logits, Apad, nullptr, nullptr, 0, R, A, 4 * D, 0, 0.f};
        if ((rc = gemm(g, s))) return rc;
    }
    if (nc > 0) {      // raw Beta parameters of prediction head 0 (head-0 slice of the [nc][mtp][4D][2] parameter as a GEMM weight)
        if ((rc = cunembed_gather(e->cont_unembed, e->cu_w, nc, c.multi_token_pred_len, 4 * D, s))) return rc;
        if ((rc = fill_f32(e->l_cparams, 0.f, (int64_t)R * Cpad, s))) return rc;
        GemmArgs g{pe, 4 * D, e->cu_w, 4 * D, e->l_cparams, Cpad, nullptr, nullptr, 0, R, 2 * nc, 4 * D, 0, 0.f};
        if ((rc = gemm(g, s))) return rc;
    }
    float* row_pl = e->l_rows, *row_ent = e->l_rows + R, *row_aux = e->l_rows + 2 * R, *row_vl = e->l_rows + 3 * R;
    {
        PolicyLossArgs p{};
        p.logits = e->l_logits; p.ld = Apad; p.actions = io->actions; p.old_lp = io->old_log_probs;
        p.old_logits = io->old_action_logits; p.ldo = A; p.adv_raw = row_a; p.mask = mask_keep; p.scal = scal;
        p.action_sizes = e->action_sizes; p.dlogits = e->l_dlogits; p.row_pl = row_pl; p.row_ent = row_ent; p.row_aux = row_aux;
        p.cparams = e->l_cparams; p.ldc = Cpad; p.actions_cont = io->actions_cont; p.old_lp_cont = io->old_log_probs_cont;
        p.old_cparams = io->old_cont_params; p.dcparams = e->l_dcparams; p.nc = nc; p.beta_param = e->c.continuous_beta_param;
        p.R = R; p.na = na; p.A = A; p.objective = io->objective; p.normalize = normalize;
        p.use_gate = io->use_delight_gating < 0 ? c.use_delight_gating : io->use_delight_gating;
        p.reverse_kl = c.pmpo_reverse_kl;
        p.eps = io->eps; p.clip = c.ppo_eps_clip; p.ent_w = c.policy_entropy_weight;
        p.gate_temp = io->delight_temperature > 0.f ? io->delight_temperature : c.delight_temperature;
        p.pmpo_alpha = c.pmpo_pos_to_neg_weight;
        p.kl_w = io->objective == 2 ? c.pmpo_kl_div_loss_weight : 0.f;
        D4_REQUIRE(!(p.kl_w > 0.f) || ((na == 0 || io->old_action_logits) && (nc == 0 || io->old_cont_params)), "pmpo with a KL weight needs old_action_unembeds  [D4:6160-6170]");
        // advantage statistics, the fused loss kernel and its row sums
        if ((rc = policy_loss_run(p, scal, io->allreduce_sum, io->allreduce_user, s))) return rc;
    }
    // ---- value head forward (saved) + HL-Gauss cross entropy
    const int vld = (c.value_num_bins + 3) / 4 * 4;
    if ((rc = mlp_forward(e, e->value, io->agent_embed, D, R, e->l_vbins, vld, save_v, s))) return rc;
    {
        const float sigma = c.hl_gauss_sigma_to_bin_ratio * (c.value_max - c.value_min) / (float)c.value_num_bins;
        if (io->clip_values) {
            if (c.reward_encoder_type == 1)
                hipLaunchKernelGGL(value_loss_clip_kernel<true>, dim3(cdiv(R, 4)), dim3(256), 0, s, e->l_vbins, vld, e->l_returns, e->l_oldv, mask_keep, scal,
                                   e->value_support, R, c.value_num_bins, sqrtf(2.f) * sigma, c.hl_gauss_eps, c.value_min, c.value_max, io->value_clip, e->l_dvbins, row_vl);
            else
                hipLaunchKernelGGL(value_loss_clip_kernel<false>, dim3(cdiv(R, 4)), dim3(256), 0, s, e->l_vbins, vld, e->l_returns, e->l_oldv, mask_keep, scal,
                                   e->value_support, R, c.value_num_bins, sqrtf(2.f) * sigma, c.hl_gauss_eps, c.value_min, c.value_max, io->value_clip, e->l_dvbins, row_vl);
        } else if (c.reward_encoder_type == 1)
            hipLaunchKernelGGL(value_loss_kernel<true>, dim3(cdiv(R, 4)), dim3(256), 0, s, e->l_vbins, vld, e->l_returns, mask_keep, scal,
                               e->value_support, R, c.value_num_bins, sqrtf(2.f) * sigma, c.hl_gauss_eps, c.value_min, c.value_max, e->l_dvbins, row_vl);
        else
            hipLaunchKernelGGL(value_loss_kernel<false>, dim3(cdiv(R, 4)), dim3(256), 0, s, e->l_vbins, vld, e->l_returns, mask_keep, scal,
                               e->value_support, R, c.value_num_bins, sqrtf(2.f) * sigma, c.hl_gauss_eps, c.value_min, c.value_max, e->l_dvbins, row_vl);
        D4_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(reduce1_kernel<RED_SUM>, dim3(1), dim3(1024), 0, s, row_vl, nullptr, scal, (int64_t)R, scal + 7);
    D4_LAUNCH_CHECK();
    if (io->allreduce_sum && (rc = io->allreduce_sum(scal + 4, 4, io->allreduce_user))) { set_error("allreduce callback failed (%d)", rc); return 5; }
    hipLaunchKernelGGL(finalize_losses_kernel, dim3(1), dim3(1), 0, s, scal, io->losses, io->objective, c.policy_entropy_weight,
                       io->objective == 2 ? c.pmpo_kl_div_loss_weight : 0.f);
    D4_LAUNCH_CHECK();

    // ---- backward: unembed head 0, policy MLP, value MLP
    const int mtp4d = c.multi_token_pred_len * 4 * D;
    // pe (policy MLP output) was saved as the last layer's z
    float *pe_x, *pe_xh, *pe_saved;
    e->policy.save_ptrs(save_p, R, e->policy.nl - 1, &pe_x, &pe_xh, &pe_saved);
    float* dpe = e->l_dpe;
    if (na > 0) {
        D4_REQUIRE(e->action_unembed_grad, "learner: discrete_action_unembed was bound without a gradient buffer");
        if ((rc = fill_f32(e->action_unembed_grad, 0.f, (int64_t)A * mtp4d, s))) return rc;
        // dU0[a][k] = sum_r dlogits[r][a] * pe[r][k]
        if ((rc = gemm_dw_l(e, e->l_dlogits, Apad, pe_saved, 4 * D, e->action_unembed_grad, mtp4d, A, 4 * D, R, s))) return rc;
        // dpe[r][k] = sum_a dlogits[r][a] * U0[a][k]      (K = Apad; pad rows of U0 are never read: mask K to A)
        if ((rc = gemm_l(e->l_dlogits, Apad, e->action_unembed, mtp4d, dpe, 4 * D, R, 4 * D, A, GEMM_TRANS_B, s))) return rc;
    }
    if (nc > 0) {
        D4_REQUIRE(e->cont_unembed_grad, "learner: continuous_action_unembed was bound without a gradient buffer");
        // d cu_w[j][k] = sum_r dcparams[r][j] * pe[r][k], scattered back into the [nc][mtp][4D][2] layout (other heads: zero)
        if ((rc = gemm_dw_l(e, e->l_dcparams, Cpad, pe_saved, 4 * D, e->l_cu_g, 4 * D, 2 * nc, 4 * D, R, s))) return rc;
        if ((rc = cunembed_scatter_grad(e->l_cu_g, e->cont_unembed_grad, nc, c.multi_token_pred_len, 4 * D, s))) return rc;
        // dpe (+)= dcparams . cu_w
        if ((rc = gemm_l(e->l_dcparams, Cpad, e->cu_w, 4 * D, dpe, 4 * D, R, 4 * D, 2 * nc, GEMM_TRANS_B | (na > 0 ? GEMM_ACCUMULATE : 0), s))) return rc;
    }
    if ((rc = mlp_backward(e, e->policy, save_p, R, dpe, 4 * D, s, io->d_agent_embed_policy))) return rc;
    if ((rc = mlp_backward(e, e->value, save_v, R, e->l_dvbins, vld, s, io->d_agent_embed_value))) return rc;
    return 0;
}

// ------------------------------------------------------------------------------------ clip_grad_norm_ + AdamW
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* g, int64_t n, float* partial) {
    __shared__ float sh[256];
    float s = 0.f;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += g[i] * g[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256) void norm_final_kernel(const float* partial, int np, float grad_scale, float* norm_out) {
    __shared__ float sh[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) s += partial[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *norm_out = sqrtf(sh[0]) * grad_scale;
}

__global__ void adamw_kernel(float* p, const float* g, float* m, float* v, int64_t n, const float* norm, float max_norm,
                             float grad_scale, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2) {
    float coef = grad_scale;
    if (max_norm > 0.f) {
        const float c = max_norm / (*norm + 1e-6f);           // torch.nn.utils.clip_grad_norm_
        coef *= c < 1.f ? c : 1.f;
    }
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * coef;
        float pi = p[i] * (1.f - lr * wd);
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) / sqrtf(bc2) + eps;
        p[i] = pi - (lr / bc1) * (mi / denom);
    }
}

}  // namespace d4

extern "C" {

int d4_gae(const float* rewards, const float* values, const int64_t* lens, const uint8_t* is_truncated,
           const uint8_t* terminals, float gamma, float lam, int batch, int time, float* returns, void* stream) {
    D4_REQUIRE(rewards && values && returns, "null argument");
    hipLaunchKernelGGL(d4::gae_kernel, dim3(d4::cdiv(batch, 128)), dim3(128), 0, static_cast<hipStream_t>(stream), rewards, values, lens,
                       is_truncated, terminals, gamma, lam, batch, time, returns, (float*)nullptr, (float*)nullptr);
    D4_LAUNCH_CHECK();
    return 0;
}

// d4_gae with the two further outputs the learner consumes: adv = returns - values (values read as 0 past `len`) and the learnable-step mask.
int d4_gae_adv(const float* rewards, const float* values, const int64_t* lens, const uint8_t* is_truncated, const uint8_t* terminals, float gamma,
               float lam, int batch, int time, float* returns, float* adv, float* mask, void* stream) {
    D4_REQUIRE(rewards && values && returns && adv && mask, "d4_gae_adv: null argument");
    D4_REQUIRE(batch >= 1 && time >= 1, "d4_gae_adv: batch >= 1 and time >= 1");
    hipLaunchKernelGGL(d4::gae_kernel, dim3(d4::cdiv(batch, 128)), dim3(128), 0, static_cast<hipStream_t>(stream), rewards, values, lens,
                       is_truncated, terminals, gamma, lam, batch, time, returns, adv, mask);
    D4_LAUNCH_CHECK();
    return 0;
}

// Stateless form of the value branch's loss (D4:6254-6295: HL-Gauss / two-hot targets of the returns, cross entropy against the value bins,
// mean over the learnable steps), forward + backward in one call:  loss[0] = sum_r mask[r] * CE_r / max(sum mask, 1),  dlogits = d loss / d logits.
// support: [bins + 1] bin edges (HL-Gauss) or [bins] bin values (two-hot), device.  mask: [rows] or null (all rows).  scratch >= 2 * rows + 64 floats.
int d4_hl_gauss_ce(const float* logits, int ld, const float* targets, const float* mask, const float* support, int rows, int bins, float vmin,
                   float vmax, float sigma, float eps, int two_hot, float* loss, float* dlogits, float* scratch, void* stream) {
    D4_REQUIRE(logits && targets && support && loss && dlogits && scratch && rows >= 1 && bins >= 1 && ld >= bins, "d4_hl_gauss_ce: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* scal = scratch;                     // [64]: [1] count, [7] summed row losses
    float* ones = scratch + 64;                // [rows]
    float* row_loss = ones + rows;             // [rows]
    D4_HIP(hipMemsetAsync(scal, 0, 64 * sizeof(float), s));
    if (!mask) { if (int rc = d4::fill_f32(ones, 1.f, rows, s)) return rc; mask = ones; }
    hipLaunchKernelGGL(d4::reduce1_kernel<d4::RED_SUM>, dim3(1), dim3(1024), 0, s, mask, (const float*)nullptr, scal, (int64_t)rows, scal + 1);
    if (two_hot)
        hipLaunchKernelGGL(d4::value_loss_kernel<true>, dim3(d4::cdiv(rows, 4)), dim3(256), 0, s, logits, ld, targets, mask, scal, support, rows, bins,
                           sqrtf(2.f) * sigma, eps, vmin, vmax, dlogits, row_loss);
    else
        hipLaunchKernelGGL(d4::value_loss_kernel<false>, dim3(d4::cdiv(rows, 4)), dim3(256), 0, s, logits, ld, targets, mask, scal, support, rows, bins,
                           sqrtf(2.f) * sigma, eps, vmin, vmax, dlogits, row_loss);
    hipLaunchKernelGGL(d4::reduce1_kernel<d4::RED_SUM>, dim3(1), dim3(1024), 0, s, row_loss, (const float*)nullptr, scal, (int64_t)rows, scal + 7);
    hipLaunchKernelGGL(d4::masked_mean_final_kernel, dim3(1), dim3(1), 0, s, scal, loss);
    D4_LAUNCH_CHECK();
    return 0;
}

// Stateless form of the return statistics (D4:5985-6015): the kernel d4_learn launches when io->ema_returns is given.
int d4_return_stats(const float* returns, const float* old_values, const float* mask, int64_t n, float* ema, double reward_ema_decay, float q_lo,
                    float q_hi, float* adv, float* stats, void* stream) {
    D4_REQUIRE(returns && old_values && ema && adv && stats, "d4_return_stats: null argument");
    D4_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "d4_return_stats: 1 <= n < 2^31");
    D4_REQUIRE(q_lo >= 0.f && q_lo <= q_hi && q_hi <= 1.f, "d4_return_stats: 0 <= q_lo <= q_hi <= 1");
    D4_REQUIRE(reward_ema_decay > 0.5 && reward_ema_decay <= 1., "d4_return_stats: 0.5 < reward_ema_decay <= 1");
    return d4::return_stats(returns, old_values, mask, n, ema, reward_ema_decay, q_lo, q_hi, adv, stats, static_cast<hipStream_t>(stream));
}

// Stateless form of the value branch's loss with the clipping option (D4:6254-6295).  clip_values = 0 launches what d4_hl_gauss_ce
// launches, on the caller's row_loss.
int d4_value_loss(const d4_value_loss_desc* d, void* stream) {
    D4_REQUIRE(d, "d4_value_loss: null argument");
    D4_REQUIRE(d->logits && d->returns && d->support && d->loss && d->row_loss && d->dlogits && d->scratch, "d4_value_loss: null argument");
    D4_REQUIRE(d->rows >= 1 && d->bins >= 1 && d->ld >= d->bins, "d4_value_loss: rows >= 1, bins >= 1, ld >= bins");
    D4_REQUIRE(!d->clip_values || (d->old_values && d->value_clip >= 0.f && (!d->two_hot || d->bins >= 2)), "d4_value_loss: clipping needs old_values, value_clip >= 0 and, two-hot, two bins");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rows = d->rows, bins = d->bins;
    float* scal = d->scratch;                  // [64]: [1] count, [7] summed row losses
    float* ones = d->scratch + 64;             // [rows]
    const float* mask = d->mask;
    const float a = sqrtf(2.f) * d->sigma;
    D4_HIP(hipMemsetAsync(scal, 0, 64 * sizeof(float), s));
    if (!mask) { if (int rc = d4::fill_f32(ones, 1.f, rows, s)) return rc; mask = ones; }
    hipLaunchKernelGGL(d4::reduce1_kernel<d4::RED_SUM>, dim3(1), dim3(1024), 0, s, mask, (const float*)nullptr, scal, (int64_t)rows, scal + 1);
    if (d->clip_values) {
        if (d->two_hot)
            hipLaunchKernelGGL(d4::value_loss_clip_kernel<true>, dim3(d4::cdiv(rows, 4)), dim3(256), 0, s, d->logits, d->ld, d->returns, d->old_values, mask, scal, d->support,
                               rows, bins, a, d->eps, d->vmin, d->vmax, d->value_clip, d->dlogits, d->row_loss);
        else
            hipLaunchKernelGGL(d4::value_loss_clip_kernel<false>, dim3(d4::cdiv(rows, 4)), dim3(256), 0, s, d->logits, d->ld, d->returns, d->old_values, mask, scal, d->support,
                               rows, bins, a, d->eps, d->vmin, d->vmax, d->value_clip, d->dlogits, d->row_loss);
    } else if (d->two_hot)
        hipLaunchKernelGGL(d4::value_loss_kernel<true>, dim3(d4::cdiv(rows, 4)), dim3(256), 0, s, d->logits, d->ld, d->returns, mask, scal, d->support, rows, bins,
                           a, d->eps, d->vmin, d->vmax, d->dlogits, d->row_loss);
    else
        hipLaunchKernelGGL(d4::value_loss_kernel<false>, dim3(d4::cdiv(rows, 4)), dim3(256), 0, s, d->logits, d->ld, d->returns, mask, scal, d->support, rows, bins,
                           a, d->eps, d->vmin, d->vmax, d->dlogits, d->row_loss);
    hipLaunchKernelGGL(d4::reduce1_kernel<d4::RED_SUM>, dim3(1), dim3(1024), 0, s, d->row_loss, (const float*)nullptr, scal, (int64_t)rows, scal + 7);
    hipLaunchKernelGGL(d4::masked_mean_final_kernel, dim3(1), dim3(1), 0, s, scal, d->loss);
    D4_LAUNCH_CHECK();
    return 0;
}

// Stateless form of the whole policy branch's loss (D4:5985-6242; test / tooling use): fills PolicyLossArgs from the descriptor
// and runs policy_loss_run, the sequence d4_learn runs, then finalize_losses_kernel.  Everything is refused before the first launch.
int d4_policy_loss(const d4_policy_loss_desc* d, void* stream) {
    D4_REQUIRE(d, "d4_policy_loss: null argument");
    D4_REQUIRE(d->advantages && d->loss && d->row_pl && d->row_ent && d->row_aux && d->scratch, "d4_policy_loss: null argument");
    D4_REQUIRE(d->rows >= 1 && d->na >= 0 && d->nc >= 0 && d->na + d->nc >= 1, "d4_policy_loss: rows >= 1 and at least one action");
    D4_REQUIRE(d->objective >= 0 && d->objective <= 2, "d4_policy_loss: objective 0 (ppo), 1 (spo) or 2 (pmpo)");
    D4_REQUIRE(d->beta_param == 0 || d->beta_param == 1, "d4_policy_loss: beta_param 0 (softplus) or 1 (exp)");
    if (d->na > 0) {
        D4_REQUIRE(d->logits && d->actions && d->old_log_probs && d->action_sizes && d->dlogits, "d4_policy_loss: null argument (discrete part)");
        D4_REQUIRE(d->total >= d->na && d->ld >= d->total, "d4_policy_loss: ld < total");
    } else {
        D4_REQUIRE(d->total == 0 && (d->ld == 0 || d->dlogits), "d4_policy_loss: without discrete actions total is 0 and ld columns of dlogits are zeroed");
    }
    if (d->nc > 0) {
        D4_REQUIRE(d->cparams && d->actions_cont && d->old_log_probs_cont && d->dcparams, "d4_policy_loss: null argument (continuous part)");
        D4_REQUIRE(d->ldc >= 2 * d->nc, "d4_policy_loss: ldc < 2 * nc");
    } else {
        D4_REQUIRE(d->ldc == 0 || d->dcparams, "d4_policy_loss: without continuous actions ldc columns of dcparams are zeroed");
    }
    if (d->objective == 2 && d->kl_w > 0.f)
        D4_REQUIRE((d->na == 0 || (d->old_logits && d->ldo >= d->total)) && (d->nc == 0 || d->old_cparams),
                   "d4_policy_loss: pmpo with a KL weight needs the old logits / old parameters  [D4:6160-6170]");
    D4_REQUIRE(!d->use_gate || d->gate_temp > 0.f, "d4_policy_loss: gate temperature must be positive");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* scal = d->scratch;                  // [64]: statistics and sums as in d4::learn; [32..33] the finalised pair
    float* ones = d->scratch + 64;             // [rows]
    const float* mask = d->mask;
    D4_HIP(hipMemsetAsync(scal, 0, 64 * sizeof(float), s));
    if (!mask) { if (int rc = d4::fill_f32(ones, 1.f, d->rows, s)) return rc; mask = ones; }
    d4::PolicyLossArgs p{};
    p.logits = d->logits; p.ld = d->ld; p.actions = d->actions; p.old_lp = d->old_log_probs; p.old_logits = d->old_logits; p.ldo = d->ldo;
    p.adv_raw = d->advantages; p.mask = mask; p.scal = scal; p.action_sizes = d->action_sizes; p.dlogits = d->dlogits;
    p.row_pl = d->row_pl; p.row_ent = d->row_ent; p.row_aux = d->row_aux;
    p.cparams = d->cparams; p.ldc = d->ldc; p.actions_cont = d->actions_cont; p.old_lp_cont = d->old_log_probs_cont; p.old_cparams = d->old_cparams;
    p.dcparams = d->dcparams; p.beta_param = d->beta_param; p.nc = d->nc;
    p.R = d->rows; p.na = d->na; p.A = d->total; p.objective = d->objective; p.normalize = d->normalize; p.use_gate = d->use_gate;
    p.reverse_kl = d->reverse_kl; p.eps = d->eps; p.clip = d->clip; p.ent_w = d->ent_w; p.gate_temp = d->gate_temp; p.pmpo_alpha = d->pmpo_alpha;
    p.kl_w = d->objective == 2 ? d->kl_w : 0.f;
    if (int rc = d4::policy_loss_run(p, scal, nullptr, nullptr, s)) return rc;
    hipLaunchKernelGGL(d4::finalize_losses_kernel, dim3(1), dim3(1), 0, s, scal, scal + 32, d->objective, d->ent_w, p.kl_w);
    D4_HIP(hipMemcpyAsync(d->loss, scal + 32, sizeof(float), hipMemcpyDeviceToDevice, s));
    D4_LAUNCH_CHECK();
    return 0;
}

// The discrete PPO / SPO form of d4_policy_loss with the advantages taken as given (no gate, no normalisation):
//   loss[0] = sum_r mask[r] (pl_r - entropy_weight * H_r) / max(sum mask, 1),  dlogits [rows][ld] = d loss / d logits.
// action_sizes: device int32 [na], total = their sum <= ld.  mask: [rows] or null.  scratch >= 5 * rows + 64 floats.
int d4_ppo_policy_loss(const float* logits, int ld, const int64_t* actions, const float* old_log_probs, const float* advantages, const float* mask,
                       const int32_t* action_sizes, int rows, int na, int total, int objective, float eps_clip, float entropy_weight, float* loss,
                       float* dlogits, float* scratch, void* stream) {
    D4_REQUIRE(logits && actions && old_log_probs && advantages && action_sizes && loss && dlogits && scratch && rows >= 1 && na >= 1 && total >= 1 && ld >= total,
               "d4_ppo_policy_loss: bad arguments");
    D4_REQUIRE(objective == 0 || objective == 1, "d4_ppo_policy_loss: objective 0 (ppo) or 1 (spo)");
    d4_policy_loss_desc d{};
    d.logits = logits; d.ld = ld; d.actions = actions; d.old_log_probs = old_log_probs; d.advantages = advantages; d.mask = mask;
    d.action_sizes = action_sizes; d.rows = rows; d.na = na; d.total = total; d.objective = objective; d.clip = eps_clip; d.ent_w = entropy_weight;
    d.eps = 1e-6f; d.gate_temp = 1.f;
    d.loss = loss; d.dlogits = dlogits; d.scratch = scratch;               // [64 + rows] of the scratch, then the three row terms
    d.row_pl = scratch + 64 + rows; d.row_ent = d.row_pl + rows; d.row_aux = d.row_ent + rows;
    return d4_policy_loss(&d, stream);
}

// Operator-level test entry points of the reductions and the RMSNorm backward: the launchers the learner and the blocks call.
int d4_colsum(const float* x, int ld, int rows, int cols, float* out, float* scratch, size_t scratch_floats, void* stream) {
    D4_REQUIRE(x && out && rows >= 1 && cols >= 1 && ld >= cols, "d4_colsum: bad arguments");
    return d4::colsum(x, ld, rows, cols, out, static_cast<hipStream_t>(stream), scratch, scratch_floats);
}
int d4_colsum_batch(int n, const float* const* x, const int32_t* ld, const int32_t* rows, const int32_t* cols, float* const* out, void* stream) {
    D4_REQUIRE(n >= 1 && n <= d4::ColsumBatch::MAX && x && ld && rows && cols && out, "d4_colsum_batch: 1 .. %d sums", (int)d4::ColsumBatch::MAX);
    d4::ColsumBatch b;
    for (int i = 0; i < n; ++i) {
        D4_REQUIRE(x[i] && out[i] && rows[i] >= 1 && cols[i] >= 1 && ld[i] >= cols[i], "d4_colsum_batch: bad arguments of sum %d", i);
        b.add(x[i], ld[i], rows[i], cols[i], out[i]);
    }
    return d4::colsum_batch(b, static_cast<hipStream_t>(stream));
}
int d4_rmsnorm_bwd(const float* x, const float* dxhat, const float* gamma, float* tg, float* dx, int rows, int dim, float eps, void* stream) {
    D4_REQUIRE(x && dxhat && gamma && tg && rows >= 0 && dim >= 1, "d4_rmsnorm_bwd: bad arguments");
    return d4::rmsnorm_bwd(x, dxhat, gamma, tg, dx, rows, dim, eps, static_cast<hipStream_t>(stream));
}
int d4_layernorm_silu_bwd(const float* z, int ldz, const float* da, const float* g, const float* b, float* tg, float* tb, float* dz, int rows, int dim, float eps,
                          void* stream) {
    D4_REQUIRE(z && da && g && b && tg && tb && dz && rows >= 1 && dim >= 1 && ldz >= dim, "d4_layernorm_silu_bwd: bad arguments");
    return d4::layernorm_silu_bwd(z, ldz, da, g, b, tg, tb, dz, rows, dim, eps, static_cast<hipStream_t>(stream));
}
int d4_silu_bwd(const float* dy, const float* z, float* dz, int64_t n, void* stream) {
    D4_REQUIRE(dy && z && dz && n >= 0, "d4_silu_bwd: bad arguments");
    return d4::silu_bwd(dy, z, dz, n, static_cast<hipStream_t>(stream));
}

// clip_grad_norm_(params, max_norm) followed by one AdamW step on a flat parameter group
// (trainers.py:1436-1452; torch.optim.AdamW semantics).  scratch: >= 1025 floats.
int d4_adamw_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                  float lr, float beta1, float beta2, float eps, float weight_decay, float max_grad_norm,
                  float grad_scale, float* scratch, void* stream) {
    D4_REQUIRE(params && grads && exp_avg && exp_avg_sq && scratch && n > 0 && step >= 1, "adamw: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int np = 1024;
    hipLaunchKernelGGL(d4::sumsq_partial_kernel, dim3(np), dim3(256), 0, s, grads, n, scratch + 1);
    hipLaunchKernelGGL(d4::norm_final_kernel, dim3(1), dim3(256), 0, s, scratch + 1, np, grad_scale, scratch);
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    int64_t g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(d4::adamw_kernel, dim3((unsigned)g), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, n, scratch, max_grad_norm,
                       grad_scale, lr, beta1, beta2, eps, weight_decay, bc1, bc2);
    D4_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
