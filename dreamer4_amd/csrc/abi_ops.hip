// Engine-free part of the C ABI: the operator-level entry points (thin wrappers over kernels.h that check their arguments, fill the launcher's
// argument struct and call it) and the profile pass-throughs.  Everything that takes a d4_engine or touches an engine hook is in engine.hip.
#include "common.h"
#include "engine.h"
#include "prof.h"

extern "C" {

int d4_profile_bf16_enable(int stride) { d4::gemm_bf16_profile_enable(stride); return 0; }
int d4_profile_bf16_read(double* ms, double* flops, int64_t* count) { return d4::gemm_bf16_profile_read(ms, flops, count); }
int d4_profile_enable(int on) { return d4::gemm_profile_enable(on); }
int d4_profile_read(double* ms, double* flops, int64_t* count, int nclass) { return d4::gemm_profile_read(ms, flops, count, nclass); }
int d4_profile_classes(void) { return d4::gemm_profile_classes(); }
int d4_profile_glue_enable(int mask) { return d4::glue_profile_enable(mask); }
int d4_profile_glue_read(double* ms, double* bytes, int64_t* count, int nclass) { return d4::glue_profile_read(ms, bytes, count, nclass); }
int d4_profile_glue_classes(void) { return d4::GL_N; }
int d4_profile_glue_read_flops(double* flops, int nclass) { return d4::glue_profile_read_flops(flops, nclass); }
const char* d4_profile_glue_class_name(int c) { return d4::glue_class_name(c); }
int d4_frame_fused_set(int mode) { return d4::frame_fused_set(mode); }
const char* d4_profile_class_name(int c) { return d4::gemm_profile_class_name(c); }

int d4_gemm(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias,
            const float* R, int ldr, int M, int N, int K, int flags, float rms_eps, void* stream) {
    d4::GemmArgs g{A, lda, W, ldw, C, ldc, bias, R, ldr, M, N, K, flags, rms_eps};
    return d4::gemm(g, static_cast<hipStream_t>(stream));
}

int d4_gemm_pair(const float* A1, int lda1, const float* W1, float* C1, int ldc1, int M1, int N1, const float* A2, int lda2, const float* W2, float* C2,
                 int ldc2, int M2, int N2, int K, int flags, float rms_eps, void* stream) {
    d4::GemmArgs a{A1, lda1, W1, K, C1, ldc1, nullptr, nullptr, 0, M1, N1, K, flags, rms_eps};
    d4::GemmArgs b{A2, lda2, W2, K, C2, ldc2, nullptr, nullptr, 0, M2, N2, K, flags, rms_eps};
    return d4::gemm_pair(a, b, static_cast<hipStream_t>(stream));
}

int d4_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, float* part, int64_t part_floats,
               int tile_n, int slices, void* stream) {
    return d4::gemm_tn(A, lda, B, ldb, C, ldc, M, N, K, part, (size_t)part_floats, static_cast<hipStream_t>(stream), tile_n, slices);
}

int d4_gemm_batched(const float* A, int lda, const float* W, int ldw, float* C, int ldc, const float* bias,
                    const float* R, int ldr, int M, int N, int K, int flags, float rms_eps, int batch,
                    int64_t strideA, int64_t strideW, int64_t strideC, void* stream) {
    d4::GemmArgs g{A, lda, W, ldw, C, ldc, bias, R, ldr, M, N, K, flags, rms_eps};
    g.batch = batch; g.strideA = strideA; g.strideW = strideW; g.strideC = strideC;
    return d4::gemm(g, static_cast<hipStream_t>(stream));
}

int d4_split_bf16x3(const float* src, uint16_t* dst, int64_t n, int64_t plane_stride, void* stream) {
    D4_REQUIRE(src && dst && n >= 0 && plane_stride >= n && (plane_stride % 8) == 0, "d4_split_bf16x3: bad arguments");
    return d4::split_bf16x3(src, dst, n, plane_stride, static_cast<hipStream_t>(stream));
}
int d4_gemm_split(const float* A, int lda, const uint16_t* W3, int64_t plane_stride, int ldw, float* C, int ldc, const float* bias,
                  const float* R, int ldr, int M, int N, int K, int flags, float rms_eps, int config, void* stream) {
    d4::GemmArgs g{A, lda, reinterpret_cast<const float*>(W3), ldw, C, ldc, bias, R, ldr, M, N, K, flags, rms_eps};
    g.Wb = W3; g.wplane = plane_stride;
    D4_REQUIRE(d4::gemm_x3_applicable(g), "d4_gemm_split: call not supported (M=%d N=%d K=%d flags=%d: K %% 32, ldw %% 8, plane_stride %% 8, 16-byte alignment)", M, N, K, flags);
    if (M == 0) return 0;
    if (config == d4::gemm_x3_configs()) return d4::gemm_x3sk_launch(g, static_cast<hipStream_t>(stream));      // 6: the persistent form (the engine's)
    if (config >= 0) return d4::gemm_x3_launch(config, g, static_cast<hipStream_t>(stream));
    return d4::gemm_x3_launch(d4::gemm_x3_heuristic(g), g, static_cast<hipStream_t>(stream));
}
int d4_split_f16x2(const float* src, uint16_t* dst, int rows, int cols, int ld, int64_t plane_stride, float* inv_scale, void* stream) {
    D4_REQUIRE(src && dst && inv_scale && rows >= 0 && cols >= 1 && ld >= cols && (ld % 8) == 0 && plane_stride >= (int64_t)rows * ld && (plane_stride % 8) == 0,
               "d4_split_f16x2: bad arguments");
    return d4::split_f16x2_rows(src, dst, rows, cols, ld, plane_stride, inv_scale, static_cast<hipStream_t>(stream));
}
int d4_row_scale_exp(const float* A, int64_t lda, int rows, int K, int32_t* exp_out, void* stream) {
    D4_REQUIRE(A && exp_out && rows >= 0 && K >= 4 && lda >= K, "d4_row_scale_exp: bad arguments");
    return d4::row_scale_exp(A, lda, rows, K, exp_out, static_cast<hipStream_t>(stream));
}
int d4_gemm_split2(const float* A, int lda, const uint16_t* W2, int64_t plane_stride, int ldw, const float* w_inv_scale, float* C, int ldc, const float* bias,
                   const float* R, int ldr, int M, int N, int K, int flags, float rms_eps, int config, const int32_t* a_exp, void* stream) {
    d4::GemmArgs g{A, lda, reinterpret_cast<const float*>(W2), ldw, C, ldc, bias, R, ldr, M, N, K, flags, rms_eps};
    g.Wb = W2; g.wplane = plane_stride; g.wscale = w_inv_scale; g.aexp = a_exp;
    D4_REQUIRE(d4::gemm_h2_applicable(g), "d4_gemm_split2: call not supported (M=%d N=%d K=%d flags=%d: K %% 32, lda %% 4, ldw %% 8, plane_stride %% 8, 16-byte alignment)", M, N, K, flags);
    if (M == 0) return 0;
    return d4::gemm_h2_launch(config >= 0 ? config : d4::gemm_h2_heuristic(g), g, static_cast<hipStream_t>(stream));
}
int d4_gemm_bf16(const float* A, int lda, const uint16_t* Wb, int ldw, float* C, int ldc, const float* bias,
                 const float* R, int ldr, int M, int N, int K, int flags, float rms_eps, void* stream) {
    d4::GemmArgs g{A, lda, reinterpret_cast<const float*>(Wb), ldw, C, ldc, bias, R, ldr, M, N, K, flags, rms_eps};
    g.Wb = Wb;
    return d4::gemm_bf16(g, static_cast<hipStream_t>(stream));
}

int d4_cvt_bf16(const float* src, uint16_t* dst, int64_t n, void* stream) { return d4::cvt_f32_to_bf16(src, dst, n, static_cast<hipStream_t>(stream)); }

int d4_gemm_bf16a(const uint16_t* Ab, int lda, const uint16_t* Wb, int ldw, float* C, int ldc, uint16_t* Cb, const float* bias, const float* R, int ldr,
                  int M, int N, int K, int flags, float rms_eps, int config, void* stream) {
    d4::GemmArgs g{nullptr, lda, nullptr, ldw, C, ldc, bias, R, ldr, M, N, K, flags, rms_eps};
    g.Ab = Ab; g.Wb = Wb; g.Cb = Cb;
    D4_REQUIRE(d4::gemm_bf16a_applicable(g), "d4_gemm_bf16a: call not supported (K %% 64, lda / ldw %% 8, 16-byte aligned operands)");
    if (config >= 100) { g.group_m = -1; config -= 100; }       // 100 + c: configuration c with the plain row-major tile order (A/B of the grouped order)
    return d4::gemm_bf16a_launch(config >= 0 ? config : d4::gemm_bf16a_rule(g), g, static_cast<hipStream_t>(stream));
}

int d4_gemm_bf16a_compact(const uint16_t* Ab, int lda, const uint16_t* Wb, int ldw, float* C, int ldc, uint16_t* Cb, const float* bias, const float* R, int ldr,
                          int M, int N, int K, int flags, float rms_eps, float* C2, uint16_t* C2b, int ldc2, int c2_S, int c2_lo, int c2_hi, int c2_last,
                          int config, void* stream) {
    d4::GemmArgs g{nullptr, lda, nullptr, ldw, C, ldc, bias, R, ldr, M, N, K, flags, rms_eps};
    g.Ab = Ab; g.Wb = Wb; g.Cb = Cb;
    g.C2 = C2; g.C2b = C2b; g.ldc2 = ldc2; g.c2_S = c2_S; g.c2_lo = c2_lo; g.c2_hi = c2_hi; g.c2_last = c2_last;
    D4_REQUIRE(C2 && c2_S >= 1 && c2_lo >= 0 && c2_hi >= c2_lo && c2_hi <= c2_S, "d4_gemm_bf16a_compact: bad compaction arguments");
    D4_REQUIRE(d4::gemm_bf16a_applicable(g), "d4_gemm_bf16a_compact: call not supported (K %% 64, lda / ldw %% 8, 16-byte aligned operands)");
    return d4::gemm_bf16a_launch(config >= 0 ? config : d4::gemm_bf16a_rule(g), g, static_cast<hipStream_t>(stream));
}

int d4_gemm_bf16a_batched(const uint16_t* Ab, int lda, const uint16_t* Wb, int ldw, float* C, int ldc, uint16_t* Cb, const float* bias, const float* R, int ldr,
                          int M, int N, int K, int flags, float rms_eps, int batch, int64_t strideA, int64_t strideW, int64_t strideC, int config, void* stream) {
    d4::GemmArgs g{nullptr, lda, nullptr, ldw, C, ldc, bias, R, ldr, M, N, K, flags, rms_eps};
    g.Ab = Ab; g.Wb = Wb; g.Cb = Cb;
    g.batch = batch; g.strideA = strideA; g.strideW = strideW; g.strideC = strideC;
    D4_REQUIRE(C || Cb, "d4_gemm_bf16a_batched: no output");
    if (M == 0) return 0;
    D4_REQUIRE(d4::gemm_bf16a_applicable(g), "d4_gemm_bf16a_batched: call not supported (K %% 64, lda / ldw / strides %% 8, 16-byte aligned operands)");
    return d4::gemm_bf16a_launch(config >= 0 ? config : d4::gemm_bf16a_rule(g), g, static_cast<hipStream_t>(stream));
}
int d4_cvt_rows_bf16(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int rows, int cols, void* stream) {
    D4_REQUIRE(src && dst && rows >= 0 && cols >= 0 && lds >= cols && ldd >= cols, "d4_cvt_rows_bf16: bad arguments");
    return d4::cvt_rows_bf16(src, lds, dst, ldd, rows, cols, static_cast<hipStream_t>(stream));
}

int d4_rmsnorm(const float* x, int ldx, const float* gamma, float* y, int ldy, int rows, int dim, float eps, void* stream) {
    return d4::rmsnorm_rows(x, ldx, gamma, y, ldy, rows, dim, eps, static_cast<hipStream_t>(stream));
}

// Operator-level test entry points of the glue launchers of elementwise.hip: each checks its pointers and sizes, fills the launcher's
// arguments and calls it.
int d4_layernorm_rows(const float* x, int ldx, const float* g, const float* b, float* y, int ldy, int rows, int dim, float eps, int silu, void* stream) {
    D4_REQUIRE(x && g && y && rows >= 0 && dim >= 1 && ldx >= dim && ldy >= dim, "d4_layernorm_rows: bad arguments");
    return d4::layernorm_rows(x, ldx, g, b, y, ldy, rows, dim, eps, silu, static_cast<hipStream_t>(stream));
}
int d4_assemble_tokens(const d4_assemble_desc* d, void* stream) {
    D4_REQUIRE(d && d->tokens && d->signal_embed && d->step_embed && d->agent_embed, "d4_assemble_tokens: null argument");
    D4_REQUIRE(d->B >= 0 && d->Tq >= 0 && d->D >= 2 && d->D % 2 == 0 && d->ns >= 0 && d->nr >= 0 && d->na >= 0 && d->nc >= 0 && d->step_log2 >= 0 &&
               (d->has_agent == 0 || d->has_agent == 1), "d4_assemble_tokens: bad sizes");
    D4_REQUIRE(d->S == 1 + d->ns + d->nr + (d->na > 0 || d->nc > 0 ? 1 : 0) + d->has_agent, "d4_assemble_tokens: S %d is not 1 + ns + nr (+ action) (+ agent)", d->S);
    D4_REQUIRE((d->ns == 0 || d->space) && (d->nr == 0 || d->registers) && (d->signal_levels || d->signal_uniform >= 0), "d4_assemble_tokens: table missing");
    D4_REQUIRE((d->na == 0 && d->nc == 0) || d->action_learned, "d4_assemble_tokens: action_learned missing");
    D4_REQUIRE(d->na == 0 || !d->prev_actions || (d->action_embed && d->action_offsets), "d4_assemble_tokens: action tables missing");
    D4_REQUIRE(d->nc == 0 || !d->prev_cont || d->cont_embed, "d4_assemble_tokens: cont_embed missing");
    D4_REQUIRE(!d->tasks || d->task_embed, "d4_assemble_tokens: task_embed missing");
    d4::AssembleArgs a{};
    a.tokens = d->tokens; a.space = d->space; a.signal_embed = d->signal_embed; a.step_embed = d->step_embed; a.registers = d->registers;
    a.agent_embed = d->agent_embed; a.task_embed = d->task_embed; a.action_embed = d->action_embed; a.action_learned = d->action_learned;
    a.signal_levels = d->signal_levels; a.signal_uniform = d->signal_uniform; a.prev_actions = d->prev_actions; a.prev_cont = d->prev_cont;
    a.cont_embed = d->cont_embed; a.tasks = d->tasks; a.action_offsets = d->action_offsets;
    a.B = d->B; a.Tq = d->Tq; a.S = d->S; a.D = d->D; a.ns = d->ns; a.nr = d->nr; a.na = d->na; a.nc = d->nc; a.step_log2 = d->step_log2;
    a.compact = d->compact; a.has_agent = d->has_agent;
    return d4::assemble_tokens(a, static_cast<hipStream_t>(stream));
}
int d4_gather_space_double_norm(const float* tokens, float* out, const float* g0, const float* g1, int frames, int S, int first, int dim, int ns,
                                float eps, void* stream) {
    D4_REQUIRE(tokens && out && g0 && g1 && frames >= 0 && dim >= 1 && ns >= 1 && first >= 0 && first + ns <= S, "d4_gather_space_double_norm: bad arguments");
    return d4::gather_space_double_norm(tokens, out, g0, g1, frames, S, first, dim, ns, eps, static_cast<hipStream_t>(stream));
}
int d4_euler_step_rows(float* x, int ldx, const float* pred, int ldp, int B, int n_el, float one_minus_t, float dt, void* stream) {
    D4_REQUIRE(x && pred && B >= 0 && n_el >= 0 && ldx >= n_el && ldp >= n_el, "d4_euler_step_rows: bad arguments");
    return d4::euler_step(x, ldx, pred, ldp, B, n_el, one_minus_t, dt, static_cast<hipStream_t>(stream));
}
int d4_splitk_reduce(const float* part, int S, int M, int N, const float* bias, int silu, float* y, int ldy, void* stream) {
    D4_REQUIRE(part && y && S >= 1 && M >= 0 && N >= 1 && ldy >= N, "d4_splitk_reduce: bad arguments");
    return d4::splitk_reduce(part, S, M, N, bias, silu, y, ldy, static_cast<hipStream_t>(stream));
}
int d4_mean_tokens(const float* x, float* out, int B, int n, int d, void* stream) {
    D4_REQUIRE(x && out && B >= 0 && n >= 1 && d >= 1, "d4_mean_tokens: bad arguments");
    return d4::mean_tokens(x, out, B, n, d, static_cast<hipStream_t>(stream));
}
int d4_hl_gauss_scalar_strided(const float* logits, int ld, const float* centers, float* out, int out_stride, int rows, int bins, void* stream) {
    D4_REQUIRE(logits && centers && out && rows >= 0 && bins >= 1 && ld >= bins && out_stride >= 1, "d4_hl_gauss_scalar_strided: bad arguments");
    return d4::hl_gauss_scalar(logits, ld, centers, out, out_stride, rows, bins, static_cast<hipStream_t>(stream));
}
int d4_fold_rows(const float* W, const float* gamma, float* out, int rows, int K, int ld_out, void* stream) {
    D4_REQUIRE(W && out && rows >= 0 && K >= 1 && ld_out >= K, "d4_fold_rows: bad arguments");
    return d4::fold_rows(W, gamma, out, rows, K, ld_out, static_cast<hipStream_t>(stream));
}
int d4_swiglu_pack_rows(const float* W, const float* bias, const float* gamma, float* Wp, float* bp, int inner, int inner_pad, int K, void* stream) {
    D4_REQUIRE(W && bias && gamma && Wp && bp && inner >= 1 && inner_pad >= inner && inner_pad % 32 == 0 && K >= 1, "d4_swiglu_pack_rows: bad arguments (inner_pad %% 32)");
    return d4::swiglu_pack_rows(W, bias, gamma, Wp, bp, inner, inner_pad, K, static_cast<hipStream_t>(stream));
}
int d4_build_latent_input(float* out, const float* hist, const float* ctx_noise, const float* x, int B, int Tq, int n_el, int hist_t_stride, float w, void* stream) {
    D4_REQUIRE(out && x && B >= 0 && Tq >= 1 && n_el >= 0 && (Tq == 1 || (hist && hist_t_stride >= Tq - 1)), "d4_build_latent_input: bad arguments");
    return d4::build_latent_input(out, hist, ctx_noise, x, B, Tq, n_el, hist_t_stride, w, static_cast<hipStream_t>(stream));
}
int d4_copy_rows(const float* src, int lds, float* dst, int ldd, int rows, int cols, void* stream) {
    D4_REQUIRE(src && dst && rows >= 0 && cols >= 0 && lds >= cols && ldd >= cols, "d4_copy_rows: bad arguments");
    return d4::copy_rows(src, lds, dst, ldd, rows, cols, static_cast<hipStream_t>(stream));
}
int d4_pad_cols(const float* W, float* out, int rows, int cols, int cols_pad, void* stream) {
    D4_REQUIRE(W && out && rows >= 1 && cols >= 1 && cols_pad >= cols, "d4_pad_cols: bad arguments");
    return d4::pad_cols(W, out, rows, cols, cols_pad, static_cast<hipStream_t>(stream));
}
int d4_video_patches(const float* src, float* dst, int B, int C, int T, int nh, int nw, int ps, int to_patches, void* stream) {
    D4_REQUIRE(src && dst && B >= 0 && C >= 1 && T >= 1 && nh >= 1 && nw >= 1 && ps >= 1, "d4_video_patches: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return to_patches ? d4::video_to_patches(src, dst, B, C, T, nh, nw, ps, s) : d4::patches_to_video(src, dst, B, C, T, nh, nw, ps, s);
}
int d4_cache_transfer(float* cache, float* ext, int Lt, int cache_batch, int B, int S, int H, int Tcap, int frames, int to_ext, int dh, void* stream) {
    D4_REQUIRE(cache && ext && Lt >= 0 && B >= 0 && cache_batch >= B && S >= 1 && H >= 1 && frames >= 0 && Tcap >= frames && dh >= 1, "d4_cache_transfer: bad arguments");
    return d4::cache_transfer(cache, ext, Lt, cache_batch, B, S, H, Tcap, frames, to_ext, dh, static_cast<hipStream_t>(stream));
}
int d4_cunembed(int op, const float* src, float* dst, int nc, int mtp, int d, void* stream) {
    D4_REQUIRE(src && dst && nc >= 0 && mtp >= 1 && d >= 1 && (op == 0 || op == 1), "d4_cunembed: op 0 (gather) or 1 (scatter the gradient)");
    return op == 0 ? d4::cunembed_gather(src, dst, nc, mtp, d, static_cast<hipStream_t>(stream)) : d4::cunembed_scatter_grad(src, dst, nc, mtp, d, static_cast<hipStream_t>(stream));
}
int d4_coord_grid(float* out, int nh, int nw, int ld, void* stream) {
    D4_REQUIRE(out && nh >= 1 && nw >= 1 && ld >= 2, "d4_coord_grid: bad arguments");
    return d4::coord_grid(out, nh, nw, ld, static_cast<hipStream_t>(stream));
}
int d4_pack_tokens(int which, float* tokens, float* compact, const float* pos, const float* img, const float* lat, int frames, int P, int n_lat, int n_total,
                   int D, void* stream) {
    D4_REQUIRE(tokens && compact && img && lat && frames >= 0 && P >= 0 && n_lat >= 0 && D >= 1 && (which == 0 || which == 1), "d4_pack_tokens: bad arguments");
    D4_REQUIRE(which == 1 || (pos && n_total >= n_lat), "d4_pack_tokens: the decoder form needs pos and n_total >= n_lat");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return which == 0 ? d4::decoder_pack_tokens(tokens, compact, pos, img, lat, frames, P, n_lat, n_total, D, s)
                      : d4::encoder_pack_tokens(tokens, compact, img, lat, frames, P, n_lat, D, s);
}
int d4_pack_tokens_bf16(int which, float* tokens, uint16_t* tokens_b, float* compact, uint16_t* compact_b, const float* pos, const float* img, const float* lat,
                        int frames, int P, int n_lat, int n_total, int D, void* stream) {
    D4_REQUIRE(tokens && tokens_b && compact && img && lat && frames >= 0 && P >= 0 && n_lat >= 0 && D >= 1 && (which == 0 || which == 1), "d4_pack_tokens_bf16: bad arguments");
    D4_REQUIRE(which == 1 || (pos && n_total >= n_lat), "d4_pack_tokens_bf16: the decoder form needs pos and n_total >= n_lat");
    return d4::pack_tokens_img(which, tokens, tokens_b, compact, compact_b, pos, img, lat, frames, P, n_lat, which == 0 ? n_total : n_lat, D, static_cast<hipStream_t>(stream));
}
int d4_prep_eval_inputs(int32_t* sig, int64_t* pact, const int64_t* actions_hist, int B, int Tq, int na, int frame_base, int hist_stride, int sig_val, int ctx_sig,
                        float* pcont, const float* cont_hist, int nc, void* stream) {
    D4_REQUIRE(sig && B >= 1 && Tq >= 1 && na >= 0 && nc >= 0 && frame_base >= 0 && hist_stride >= frame_base + Tq - 1, "d4_prep_eval_inputs: bad arguments");
    D4_REQUIRE((na == 0 || pact) && (nc == 0 || pcont), "d4_prep_eval_inputs: pact / pcont missing");
    return d4::prep_eval_inputs(sig, pact, actions_hist, B, Tq, na, frame_base, hist_stride, sig_val, ctx_sig, static_cast<hipStream_t>(stream), pcont, cont_hist, nc);
}
int d4_unary_rows(int op, const float* x, float* y, int64_t n, void* stream) {
    D4_REQUIRE(x && y && n >= 0 && (op == 0 || op == 1), "d4_unary_rows: op 0 (silu) or 1 (tanh)");
    return op == 0 ? d4::silu_rows(x, y, n, static_cast<hipStream_t>(stream)) : d4::tanh_rows(x, y, n, static_cast<hipStream_t>(stream));
}

// Operator-level test entry points of the inference attention cores (attn.hip): each fills the launcher's argument struct and calls it.
static int small_attn_entry(int wide, const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                  const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                  const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                  int64_t m_item_stride, float* out, int64_t o_group_stride, int64_t o_item_stride, uint16_t* out_b, int groups, int heads, int nq, int nk,
                  float softclamp, int mask_special, int belief, int q_lo, int q_hi, int q_last, int dh, void* stream) {
    d4::SmallAttnArgs sa{};
    sa.wide = wide;
    sa.q = q; sa.q_group_stride = q_group_stride; sa.q_item_stride = q_item_stride;
    sa.k = k; sa.k_group_stride = k_group_stride; sa.k_item_stride = k_item_stride;
    sa.v = v; sa.v_group_stride = v_group_stride; sa.v_item_stride = v_item_stride;
    sa.gate = gate; sa.g_group_stride = g_group_stride; sa.g_item_stride = g_item_stride;
    sa.k_gamma = k_gamma;
    sa.vres = vres; sa.r_group_stride = r_group_stride; sa.r_item_stride = r_item_stride;
    sa.mix = mix; sa.m_group_stride = m_group_stride; sa.m_item_stride = m_item_stride;
    sa.out = out; sa.o_group_stride = o_group_stride; sa.o_item_stride = o_item_stride; sa.out_b = out_b;
    sa.groups = groups; sa.heads = heads; sa.nq = nq; sa.nk = nk;
    sa.softclamp = softclamp; sa.mask_special = mask_special; sa.belief = belief;
    sa.q_lo = q_lo; sa.q_hi = q_hi; sa.q_last = q_last; sa.dh = dh;
    return d4::small_attn(sa, static_cast<hipStream_t>(stream));
}
int d4_small_attn(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                  const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                  const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                  int64_t m_item_stride, float* out, int64_t o_group_stride, int64_t o_item_stride, uint16_t* out_b, int groups, int heads, int nq, int nk,
                  float softclamp, int mask_special, int belief, int q_lo, int q_hi, int q_last, int dh, void* stream) {
    return small_attn_entry(0, q, q_group_stride, q_item_stride, k, k_group_stride, k_item_stride, v, v_group_stride, v_item_stride, gate, g_group_stride, g_item_stride,
                            k_gamma, vres, r_group_stride, r_item_stride, mix, m_group_stride, m_item_stride, out, o_group_stride, o_item_stride, out_b, groups, heads,
                            nq, nk, softclamp, mask_special, belief, q_lo, q_hi, q_last, dh, stream);
}
int d4_small_attn_wide(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                  const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                  const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                  int64_t m_item_stride, float* out, int64_t o_group_stride, int64_t o_item_stride, uint16_t* out_b, int groups, int heads, int nq, int nk,
                  float softclamp, int mask_special, int belief, int q_lo, int q_hi, int q_last, int dh, void* stream) {
    return small_attn_entry(1, q, q_group_stride, q_item_stride, k, k_group_stride, k_item_stride, v, v_group_stride, v_item_stride, gate, g_group_stride, g_item_stride,
                            k_gamma, vres, r_group_stride, r_item_stride, mix, m_group_stride, m_item_stride, out, o_group_stride, o_item_stride, out_b, groups, heads,
                            nq, nk, softclamp, mask_special, belief, q_lo, q_hi, q_last, dh, stream);
}

int d4_small_attn_wide_bf16(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                  const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                  const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                  int64_t m_item_stride, float* out, int64_t o_group_stride, int64_t o_item_stride, uint16_t* out_b, int groups, int heads, int nq, int nk,
                  float softclamp, int mask_special, int belief, int q_lo, int q_hi, int q_last, int dh, void* stream) {
    return small_attn_entry(2, q, q_group_stride, q_item_stride, k, k_group_stride, k_item_stride, v, v_group_stride, v_item_stride, gate, g_group_stride, g_item_stride,
                            k_gamma, vres, r_group_stride, r_item_stride, mix, m_group_stride, m_item_stride, out, o_group_stride, o_item_stride, out_b, groups, heads,
                            nq, nk, softclamp, mask_special, belief, q_lo, q_hi, q_last, dh, stream);
}

int d4_lqap_in(const float* latents, int ldl, const float* w_kv, int ldw, const float* q, const float* gate, const float* k_gamma, float* out, int frames,
               int heads, int n, int ns, int dl, float eps, void* stream) {
    D4_REQUIRE(latents && w_kv && q && gate && k_gamma && out, "d4_lqap_in: null argument");
    return d4::lqap_in(latents, ldl, w_kv, ldw, q, gate, k_gamma, out, frames, heads, n, ns, dl, eps, static_cast<hipStream_t>(stream));
}
int d4_lqap_out(const float* kv, int ldkv, const float* q, const float* gate, const float* k_gamma, const float* w_out, int ldw, float* pred, int ldp,
                int frames, int heads, int n, int ns, int dl, void* stream) {
    D4_REQUIRE(kv && q && gate && k_gamma && w_out && pred, "d4_lqap_out: null argument");
    return d4::lqap_out(kv, ldkv, q, gate, k_gamma, w_out, ldw, pred, ldp, frames, heads, n, ns, dl, static_cast<hipStream_t>(stream));
}

int d4_pool_mix(const float* q, int ldq, const float* x, int ldx, const float* gate_w, const float* k, int ldk, const float* hid, int D,
                const float* k_gamma, float* u, int M, int L, int heads, float eps, uint16_t* u_b, const uint16_t* k_b, const uint16_t* q_b,
                const uint16_t* hid_b, void* stream) {
    d4::PoolMixArgs pm{};
    pm.q = q; pm.ldq = ldq; pm.x = x; pm.ldx = ldx; pm.gate_w = gate_w; pm.k = k; pm.ldk = ldk; pm.hid = hid; pm.D = D; pm.k_gamma = k_gamma;
    pm.u = u; pm.M = M; pm.L = L; pm.heads = heads; pm.eps = eps; pm.u_b = u_b; pm.k_b = k_b; pm.q_b = q_b; pm.hid_b = hid_b;
    return d4::pool_mix(pm, static_cast<hipStream_t>(stream));
}

int d4_time_attn_decode(const float* proj, int ldp, const float* vres, int ldv, const float* k_gamma, const float* inv_freq, float* cache, float* out,
                        int ldo, uint16_t* out_b, int B, int S, int H, int Tq, int t0, int Tcap, int cache_batch, int cache_S, const int* t0_dev,
                        float softclamp, int dh, int mode, void* stream) {
    D4_REQUIRE(mode >= 0 && mode <= 2, "d4_time_attn_decode: mode %d (0 append + attend, 1 append only, 2 attend only)", mode);
    d4::TimeAttnArgs ta{};
    ta.proj = proj; ta.ldp = ldp; ta.vres = vres; ta.ldv = ldv; ta.k_gamma = k_gamma; ta.inv_freq = inv_freq; ta.cache = cache;
    ta.out = out; ta.ldo = ldo; ta.out_b = out_b; ta.B = B; ta.S = S; ta.H = H; ta.Tq = Tq; ta.t0 = t0; ta.Tcap = Tcap;
    ta.cache_batch = cache_batch; ta.cache_S = cache_S; ta.t0_dev = t0_dev; ta.softclamp = softclamp; ta.dh = dh;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return mode == 0 ? d4::time_attn_append(ta, s) : mode == 1 ? d4::time_kv_append(ta, s) : d4::time_attn(ta, s);
}

int d4_pool_mix_deep(const float* q, int ldq, const float* x, int ldx, const float* gate_w, const float* k, int ldk, const float* hid, int D,
                     const float* k_gamma, float* u, int M, int L, int heads, float eps, uint16_t* u_b, const uint16_t* k_b, const uint16_t* q_b,
                     const uint16_t* hid_b, void* stream) {
    d4::PoolMixArgs pm{};
    pm.q = q; pm.ldq = ldq; pm.x = x; pm.ldx = ldx; pm.gate_w = gate_w; pm.k = k; pm.ldk = ldk; pm.hid = hid; pm.D = D; pm.k_gamma = k_gamma;
    pm.u = u; pm.M = M; pm.L = L; pm.heads = heads; pm.eps = eps; pm.u_b = u_b; pm.k_b = k_b; pm.q_b = q_b; pm.hid_b = hid_b;
    return d4::pool_mix_deep(pm, static_cast<hipStream_t>(stream));
}

const char* d4_debug_last_form(const char* family) { return d4::attn_last_form(family); }
int d4_debug_forms(const char* family, int i, const char** name) { return d4::attn_form_name(family, i, name); }

// Operator-level test entry points of the GEMM launches only the engine reaches otherwise: one family / configuration named by the caller, straight to
// its launcher; and the pair launches.  A refusal names its reason and nothing falls through to another family.
static d4::GemmArgs gemm_args_of(const d4_gemm_desc& d) {
    d4::GemmArgs g{d.A, d.lda, d.W, d.ldw, d.C, d.ldc, d.bias, d.R, d.ldr, d.M, d.N, d.K, d.flags, d.rms_eps};
    g.C2 = d.C2; g.ldc2 = d.ldc2; g.c2_S = d.c2_S; g.c2_lo = d.c2_lo; g.c2_hi = d.c2_hi; g.c2_last = d.c2_last;
    g.batch = d.batch > 0 ? d.batch : 1; g.strideA = d.strideA; g.strideW = d.strideW; g.strideC = d.strideC;
    g.Ab = d.Ab; g.Wb = d.Wb; g.Cb = d.Cb; g.C2b = d.C2b; g.wplane = d.wplane; g.wscale = d.wscale; g.strideWs = d.strideWs; g.aexp = d.aexp;
    return g;
}
static int gemm_desc_check(const char* who, const d4_gemm_desc* d) {
    D4_REQUIRE(d && d->M >= 1 && d->N >= 1 && d->K >= 1 && (d->C || d->Cb), "%s: null descriptor, no output or bad sizes", who);
    D4_REQUIRE(!(d->C2 || d->C2b) || (d->C2 && d->c2_S >= 1 && d->c2_lo >= 0 && d->c2_hi >= d->c2_lo && d->c2_hi <= d->c2_S && d->ldc2 >= d->N &&
                                      (d->c2_last == 0 || d->c2_last == 1) && !(d->flags & d4::GEMM_SWIGLU)),
               "%s: bad compaction arguments", who);
    return 0;
}
int d4_gemm_family_configs(int family) {
    switch (family) {
        case D4_GEMM_TILE: return d4::gemm_configs();
        case D4_GEMM_V2: return d4::gemm2_configs();
        case D4_GEMM_X3: return d4::gemm_x3_configs();
        case D4_GEMM_H2: return d4::gemm_h2_configs();
        case D4_GEMM_BF16: return d4::gemm_bf16_configs();
        case D4_GEMM_BF16A: return d4::gemm_bf16a_configs();
        case D4_GEMM_V2_KSPLIT: case D4_GEMM_X3SK: case D4_GEMM_SKINNY: return 1;
    }
    return -1;
}
int d4_gemm_route(const d4_gemm_desc* d, int rule_M) {
    if (gemm_desc_check("d4_gemm_route", d)) return -1;
    d4::GemmArgs g = gemm_args_of(*d);
    g.rule_M = rule_M;
    int family = -1;
    return d4::gemm_route_checked(g, &family) ? -1 : family;
}
static int gemm_run_args(const d4::GemmArgs& g, int family, int config, void* stream);
int d4_gemm_run(const d4_gemm_desc* d, int family, int config, void* stream) {
    if (int rc = gemm_desc_check("d4_gemm_run", d)) return rc;
    return gemm_run_args(gemm_args_of(*d), family, config, stream);
}
// ... with the output row map (GemmArgs::rm_*): the families that implement it run it, every other launcher refuses
int d4_gemm_run_rowmap(const d4_gemm_desc* d, int family, int config, int rm_Sc, int rm_S, int rm_lo, int rm_nr, void* stream) {
    if (int rc = gemm_desc_check("d4_gemm_run_rowmap", d)) return rc;
    D4_REQUIRE(rm_Sc >= 1 && rm_nr >= 0 && rm_lo >= 0 && rm_lo <= rm_Sc && rm_S == rm_Sc + rm_nr && rm_S <= 65535, "d4_gemm_run_rowmap: bad row map (Sc=%d S=%d lo=%d nr=%d)", rm_Sc, rm_S, rm_lo, rm_nr);
    d4::GemmArgs g = gemm_args_of(*d);
    g.rm_Sc = (uint16_t)rm_Sc; g.rm_lo = (uint16_t)rm_lo; g.rm_nr = (uint16_t)rm_nr;
    return gemm_run_args(g, family, config, stream);
}
static int gemm_run_args(const d4::GemmArgs& g, int family, int config, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool al16 = ((uintptr_t)g.A % 16) == 0 && ((uintptr_t)g.W % 16) == 0 && (g.lda % 4) == 0 && (g.ldw % 4) == 0;
#define D4_RUN_REFUSE(cond, why) D4_REQUIRE(cond, "d4_gemm_run: call not supported (family %d, configuration %d, M=%d N=%d K=%d flags=%d: " why ")", family, config, g.M, g.N, g.K, g.flags)
    switch (family) {
        case D4_GEMM_TILE: {
            D4_RUN_REFUSE(d4::gemm_config_valid(config, g), "the dispatcher does not run this configuration of the first family here - few-row shape, mirror weights or an epilogue the tile lacks");
            d4_gemm_force_config(config);
            const int rc = d4::gemm(g, s);
            d4_gemm_force_config(-1);
            return rc;
        }
        case D4_GEMM_V2:
            D4_RUN_REFUSE(al16 && !g.Wb && d4::gemm2_config_valid(config, g), "gemm2_config_valid: K %% 32, lda / ldw %% 4, no transposed operand, SiLU-GLU tiles");
            return d4::gemm2_launch(config, g, s);
        case D4_GEMM_V2_KSPLIT:
            D4_RUN_REFUSE(al16 && d4::gemm2_ksplit_applicable(g), "gemm2_ksplit_applicable: no batch, C2, row scale, bias-free flags other than SiLU; K >= 4 k-tiles");
            return d4::gemm2_ksplit_launch(g, s);
        case D4_GEMM_X3:
            D4_RUN_REFUSE(al16 && !g.wscale && d4::gemm_x3_config_valid(config, g), "gemm_x3_config_valid: three bf16 planes, K %% 32, ldw / plane %% 8, SiLU-GLU tiles");
            return d4::gemm_x3_launch(config, g, s);
        case D4_GEMM_X3SK:
            D4_RUN_REFUSE(al16 && !g.wscale && d4::gemm_x3sk_applicable(g), "gemm_x3sk_applicable: as gemm_x3, no batch");
            return d4::gemm_x3sk_launch(g, s);
        case D4_GEMM_H2:
            D4_RUN_REFUSE(al16 && d4::gemm_h2_config_valid(config, g), "gemm_h2_config_valid: two fp16 planes + row scales, K %% 32, ldw / plane %% 8, SiLU-GLU tiles");
            return d4::gemm_h2_launch(config, g, s);
        case D4_GEMM_SKINNY:
            D4_RUN_REFUSE(al16 && !g.Wb && d4::gemm_skinny_applicable(g) && (!(g.flags & d4::GEMM_SWIGLU) || g.N % 64 == 0),
                          "gemm_skinny_applicable: at most 256 rows and fewer than 64 tiles, K % 4, no transposed operand, C2 without batch");
            return d4::gemm_skinny(g, s);
        case D4_GEMM_BF16: {
            D4_RUN_REFUSE(((uintptr_t)g.A % 16) == 0 && !g.Ab && g.wplane == 0 && d4::gemm_bf16_config_valid(config, g), "gemm_bf16: bf16 weights, K %% 32, lda %% 4, ldw %% 8, SiLU-GLU tiles");
            d4::gemm_bf16_force_config(config);
            const int rc = d4::gemm_bf16(g, s);
            d4::gemm_bf16_force_config(-1);
            return rc;
        }
        case D4_GEMM_BF16A:
            D4_RUN_REFUSE(d4::gemm_bf16a_config_valid(config, g), "gemm_bf16a_config_valid: bf16 images of both operands, K %% 64, lda / ldw %% 8, SiLU-GLU tiles");
            return d4::gemm_bf16a_launch(config, g, s);
    }
    D4_REQUIRE(false, "d4_gemm_run: unknown family %d", family);
#undef D4_RUN_REFUSE
}
// The filled form of the persistent split-operand kernel (gemm_x3sk.hip): `main` in whole tiles with the first `fill_tiles` 128 x 64 tiles of `fill` on the
// workgroups its last round leaves idle; the launcher's refusals come back as errors
int d4_gemm_fill_capacity(const d4_gemm_desc* main) {
    if (!main || main->M < 1 || main->N < 1 || main->K < 1) return 0;
    return d4::gemm_x3sk_fill_capacity(gemm_args_of(*main));
}
int d4_gemm_run_fill(const d4_gemm_desc* main, const d4_gemm_desc* fill, int fill_tiles, void* stream) {
    if (int rc = gemm_desc_check("d4_gemm_run_fill", main)) return rc;
    D4_REQUIRE(fill_tiles == 0 || fill, "d4_gemm_run_fill: fill tiles without a fill descriptor");
    if (fill_tiles != 0) if (int rc = gemm_desc_check("d4_gemm_run_fill", fill)) return rc;
    const d4::GemmArgs g = gemm_args_of(*main);
    D4_REQUIRE(((uintptr_t)g.A % 16) == 0 && (g.lda % 4) == 0 && !g.wscale, "d4_gemm_run_fill: main operands must be 16-byte aligned split-operand planes");
    return d4::gemm_x3sk_fill(g, fill ? gemm_args_of(*fill) : d4::GemmArgs{}, fill_tiles, static_cast<hipStream_t>(stream));
}
// ... with an output row map on the FILL problem (as d4_gemm_run_rowmap): the filled form does not implement it, so this is an error — the entry exists
// so that the refusal can be observed
int d4_gemm_run_fill_rowmap(const d4_gemm_desc* main, const d4_gemm_desc* fill, int fill_tiles, int rm_Sc, int rm_S, int rm_lo, int rm_nr, void* stream) {
    if (int rc = gemm_desc_check("d4_gemm_run_fill_rowmap", main)) return rc;
    if (int rc = gemm_desc_check("d4_gemm_run_fill_rowmap", fill)) return rc;
    D4_REQUIRE(rm_Sc >= 1 && rm_nr >= 0 && rm_lo >= 0 && rm_lo <= rm_Sc && rm_S == rm_Sc + rm_nr && rm_S <= 65535, "d4_gemm_run_fill_rowmap: bad row map (Sc=%d S=%d lo=%d nr=%d)", rm_Sc, rm_S, rm_lo, rm_nr);
    d4::GemmArgs f = gemm_args_of(*fill);
    f.rm_Sc = (uint16_t)rm_Sc; f.rm_lo = (uint16_t)rm_lo; f.rm_nr = (uint16_t)rm_nr;
    return d4::gemm_x3sk_fill(gemm_args_of(*main), f, fill_tiles, static_cast<hipStream_t>(stream));
}
int d4_gemm_run_pair(const d4_gemm_desc* da, const d4_gemm_desc* db, int target, int config, void* stream) {
    if (int rc = gemm_desc_check("d4_gemm_run_pair", da)) return rc;
    if (int rc = gemm_desc_check("d4_gemm_run_pair", db)) return rc;
    const d4::GemmArgs a = gemm_args_of(*da), b = gemm_args_of(*db);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto al16 = [](const d4::GemmArgs& g) { return ((uintptr_t)g.A % 16) == 0 && ((uintptr_t)g.W % 16) == 0 && (g.lda % 4) == 0 && (g.ldw % 4) == 0; };
    switch (target) {
        case D4_PAIR_SKINNY:
            D4_REQUIRE(al16(a) && al16(b) && d4::gemm_skinny_pair_applicable(a, b),
                       "d4_gemm_run_pair: call not supported (gemm_skinny_pair_applicable: two few-row products of equal K, no SiLU-GLU, batch or mirror weights)");
            return d4::gemm_skinny_pair(a, b, s);
        case D4_PAIR_BF16A:
            D4_REQUIRE(d4::gemm_bf16a_pair_applicable(a, b),
                       "d4_gemm_run_pair: call not supported (gemm_bf16a_pair_applicable: equal K, flags == RMS, no bias / R / C2 / batch, a 64 x 64 or 128 x 64 tile by the rule)");
            return d4::gemm_bf16a_pair_launch(a, b, s);
        case D4_PAIR_V2:
            D4_REQUIRE(al16(a) && al16(b) && !a.Wb && !b.Wb && a.K == b.K && d4::gemm2_pair_config_ok(config) && d4::gemm2_pair_applicable(a, b) &&
                       d4::gemm2_config_valid(config, a) && d4::gemm2_config_valid(config, b),
                       "d4_gemm_run_pair: call not supported (gemm2 pair configuration %d: gemm2_pair_config_ok / gemm2_pair_applicable)", config);
            return d4::gemm2_pair_launch(config, a, b, s);
    }
    D4_REQUIRE(false, "d4_gemm_run_pair: unknown target %d", target);
}

// ... and of the per-frame fused block tails (frame_fused.hip)
int d4_tile16_weights(const float* W, int ldw, float* Wt, int N, int K, void* stream) {
    D4_REQUIRE(W && Wt && N >= 16 && K >= 4 && ldw >= K && ((uintptr_t)W % 16) == 0 && ((uintptr_t)Wt % 16) == 0, "d4_tile16_weights: bad arguments");
    return d4::tile16_weights(W, ldw, Wt, N, K, static_cast<hipStream_t>(stream));
}
static d4::SmallAttnArgs frame_attn_args(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                                         const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                                         const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                                         int64_t m_item_stride, uint16_t* out_b, int frames, int heads, int S, float softclamp, int mask_special, int belief, int dh) {
    d4::SmallAttnArgs sa{};
    sa.q = q; sa.q_group_stride = q_group_stride; sa.q_item_stride = q_item_stride;
    sa.k = k; sa.k_group_stride = k_group_stride; sa.k_item_stride = k_item_stride;
    sa.v = v; sa.v_group_stride = v_group_stride; sa.v_item_stride = v_item_stride;
    sa.gate = gate; sa.g_group_stride = g_group_stride; sa.g_item_stride = g_item_stride;
    sa.k_gamma = k_gamma;
    sa.vres = vres; sa.r_group_stride = r_group_stride; sa.r_item_stride = r_item_stride;
    sa.mix = mix; sa.m_group_stride = m_group_stride; sa.m_item_stride = m_item_stride;
    sa.out_b = out_b;
    sa.groups = frames; sa.heads = heads; sa.nq = S; sa.nk = S;
    sa.softclamp = softclamp; sa.mask_special = mask_special; sa.belief = belief; sa.dh = dh;
    return sa;
}
static int frame_out_check(const char* who, const float* resid, const float* out, const float* c2, int S, int c2_lo, int c2_hi, int c2_last) {
    D4_REQUIRE(resid && out && ((uintptr_t)resid % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)c2 % 16) == 0, "%s: residual / output missing or not 16-byte aligned", who);
    D4_REQUIRE(!c2 || (c2_lo >= 0 && c2_hi >= c2_lo && c2_hi <= S && (c2_last == 0 || c2_last == 1)), "%s: bad compaction arguments", who);
    return 0;
}
int d4_frame_attn_out(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                      const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                      const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                      int64_t m_item_stride, uint16_t* out_b, int frames, int heads, int S, float softclamp, int mask_special, int belief, int dh,
                      const float* wo_t, int D, const float* resid, int ldr, float* out, int ldo, float* c2, int ldc2, int c2_lo, int c2_hi, int c2_last,
                      void* stream) {
    const d4::SmallAttnArgs sa = frame_attn_args(q, q_group_stride, q_item_stride, k, k_group_stride, k_item_stride, v, v_group_stride, v_item_stride, gate, g_group_stride,
                                                 g_item_stride, k_gamma, vres, r_group_stride, r_item_stride, mix, m_group_stride, m_item_stride, out_b, frames, heads, S,
                                                 softclamp, mask_special, belief, dh);
    if (int rc = frame_out_check("d4_frame_attn_out", resid, out, c2, S, c2_lo, c2_hi, c2_last)) return rc;
    D4_REQUIRE(wo_t && ((uintptr_t)wo_t % 16) == 0 && ldr >= D && ldo >= D && (!c2 || ldc2 >= D), "d4_frame_attn_out: weight image missing / misaligned or a leading dimension below D");
    return d4::frame_attn_out(sa, wo_t, D, resid, ldr, out, ldo, c2, ldc2, c2_lo, c2_hi, c2_last, static_cast<hipStream_t>(stream));
}
int d4_attn_out_cols(const float* q, int64_t q_group_stride, int64_t q_item_stride, const float* k, int64_t k_group_stride, int64_t k_item_stride,
                     const float* v, int64_t v_group_stride, int64_t v_item_stride, const float* gate, int64_t g_group_stride, int64_t g_item_stride,
                     const float* k_gamma, const float* vres, int64_t r_group_stride, int64_t r_item_stride, const float* mix, int64_t m_group_stride,
                     int64_t m_item_stride, uint16_t* out_b, int frames, int heads, int S, float softclamp, int mask_special, int belief, int dh,
                     const float* W, int ldw, int D, const float* resid, int ldr, float* out, int ldo, float* c2, int ldc2, int c2_lo, int c2_hi, int c2_last,
                     void* stream) {
    const d4::SmallAttnArgs sa = frame_attn_args(q, q_group_stride, q_item_stride, k, k_group_stride, k_item_stride, v, v_group_stride, v_item_stride, gate, g_group_stride,
                                                 g_item_stride, k_gamma, vres, r_group_stride, r_item_stride, mix, m_group_stride, m_item_stride, out_b, frames, heads, S,
                                                 softclamp, mask_special, belief, dh);
    D4_REQUIRE(resid && out && (!c2 || (c2_lo >= 0 && c2_hi >= c2_lo && c2_hi <= S && (c2_last == 0 || c2_last == 1))), "d4_attn_out_cols: residual / output missing or bad compaction arguments");
    D4_REQUIRE(W && ldw >= heads * 64 && ldr >= D && ldo >= D && (!c2 || ldc2 >= D), "d4_attn_out_cols: weights missing or a leading dimension below its width");
    return d4::attn_out_cols(sa, W, ldw, D, resid, ldr, out, ldo, c2, ldc2, c2_lo, c2_hi, c2_last, static_cast<hipStream_t>(stream));
}
int d4_frame_pool(const float* q, int ldq, const float* x, int ldx, const float* gate_w, const float* k, int ldk, const float* hid, int D,
                  const float* k_gamma, int M, int L, int heads, float eps, const float* wv_t, const float* wo_t, int frames, int S, const float* resid,
                  int ldr, float* out, int ldo, float* c2, int ldc2, int c2_lo, int c2_hi, int c2_last, void* stream) {
    d4::PoolMixArgs pm{};
    pm.q = q; pm.ldq = ldq; pm.x = x; pm.ldx = ldx; pm.gate_w = gate_w; pm.k = k; pm.ldk = ldk; pm.hid = hid; pm.D = D; pm.k_gamma = k_gamma;
    pm.M = M; pm.L = L; pm.heads = heads; pm.eps = eps;
    if (int rc = frame_out_check("d4_frame_pool", resid, out, c2, S, c2_lo, c2_hi, c2_last)) return rc;
    D4_REQUIRE(x && gate_w && hid && k_gamma && wv_t && wo_t && ((uintptr_t)wv_t % 16) == 0 && ((uintptr_t)wo_t % 16) == 0 && ((uintptr_t)q % 16) == 0 &&
               ((uintptr_t)k % 16) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)hid % 16) == 0 && ((uintptr_t)gate_w % 16) == 0 && ((uintptr_t)k_gamma % 16) == 0 &&
               ldq % 4 == 0 && ldk % 4 == 0 && ldx % 4 == 0 && ldq >= heads * 64 && ldk >= heads * 64 && ldx >= D && ldr >= D && ldo >= D && (!c2 || ldc2 >= D),
               "d4_frame_pool: operand missing / not 16-byte aligned or a leading dimension below its width");
    return d4::frame_pool(pm, wv_t, wo_t, frames, S, resid, ldr, out, ldo, c2, ldc2, c2_lo, c2_hi, c2_last, static_cast<hipStream_t>(stream));
}
int d4_frame_pool_tail(const float* u, const float* wv_t, const float* wo_t, int frames, int S, int D, int pool_heads, const float* resid, int ldr,
                       float* out, int ldo, float* c2, int ldc2, int c2_lo, int c2_hi, int c2_last, void* stream) {
    if (int rc = frame_out_check("d4_frame_pool_tail", resid, out, c2, S, c2_lo, c2_hi, c2_last)) return rc;
    D4_REQUIRE(u && wv_t && wo_t && ((uintptr_t)u % 16) == 0 && ((uintptr_t)wv_t % 16) == 0 && ((uintptr_t)wo_t % 16) == 0 && ldr >= D && ldo >= D && (!c2 || ldc2 >= D),
               "d4_frame_pool_tail: operand missing / not 16-byte aligned or a leading dimension below D");
    return d4::frame_pool_tail(u, wv_t, wo_t, frames, S, D, pool_heads, resid, ldr, out, ldo, c2, ldc2, c2_lo, c2_hi, c2_last, static_cast<hipStream_t>(stream));
}

int d4_rmsnorm_backward(const float* x, const float* dy, const float* gamma, float* dx, float* d_gamma, float* scratch, int rows, int dim, float eps, void* stream) {
    D4_REQUIRE(x && dy && gamma && dx && d_gamma && scratch, "d4_rmsnorm_backward: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rows == 0) return 0;
    if (int rc = d4::rmsnorm_bwd(x, dy, gamma, scratch, dx, rows, dim, eps, s)) return rc;
    return d4::colsum(scratch, dim, rows, dim, d_gamma, s);
}

// MultiCategorical.sample + log_prob of the sample (D4:485-497, 1374-1376, 1422-1423), stateless: Gumbel-max per action type from injected
// uniforms (same shape as the logits), log-softmax gather.  action_sizes: device [na].
int d4_categorical_sample_logp(const float* logits, int ld, const float* uniform, int ld_u, const int32_t* action_sizes, int rows, int na,
                               float temperature, int64_t* actions, float* log_probs, void* stream) {
    D4_REQUIRE(logits && uniform && action_sizes && actions && log_probs && rows >= 0 && na >= 1, "d4_categorical_sample_logp: bad arguments");
    d4::SampleArgs sa{};
    sa.logits = logits; sa.ld = ld; sa.gumbel_u = uniform; sa.ld_u = ld_u; sa.actions = actions; sa.act_stride = na; sa.log_probs = log_probs;
    sa.lp_stride = na; sa.action_sizes = action_sizes; sa.B = rows; sa.na = na; sa.temperature = temperature;
    return d4::sample_actions_terminals(sa, static_cast<hipStream_t>(stream));
}
int d4_hl_gauss_scalar(const float* logits, int ld, const float* centers, float* out, int rows, int bins, void* stream) {
    return d4::hl_gauss_scalar(logits, ld, centers, out, 1, rows, bins, static_cast<hipStream_t>(stream));
}

}  // extern "C"
