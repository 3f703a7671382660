"""Plain references of the glue launchers that tests/test_gpu_glue.py calls alone: the row norms of csrc/elementwise.hip (rmsnorm_rows,
layernorm_rows, gather_space_double_norm), the token assembly, its index permutations, pointwise kernels and small sums, the bf16 image builders
of csrc/gemm_bf16.hip and csrc/gemm_tn_bf16.hip (cvt_rows_bf16, cvt_f32_to_bf16, cvt_pad_bf16, cvt_transpose_bf16),
and the reductions, the RMSNorm backward and the optimiser step of csrc/learn.hip (colsum, colsum_batch, rmsnorm_bwd, d4_adamw_clip).  Logical
tensors only: no strides, no grids, no chunks.  Every numeric function takes a `dtype` (float64: the reference of the GPU tests; float32: the same
code at the kernels' precision, whose distance to float64 is the E32 of glue_cases.py).  A float32 reduction over rows (colsum) or over a whole
gradient (the AdamW norm) is summed strictly one term after the other, the least accurate order there is, so E32 bounds every order a kernel may
choose; the kernels' trees are more accurate.

`mut` names deliberate mistakes (tests/test_glue_host.py shows that the inputs and the bound of the GPU tests can see each):
    last_row       the last row of the output is never written (reads 0 here); for colsum the last row is not summed
    last_col       the last column is not written and is missing from the row statistics
    last_f4        the same for the last four columns (the last float4 of the register forms)
    no_gamma       the (first) gain ignored
    no_eps         eps dropped
    no_second      the second norm of the double norm skipped
    first_zero     the double norm gathers from token 0 instead of `first`
    no_mean        LayerNorm without subtracting the mean
    var_dm1        LayerNorm with the unbiased variance (D - 1)
    no_bias        the LayerNorm bias ignored
    no_silu        the SiLU skipped
    no_proj        RMSNorm backward without the projection onto x
    skip64         colsum: the row at index 64 skipped
    last_chunk     colsum: the last of the 16 row chunks dropped
    first_off      colsum_batch: `first[]` off by one block (the first 16 columns of a sum come from its neighbour's last block)
    truncate       bf16 by truncation instead of round-to-nearest-even
    no_offset      assemble_tokens: the action offsets ignored
    no_sentinel    assemble_tokens: the -1 / NaN sentinel ignored (the frame gets an action token built from index 0 / value 0)
    rank_off       assemble_tokens: the agent row of the compact copy one rank early
    no_task        assemble_tokens: the task embedding not added
    no_bias_corr   AdamW without bias correction
    l2_decay       AdamW with the decay added to the gradient (L2) instead of decoupled
    clip_always    the clip coefficient applied even when the norm is below max_norm
    scale_not_in_norm   grad_scale left out of the norm
    tail           AdamW: the elements past one trip of the grid (the last element of a short group) never updated
    last_slice     splitk_reduce: the last k-slice not added
    last_token     mean_tokens: the last token not added
    sum_not_mean   mean_tokens: the division by n left out
    no_div         euler_step: the division by 1 - t left out
    pad_unzeroed   bf16 images, pad_cols, coord_grid: the padding columns / rows left as they were (NaN here)
    swap_hw, swap_p, swap_th, swap_bcol   a permutation with two adjacent axes exchanged (h with w, p1 with p2, t with h; cache: batch column with head)
    batch_as_b     cache_transfer: cache_batch taken as B
    tcap_as_frames cache_transfer: Tcap taken as frames
    head1          cunembed: prediction head 1 read / written instead of head 0
    all_latents    decoder pack: latent row s read at stride n_lat instead of n_total
    gate_first     swiglu_pack_rows: the gate rows packed in front of their value rows
    stride_as_tq   build_latent_input: the history read at a frame stride of Tq
    no_last        build_latent_input: the last frame taken from the history like the others
    no_base        prep_eval_inputs: frame_base ignored (every evaluation read as if it began at global frame 0)
    sig_only       silu_bwd, layernorm_silu_bwd, swiglu_bwd: SiLU' taken as the sigmoid alone (its z (1 - sigmoid) term dropped)
    no_mean_term   layernorm_silu_bwd: the mean of g dy not subtracted from dz
    halves_swapped swiglu: the value half and the gate half of h exchanged
    no_zero        multi_copy: a null source leaves its destination as it was
    ld_as_n        zero_pad_cols: the rows taken at a stride of c1 - c0 instead of ld"""
import numpy as np
import torch

from attn_core_ref import rel_err

MUTATIONS = ('last_row', 'last_col', 'last_f4', 'no_gamma', 'no_eps', 'no_second', 'first_zero', 'no_mean', 'var_dm1', 'no_bias', 'no_silu', 'no_proj',
             'skip64', 'last_chunk', 'first_off', 'truncate', 'no_offset', 'no_sentinel', 'rank_off', 'no_task', 'no_bias_corr', 'l2_decay', 'clip_always',
             'scale_not_in_norm', 'tail', 'last_slice', 'last_token', 'sum_not_mean', 'no_div', 'pad_unzeroed', 'swap_hw', 'swap_p', 'swap_th', 'swap_bcol',
             'batch_as_b', 'tcap_as_frames', 'head1', 'all_latents', 'gate_first', 'stride_as_tq', 'no_last', 'no_base', 'sig_only', 'no_mean_term', 'halves_swapped', 'no_zero', 'ld_as_n')


def rel_err_all(got, want):
    """Largest rel_err over the pairs of two results (tuples; a None reference is an output the call does not write)."""
    return max(rel_err(g, w) for g, w in zip(got, want) if w is not None)


def _drop(y, stat_cols, mut):
    """The not-written rows / columns of a row-norm output."""
    if 'last_row' in mut or stat_cols < y.shape[-1]:
        y = y.clone()
    if 'last_row' in mut:
        y[-1] = 0
    y[..., stat_cols:] = 0
    return y


def _stat_cols(D, mut):
    return max(D - 4, 0) if 'last_f4' in mut else D - 1 if 'last_col' in mut else D


def _rms(x, D, eps, n=None):
    """1 / sqrt(mean over D of the first n columns' squares + eps)"""
    xs = x if n is None else x[..., :n]
    return torch.rsqrt((xs * xs).sum(-1, keepdim=True) / D + eps)


# ------------------------------------------------------------------------------------------------------------------- row norms
def rmsnorm_ref(x, gamma, *, eps, dtype=torch.float64, mut=()):
    """x [rows, D]; gamma [D] or None  ->  x / sqrt(mean(x^2) + eps) * gamma"""
    x = x.to(dtype)
    D = x.shape[-1]
    n = _stat_cols(D, mut)
    y = x * _rms(x, D, 0. if 'no_eps' in mut else eps, n)
    if gamma is not None and 'no_gamma' not in mut:
        y = y * gamma.to(dtype)
    return _drop(y, n, mut)


def layernorm_ref(x, g, b, *, eps, silu, dtype=torch.float64, mut=()):
    """x [rows, D]; g [D]; b [D] or None  ->  (x - mean) / sqrt(var + eps) * g + b (biased variance), then SiLU when `silu`"""
    x, g = x.to(dtype), g.to(dtype)
    D = x.shape[-1]
    n = _stat_cols(D, mut)
    xs = x[..., :n]
    mean = xs.sum(-1, keepdim=True) / D
    d = x if 'no_mean' in mut else x - mean
    var = (d[..., :n] * d[..., :n]).sum(-1, keepdim=True) / (D - 1 if 'var_dm1' in mut else D)
    y = d * torch.rsqrt(var + (0. if 'no_eps' in mut else eps)) * g
    if b is not None and 'no_bias' not in mut:
        y = y + b.to(dtype)
    if silu and 'no_silu' not in mut:
        y = torch.nn.functional.silu(y)
    return _drop(y, n, mut)


def gather_space_ref(tokens, g0, g1, *, first, ns, eps, dtype=torch.float64, mut=()):
    """tokens [frames, S, D]  ->  [frames * ns, D]: RMSNorm(g1)(RMSNorm(g0)(tokens[:, first : first + ns]))"""
    t, g0, g1 = tokens.to(dtype), g0.to(dtype), g1.to(dtype)
    lo = 0 if 'first_zero' in mut else first
    x = t[:, lo:lo + ns].reshape(-1, t.shape[-1])
    D = x.shape[-1]
    n = _stat_cols(D, mut)
    e = 0. if 'no_eps' in mut else eps
    y = x * _rms(x, D, e, n)
    if 'no_gamma' not in mut:
        y = y * g0
    if 'no_second' not in mut:
        y = y * _rms(y, D, e, n)
    return _drop(y * g1, n, mut)


def rmsnorm_bwd_ref(x, dxhat, gamma, *, eps, want_dx=True, dtype=torch.float64, mut=()):
    """x, dxhat [rows, D]; gamma [D]  ->  (tg = dxhat * x * rstd, dx = rstd * (gamma dxhat - x rstd^2 mean(gamma dxhat x)) or None)"""
    x, g, gamma = x.to(dtype), dxhat.to(dtype), gamma.to(dtype)
    D = x.shape[-1]
    if 'no_gamma' in mut:
        gamma = torch.ones_like(gamma)
    rstd = _rms(x, D, 0. if 'no_eps' in mut else eps)
    tg = g * x * rstd
    dot = (gamma * g * x).sum(-1, keepdim=True) / D
    dx = rstd * (gamma * g - (0. if 'no_proj' in mut else x * rstd * rstd * dot))
    if 'last_row' in mut:
        tg, dx = tg.clone(), dx.clone()
        tg[-1] = 0
        dx[-1] = 0
    return tg, (dx if want_dx else None)


# ------------------------------------------------------------------------------------------------------------------- reductions
def _sum_rows(x, dtype):
    """Column sums of x [rows, cols]: float64 by torch; float32 one row after the other in float32 (numpy's cumulative sum keeps the dtype)."""
    if dtype == torch.float64:
        return x.double().sum(0)
    if x.shape[0] == 0:
        return torch.zeros(x.shape[1], dtype=torch.float32)
    return torch.from_numpy(np.cumsum(x.numpy().astype(np.float32), axis=0, dtype=np.float32)[-1].copy())


def colsum_ref(x, *, dtype=torch.float64, mut=()):
    """x [rows, cols] -> [cols]"""
    rows = x.shape[0]
    keep = torch.ones(rows, dtype=torch.bool)
    if 'skip64' in mut:
        keep[64] = False
    if 'last_row' in mut:
        keep[rows - 1] = False
    if 'last_chunk' in mut:                                  # the chunk length of the two-launch form: rows / 16 rounded up to 64
        chunk = -(-(-(-rows // 16)) // 64) * 64
        keep[(-(-rows // chunk) - 1) * chunk:] = False
    y = _sum_rows(x[keep], dtype)
    if 'last_col' in mut:
        y[-1] = 0
    return y


def colsum_batch_ref(mats, *, dtype=torch.float64, mut=()):
    """[x_i [rows_i, cols_i]] -> [colsum_i]"""
    outs = [colsum_ref(x, dtype=dtype) for x in mats]
    if 'first_off' in mut:
        for i in range(len(mats) - 1, 0, -1):
            prev = outs[i - 1]
            blk = prev[(len(prev) - 1) // 16 * 16:]
            k = min(len(blk), 16, len(outs[i]))
            outs[i][:16] = 0
            outs[i][:k] = blk[:k]
    return outs


# ------------------------------------------------------------------------------------------------------------------- bf16 images
def bf16_ref(x, mut=()):
    """x (float32) -> bf16, round-to-nearest-even (torch's conversion)"""
    if 'truncate' in mut:
        return (x.contiguous().view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)
    y = x.to(torch.bfloat16)
    if 'last_row' in mut or 'last_col' in mut:
        y = y.clone()
        if 'last_row' in mut:
            y[-1] = 0
        else:
            y[..., -1] = 0
    return y


def cvt_pad_ref(x, cols_pad, mut=()):
    """x [rows, cols] -> bf16 [rows, cols_pad], zeros in the padding columns"""
    y = torch.full((x.shape[0], cols_pad), float('nan') if 'pad_unzeroed' in mut else 0., dtype=torch.bfloat16)
    y[:, :x.shape[1]] = bf16_ref(x, mut)
    return y


def cvt_transpose_ref(x, rows_pad, mut=()):
    """x [rows, cols] -> bf16 [cols, rows_pad] = x^T, zeros in the padding rows of x"""
    return cvt_pad_ref(x.t().contiguous(), rows_pad, mut)


# ------------------------------------------------------------------------------------------------------------------- index permutations (exact)
NAN = float('nan')


def pad_cols_ref(W, cols_pad, mut=()):
    y = torch.full((W.shape[0], cols_pad), NAN if 'pad_unzeroed' in mut else 0.)
    y[:, :W.shape[1]] = W
    if 'last_row' in mut:
        y[-1] = 0
    return y


def video_to_patches_ref(video, ps, mut=()):
    """video [B, C, T, nh * ps, nw * ps] -> [(b t h w), (p1 p2 c)]"""
    B, C, T, H, W = video.shape
    v = video.reshape(B, C, T, H // ps, ps, W // ps, ps)                    # b c t h p1 w p2
    order = [0, 2, 3, 5, 4, 6, 1]                                           # b t h w p1 p2 c
    if 'swap_hw' in mut:
        order = [0, 2, 5, 3, 4, 6, 1]
    if 'swap_p' in mut:
        order = [0, 2, 3, 5, 6, 4, 1]
    if 'swap_th' in mut:
        order = [0, 3, 2, 5, 4, 6, 1]
    return v.permute(*order).reshape(B * T * (H // ps) * (W // ps), ps * ps * C).contiguous()


def patches_to_video_ref(patches, B, C, T, nh, nw, ps, mut=()):
    p = patches.reshape(B, T, nh, nw, ps, ps, C)                            # b t h w p1 p2 c
    if 'swap_hw' in mut:
        p = p.reshape(B, T, nw, nh, ps, ps, C).transpose(2, 3)
    if 'swap_p' in mut:
        p = p.transpose(4, 5)
    return p.permute(0, 6, 1, 2, 4, 3, 5).reshape(B, C, T, nh * ps, nw * ps).contiguous()


def cache_to_ext_ref(cache, B, S, frames, mut=()):
    """cache [Lt, 2, cache_batch * S, H, Tcap, dh] -> [Lt, 2, B * S, H, frames, dh] (the first B * S columns, the first `frames` positions)"""
    Lt, _, cols, H, Tcap, dh = cache.shape
    if 'batch_as_b' in mut:                                                 # the cache read as if it held B * S columns per (layer, k / v)
        cache = cache.reshape(-1)[:Lt * 2 * B * S * H * Tcap * dh].reshape(Lt, 2, B * S, H, Tcap, dh)
    if 'tcap_as_frames' in mut:
        cache = cache.reshape(-1)[:Lt * 2 * cache.shape[2] * H * frames * dh].reshape(Lt, 2, cache.shape[2], H, frames, dh)
    if 'swap_bcol' in mut:
        cache = cache.reshape(Lt, 2, H, -1, cache.shape[4], dh).transpose(2, 3)
    return cache[:, :, :B * S, :, :frames].contiguous()


def ext_to_cache_ref(ext, cache0, mut=()):
    """ext [Lt, 2, B * S, H, frames, dh] written into a copy of cache0 [Lt, 2, cache_batch * S, H, Tcap, dh] (NaN where nothing is written)"""
    Lt, _, cols, H, Tcap, dh = cache0.shape
    bs, frames = ext.shape[2], ext.shape[4]
    out = cache0.clone()
    if 'batch_as_b' in mut:                                                 # the cache written as if it held B * S columns per (layer, k / v)
        out.reshape(-1)[:Lt * 2 * bs * H * Tcap * dh].reshape(Lt, 2, bs, H, Tcap, dh)[:, :, :, :, :frames] = ext
    elif 'tcap_as_frames' in mut:
        out.reshape(-1)[:Lt * 2 * cols * H * frames * dh].reshape(Lt, 2, cols, H, frames, dh)[:, :, :bs] = ext
    elif 'swap_bcol' in mut:
        out.reshape(Lt, 2, H, cols, Tcap, dh)[:, :, :, :bs, :frames] = ext.transpose(2, 3)
    else:
        out[:, :, :bs, :, :frames] = ext
    return out


def cunembed_gather_ref(U, mut=()):
    """U [nc, mtp, d, 2] -> [2 nc, d], row 2 n + t = U[n, 0, :, t]"""
    return U[:, 1 if 'head1' in mut else 0].permute(0, 2, 1).reshape(-1, U.shape[2]).contiguous()


def cunembed_scatter_ref(g, nc, mtp, d, mut=()):
    dU = torch.zeros(nc, mtp, d, 2)
    dU[:, 1 if 'head1' in mut else 0] = g.reshape(nc, 2, d).permute(0, 2, 1)
    return dU


def _linspace_fma(n):
    """torch.linspace(-1, 1, n) in float32 as the kernel forms it: -1 + step k in the first half, 1 - step (n - 1 - k) in the second, each one fused
    multiply-add (exact wherever step k is exact; n = 1 -> -1)"""
    if n == 1:
        return torch.tensor([-1.])
    k = torch.arange(n, dtype=torch.float32)
    step = torch.tensor(2., dtype=torch.float32) / torch.tensor(float(n - 1), dtype=torch.float32)
    return torch.where(k < n // 2, _fma32(step, k, torch.tensor(-1.)), _fma32(-step, (n - 1) - k, torch.tensor(1.)))


def coord_grid_ref(nh, nw, ld, mut=()):
    """[nh * nw, ld]: column 0 the row coordinate, column 1 the column coordinate, the rest zero"""
    out = torch.full((nh, nw, ld), NAN if 'pad_unzeroed' in mut else 0.)
    out[..., 1 if 'swap_hw' in mut else 0] = _linspace_fma(nh)[:, None]
    out[..., 0 if 'swap_hw' in mut else 1] = _linspace_fma(nw)[None, :]
    return out.reshape(nh * nw, ld)


def fold_rows_ref(W, gamma, mut=()):
    """W [rows, K] * gamma [K] in float32 (one correctly rounded product per element); gamma None: W"""
    y = W.clone() if gamma is None or 'no_gamma' in mut else W * gamma
    if 'last_row' in mut:
        y[-1] = 0
    return y


def swiglu_pack_ref(W, bias, gamma, inner, inner_pad, mut=()):
    """W [2 inner, K], bias [2 inner] -> (Wp [2 inner_pad, K], bp [2 inner_pad]): per 64 packed rows 32 value rows then their 32 gate rows"""
    K = W.shape[1]
    fill = NAN if 'pad_unzeroed' in mut else 0.
    Wp, bp = torch.full((inner_pad // 32, 2, 32, K), fill), torch.full((inner_pad // 32, 2, 32), fill)
    Wg = W if 'no_gamma' in mut else W * gamma
    for part in (0, 1):
        rows = torch.full((inner_pad, K), fill)
        rows[:inner] = Wg[part * inner:(part + 1) * inner]
        b = torch.full((inner_pad,), fill)
        b[:inner] = bias[part * inner:(part + 1) * inner]
        slot = 1 - part if 'gate_first' in mut else part
        Wp[:, slot], bp[:, slot] = rows.reshape(-1, 32, K), b.reshape(-1, 32)
    return Wp.reshape(2 * inner_pad, K), bp.reshape(2 * inner_pad)


def build_latent_ref(hist, ctx, x, *, Tq, w, dtype=torch.float64, mut=()):
    """hist, ctx [B, stride, n_el] (ctx None: hist); x [B, n_el] -> [B, Tq, n_el]: lerp(hist, ctx, w) for t < Tq - 1, x at the last frame"""
    h, x = hist.to(dtype), x.to(dtype)
    c = h if ctx is None else ctx.to(dtype)
    if 'stride_as_tq' in mut:
        B, n = h.shape[0], h.shape[2]
        h, c = (t.reshape(-1)[:B * Tq * n].reshape(B, Tq, n) for t in (h, c))
    out = (h + w * (c - h) if abs(w) < 0.5 else c - (c - h) * (1. - w))[:, :Tq].clone()      # torch.lerp's two forms: exact at w = 0 and at w = 1
    if 'no_last' not in mut:
        out[:, Tq - 1] = x
    return out


def decoder_pack_ref(pos, img, lat, n_lat, mut=()):
    """pos [P, D]; img [frames, P, D]; lat [frames, n_total, D] -> (tokens [frames, P + n_lat, D], compact [frames, P, D])"""
    patch = pos[None] + img
    l = lat.reshape(-1, lat.shape[-1])[:lat.shape[0] * n_lat].reshape(lat.shape[0], n_lat, -1) if 'all_latents' in mut else lat[:, :n_lat]
    return torch.cat([patch, l], 1), patch.clone()


def encoder_pack_ref(img, lt, mut=()):
    """img [frames, P, D]; lt [n, D] -> (tokens [frames, P + n, D], compact [frames, n, D])"""
    l = lt[None].expand(img.shape[0], *lt.shape)
    if 'last_row' in mut:
        l = l.clone()
        l[-1, -1] = 0
    return torch.cat([img, l], 1), l.clone()


# ------------------------------------------------------------------------------------------------------------------- pointwise and small sums
def _seq_sum(terms, dtype):
    """terms [n, ...] added in order (a float32 sum in the kernels' order; float64: order is immaterial at these lengths)"""
    s = torch.zeros_like(terms[0])
    for t in terms:
        s = s + t
    return s


def splitk_reduce_ref(part, bias, *, silu, dtype=torch.float64, mut=()):
    """part [S, M, N]; bias [N] or None -> act(sum_s part + bias)"""
    p = part.to(dtype)
    y = _seq_sum(p[:-1] if 'last_slice' in mut else p, dtype)
    if bias is not None and 'no_bias' not in mut:
        y = y + bias.to(dtype)
    if silu and 'no_silu' not in mut:
        y = torch.nn.functional.silu(y)
    return _drop(y, y.shape[-1] - (1 if 'last_col' in mut else 0), mut)


def mean_tokens_ref(x, *, dtype=torch.float64, mut=()):
    """x [B, n, d] -> [B, d]"""
    x = x.to(dtype)
    n = x.shape[1]
    y = _seq_sum(x.transpose(0, 1)[:n - 1 if 'last_token' in mut else n], dtype)
    if 'sum_not_mean' not in mut:
        y = y / n
    return _drop(y, y.shape[-1] - (1 if 'last_col' in mut else 0), mut)


def hl_gauss_scalar_ref(logits, centers, *, dtype=torch.float64, mut=()):
    """logits [rows, bins]; centers [bins] -> softmax(logits) . centers [rows]"""
    l, c = logits.to(dtype), centers.to(dtype)
    if 'last_col' in mut:
        l, c = l[:, :-1], c[:-1]
    y = torch.softmax(l, -1) @ c
    if 'last_row' in mut:
        y[-1] = 0
    return y


def euler_ref(x, pred, *, one_minus_t, dt, dtype=torch.float64, mut=()):
    """x + (pred - x) / (1 - t) * dt on [B, n_el]"""
    x, p = x.to(dtype), pred.to(dtype)
    d = p - x
    y = x + (d if 'no_div' in mut else d / one_minus_t) * dt
    if 'last_row' in mut or 'last_col' in mut:
        y = y.clone()
        if 'last_row' in mut:
            y[-1] = x[-1]
        else:
            y[:, -1] = x[:, -1]
    return y


def unary_ref(x, op, *, dtype=torch.float64, mut=()):
    x = x.to(dtype)
    y = torch.nn.functional.silu(x) if op == 'silu' else torch.tanh(x)
    if 'last_col' in mut:
        y[-1] = 0
    return y


# ------------------------------------------------------------------------------------------------------------------- token assembly
def _fma32(a, b, c):
    """float32 fma(a, b, c): the product of two float32 is exact in float64, one rounding of the sum to float64, then to float32."""
    return (a.double() * b.double() + c.double()).float()


def assemble_ref(c, d, mut=()):
    """tokens [B * Tq, S, D] = [flow | space x ns | registers x nr | action (if na or nc) | agent (if has_agent)] and the compact copy
    [B * Tq, ns + has_agent, D] (None without).  float32 throughout: everything is a copy but the action token (float adds in the kernel's
    order: discrete embeddings, then fma(continuous embedding, value), then the learned token) and the agent token (agent + task)."""
    B, Tq, D, ns, nr, na, nc = c['B'], c['Tq'], c['D'], c['ns'], c['nr'], c['na'], c['nc']
    Fr, S, half = B * Tq, c['S'], c['D'] // 2
    tok = torch.zeros(Fr, S, D)
    lev = d['signal_levels'].long() if d['signal_levels'] is not None else torch.full((Fr,), c['signal_uniform'], dtype=torch.long)
    tok[:, 0, :half] = d['signal_embed'][lev]
    tok[:, 0, half:] = d['step_embed'][c['step_log2']]
    tok[:, 1:1 + ns] = d['space']
    tok[:, 1 + ns:1 + ns + nr] = d['registers']
    if na or nc:
        pa, pc = d['prev_actions'], d['prev_cont']
        have = (pa[:, 0] >= 0) if na else ~pc[:, 0].isnan()
        if 'no_sentinel' in mut:
            have = torch.ones_like(have)
        v = torch.zeros(Fr, D)
        for a in range(na):
            idx = pa[:, a].clamp(min=0) + (0 if 'no_offset' in mut else d['action_offsets'][a].long())
            v = v + d['action_embed'][idx]
        if pc is not None:
            for k in range(nc):
                v = _fma32(d['cont_embed'][k][None], pc[:, k:k + 1].nan_to_num(0.), v)
        v = v + d['action_learned']
        tok[:, 1 + ns + nr] = torch.where(have[:, None], v, torch.zeros(()))
    if c['has_agent']:
        ag = d['agent_embed'][None].expand(Fr, D)
        if d['tasks'] is not None and 'no_task' not in mut:
            ag = ag + d['task_embed'][d['tasks'].long()].repeat_interleave(Tq, 0)
        tok[:, S - 1] = ag
    if 'last_row' in mut:
        tok[-1, -1] = 0
    comp = None
    if c['compact']:
        comp = torch.zeros(Fr, ns + c['has_agent'], D)
        comp[:, :ns] = tok[:, 1:1 + ns]
        if c['has_agent']:
            comp[:, ns - 1 if 'rank_off' in mut else ns] = tok[:, S - 1]
    return tok, comp


# ------------------------------------------------------------------------------------------------------------------- clip_grad_norm_ + AdamW
def _norm_seq32(g):
    """sqrt(sum g^2) with the squares added one after the other in float32"""
    g = g.numpy().astype(np.float32)
    return float(np.sqrt(np.cumsum(g * g, dtype=np.float32)[-1]))


def adamw_ref(p, grads, *, lr, b1, b2, eps, wd, max_norm, grad_scale, dtype=torch.float64, mut=()):
    """p [n], grads [steps, n]: `steps` consecutive clip_grad_norm_ + AdamW steps from zero moments, written out:
        norm = |grad_scale * g|_2;  g' = grad_scale * g * min(1, max_norm / (norm + 1e-6)) (max_norm > 0)
        p *= 1 - lr wd;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    -> [(p, m, v, norm) after each step]"""
    f32 = dtype == torch.float32
    sc = (lambda v: float(np.float32(v))) if f32 else float
    p = p.to(dtype).clone()
    p0 = p.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t in range(1, grads.shape[0] + 1):
        g = grads[t - 1].to(dtype)
        raw = _norm_seq32(g) if f32 else g.norm().item()
        norm = sc(raw * (1. if 'scale_not_in_norm' in mut else sc(grad_scale)))
        coef = sc(grad_scale)
        if max_norm > 0:
            k = sc(sc(max_norm) / sc(norm + 1e-6))
            coef = sc(coef * (k if k < 1. or 'clip_always' in mut else 1.))
        gi = g * coef
        if 'l2_decay' in mut:
            gi = gi + wd * p
        else:
            p = p * sc(1. - sc(lr * wd))
        m = b1 * m + sc(1. - b1) * gi
        v = b2 * v + sc(1. - b2) * gi * gi
        bc1, bc2 = (1., 1.) if 'no_bias_corr' in mut else (sc(1. - sc(b1 ** t)), sc(1. - sc(b2 ** t)))
        p = p - sc(lr / bc1) * (m / (v.sqrt() / sc(bc2 ** 0.5) + eps))
        if 'tail' in mut:                                    # the elements behind one trip of the 4096 x 256 grid (the last one of a short group) keep their state
            lo = min(4096 * 256, len(p) - 1)
            p[lo:], m[lo:], v[lo:] = out[-1][0][lo:] if out else p0[lo:], out[-1][1][lo:] if out else 0., out[-1][2][lo:] if out else 0.
        out.append((p.clone(), m.clone(), v.clone(), torch.tensor([norm], dtype=dtype)))
    return out


# ------------------------------------------------------------------------------------------------------------------- the rest of the glue
def prep_eval_ref(hist, chist, *, B, Tq, na, nc, frame_base, sig_val, ctx_sig, mut=()):
    """hist [B, stride, na] (int64) or None; chist [B, stride, nc] or None -> (sig [B * Tq] int32, pact [B * Tq, na] int64, pcont [B * Tq, nc]):
    frame t of batch b takes the history row frame_base + t - 1; global frame 0, or no history, gives -1 / NaN"""
    sig = torch.full((B, Tq), ctx_sig, dtype=torch.int32)
    sig[:, Tq - 1] = sig_val
    g = (0 if 'no_base' in mut else frame_base) + torch.arange(Tq)
    row = (g - 1).clamp(min=0)
    first = torch.zeros(Tq, dtype=torch.bool) if 'no_sentinel' in mut else g == 0
    out = []
    for h, n, fill, dt in ((hist, na, -1, torch.int64), (chist, nc, NAN, torch.float32)):
        o = torch.full((B, Tq, n), fill, dtype=dt)
        if h is not None and n:
            if 'stride_as_tq' in mut:
                h = h.reshape(-1)[:B * Tq * n].reshape(B, Tq, n)
                row = row.clamp(max=Tq - 1)
            o = torch.where(first[None, :, None], o, h[:, row])
        if 'last_row' in mut and n:
            o[-1, -1] = 0
        out.append(o.reshape(B * Tq, n))
    return sig.reshape(-1), out[0], out[1]


def _dsilu(y, mut):
    s = torch.sigmoid(y)
    return s if 'sig_only' in mut else s * (1. + y * (1. - s))


def layernorm_silu_bwd_ref(z, da, g, b, *, eps, dtype=torch.float64, mut=()):
    """backward of a = SiLU(y), y = LayerNorm(z) g + b on z, da [rows, D] -> (tg = dy zhat, tb = dy, dz = rstd (g dy - mean(g dy) - zhat mean(g dy zhat)))"""
    z, da, g, b = z.to(dtype), da.to(dtype), g.to(dtype), b.to(dtype)
    D = z.shape[-1]
    n = _stat_cols(D, mut)
    mean = z[:, :n].sum(-1, keepdim=True) / D
    d = z - mean
    rstd = torch.rsqrt((d[:, :n] * d[:, :n]).sum(-1, keepdim=True) / D + (0. if 'no_eps' in mut else eps))
    zh = d * rstd
    y = zh * g + (0. if 'no_bias' in mut else b)
    dy = da if 'no_silu' in mut else da * _dsilu(y, mut)
    gd = g * dy
    m1 = 0. if 'no_mean_term' in mut else gd[:, :n].sum(-1, keepdim=True) / D
    m2 = 0. if 'no_proj' in mut else (gd * zh)[:, :n].sum(-1, keepdim=True) / D
    dz = rstd * (gd - m1 - zh * m2)
    return tuple(_drop(t, n, mut) for t in (dy * zh, dy, dz))


def silu_bwd_ref(dy, z, *, dtype=torch.float64, mut=()):
    y = dy.to(dtype) * _dsilu(z.to(dtype), mut)
    if 'last_col' in mut:
        y[-1] = 0
    return y


def _swiglu_halves(h, I, Ip, mut):
    a, g = h[:, :Ip], h[:, Ip:]
    return (g, a) if 'halves_swapped' in mut else (a, g)


def _swiglu_pad(y, I, mut):
    """columns I .. Ip of a half are written as zero; the mutations leave what the formula gives there, or drop a row / the last real column"""
    y = y.clone()
    if 'pad_unzeroed' not in mut:
        y[:, I:] = 0
    if 'last_row' in mut:
        y[-1] = 0
    if 'last_col' in mut:
        y[:, I - 1] = 0
    return y


def swiglu_fwd_ref(h, I, *, dtype=torch.float64, mut=()):
    """h [rows, 2 Ip] = [value | gate] -> u [rows, Ip] = value * SiLU(gate), columns I .. Ip zero"""
    Ip = h.shape[1] // 2
    a, g = _swiglu_halves(h.to(dtype), I, Ip, mut)
    return _swiglu_pad(a * g * torch.sigmoid(g), I, mut)


def swiglu_bwd_ref(h, du, I, *, dtype=torch.float64, mut=()):
    """-> dh [rows, 2 Ip] = [du SiLU(gate) | du value SiLU'(gate)], columns I .. Ip of either half zero"""
    Ip = h.shape[1] // 2
    a, g = _swiglu_halves(h.to(dtype), I, Ip, mut)
    du = du.to(dtype)
    return torch.cat([_swiglu_pad(du * g * torch.sigmoid(g), I, mut), _swiglu_pad(du * a * _dsilu(g, mut), I, mut)], 1)


def multi_copy_ref(segs, src, dst0, mut=()):
    """segs: [(dst offset, src offset or None, n)] into the flat arenas src / dst0 -> dst0 with every segment copied (None: zero-filled)"""
    out = dst0.clone()
    for d, s, n in segs:
        m = n - 1 if 'last_col' in mut else n - (n % 4 or 4) if 'last_f4' in mut else n
        if s is None:
            if 'no_zero' not in mut:
                out[d:d + m] = 0
        else:
            out[d:d + m] = src[s:s + m]
    return out


def zero_pad_cols_ref(x, c0, c1, mut=()):
    """x [rows, ld] with columns c0 .. c1 zero"""
    y = x.clone()
    rows = x.shape[0] - (1 if 'last_row' in mut else 0)
    hi = c1 - (1 if 'last_col' in mut else 0)
    if 'ld_as_n' in mut:
        n = c1 - c0
        f = y.reshape(-1)
        for r in range(rows):
            f[r * n + c0:r * n + c0 + n] = 0
    else:
        y[:rows, c0:hi] = 0
    return y
