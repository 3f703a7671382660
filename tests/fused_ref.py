"""Plain references of the launches only the engine reaches (csrc/frame_fused.hip: frame_attn_out, attn_out_cols, frame_pool,
frame_pool_tail, tile16_weights; the GEMM epilogues' row-compacted second output and accumulating form), on logical tensors: no tiles, no
strides, no k-splitting.  The attention and pool cores are attn_core_ref's.  Every function takes a `dtype` (float64: the reference of the
GPU tests; float32: the same code at the kernels' precision, whose distance to float64 is the E32 of fused_cases.py).

`mut` names deliberate mistakes (tests/test_fused_launches_host.py shows that the inputs and the bound of the GPU tests can see each):
those of attn_core_ref that apply, and
    no_resid      the residual is not added
    tile_swap     the first two 16-row tiles of the output projection's weights exchanged
    k4_swap       the first two 4-wide k groups exchanged inside the first weight tile
    row_shift     every output row of a frame holds its neighbour's values
    rank_off      the compact copy's ranks shifted by one
    last_missing  c2_last ignored: the frame's last token never reaches the compact copy (the row reads 0 here)
    head_swap     the value projections of the first two pool heads exchanged"""
import torch

import attn_core_ref as R

MUTATIONS = ('no_resid', 'tile_swap', 'k4_swap', 'row_shift', 'rank_off', 'last_missing', 'head_swap')


def compact_rows(S, lo, hi, last):
    """Token rows of a frame that the row-compacted copy keeps, in rank order (GemmArgs::C2, FrameOut::c2)."""
    return list(range(lo, hi)) + ([S - 1] if last else [])


def compact_gather(out, c2, mut=()):
    """out [frames, S, N] -> [frames, keep, N], or None without a compaction (c2 = (lo, hi, last))."""
    if c2 is None:
        return None
    lo, hi, last = c2
    rows = compact_rows(out.shape[1], lo, hi, last)
    g = out[:, rows]
    if 'rank_off' in mut:
        g = g.roll(1, dims=1)
    if 'last_missing' in mut and last:
        g = g.clone()
        g[:, -1] = 0
    return g


def _mutate_w(W, mut):
    """W [N, K]: the output projection as the tiled image would hold it after a tiling mistake."""
    if 'tile_swap' in mut or 'k4_swap' in mut:
        W = W.clone()
    if 'tile_swap' in mut:
        W[0:16], W[16:32] = W[16:32].clone(), W[0:16].clone()
    if 'k4_swap' in mut:
        W[0:16, 0:4], W[0:16, 4:8] = W[0:16, 4:8].clone(), W[0:16, 0:4].clone()
    return W


def _project(a, W, resid, mut):
    """a [frames, S, K] @ W[N, K]^T + resid [frames, S, N]"""
    y = a @ _mutate_w(W, mut).t()
    if 'no_resid' not in mut:
        y = y + resid
    if 'row_shift' in mut:
        y = y.roll(1, dims=1)
    return y


def frame_attn_out_ref(q, k, v, gamma, gate, vres, mix, Wo, resid, *, clamp, mask_special, belief, c2=None, dtype=torch.float64, mut=()):
    """Within-frame self attention -> output projection + residual (+ the compact copy).  q, k, v, vres [F, H, S, dh]; gate, mix [F, H, S];
    Wo [D, H * dh]; resid [F, S, D]  ->  (out [F, S, D], c2 [F, keep, D] or None)"""
    o = R.small_attn_ref(q, k, v, gamma, gate, vres, mix, clamp=clamp, mask_special=mask_special, belief=belief, dtype=dtype, mut=mut)
    F, H, S, dh = o.shape
    y = _project(o.permute(0, 2, 1, 3).reshape(F, S, H * dh), Wo.to(dtype), resid.to(dtype), mut)
    return y, compact_gather(y, c2, mut)


def pool_tail_ref(u, Wv, Wo, resid, *, c2=None, dtype=torch.float64, mut=()):
    """AttentionPool tail from the mixes: per-head value projection -> output projection + residual.  u [F, S, 4, D]; Wv [4 * 64, D];
    Wo [D, 4 * 64]; resid [F, S, D]"""
    u, Wv = u.to(dtype), Wv.to(dtype)
    F, S, PH, D = u.shape
    wv = Wv.reshape(PH, 64, D)
    if 'head_swap' in mut:
        wv = wv[[1, 0] + list(range(2, PH))]
    p = torch.einsum('fshd,hjd->fshj', u, wv).reshape(F, S, PH * 64)
    y = _project(p, Wo.to(dtype), resid.to(dtype), mut)
    return y, compact_gather(y, c2, mut)


def frame_pool_ref(q, x, gate_w, k, hid, gamma, Wv, Wo, resid, *, eps, frames, c2=None, dtype=torch.float64, mut=()):
    """pool_mix_ref -> pool_tail_ref.  q [M, 256]; x [M, D]; k [L, M, 256]; hid [L, M, D]; M = frames * S rows"""
    u = R.pool_mix_ref(q, x, gate_w, k, hid, gamma, eps=eps, dtype=dtype, mut=mut)
    M, PH, D = u.shape
    return pool_tail_ref(u.reshape(frames, M // frames, PH, D), Wv, Wo, resid, c2=c2, dtype=dtype, mut=mut)


def tile16_ref(W, N, K):
    """W [N, >= K] -> the image [N / 16][K / 4][16][4] the per-frame kernels stream, as an index permutation."""
    return W[:N, :K].reshape(N // 16, 16, K // 4, 4).permute(0, 2, 1, 3).contiguous()


def gemm_ref(A, W, *, flags=0, bias=None, R_=None, C0=None, eps=1.1920929e-07, ta=False, tb=False, norm=None):
    """float64 epilogue of the GEMM kernels: act(rs * (A W^T) + bias) + R (+ C0 with GEMM_ACCUMULATE).  A [M, K] ([K, M] with ta);
    W [N, K] ([K, N] with tb); flags: 1 folded RMSNorm row scale (of the rows of `norm` when given: the kernel that rounds fp32 activations
    to bf16 takes the scale from the unrounded ones), 2 SiLU, 4 SiLU-GLU on packed (32 value | 32 gate) column groups."""
    Ad = (A.t() if ta else A).double()
    Wd = (W if tb else W.t()).double()
    Nd = Ad if norm is None else norm.double()
    X = Ad * torch.rsqrt(Nd.pow(2).mean(-1, keepdim=True) + eps) if flags & 1 else Ad
    y = X @ Wd
    if bias is not None:
        y = y + bias.double()
    if flags & 2:
        y = torch.nn.functional.silu(y)
    if flags & 4:
        r = y.reshape(y.shape[0], -1, 2, 32)
        y = (r[:, :, 0] * torch.nn.functional.silu(r[:, :, 1])).reshape(y.shape[0], -1)
    if R_ is not None:
        y = y + R_.double()
    if C0 is not None:
        y = y + C0.double()
    return y


def rel_err2(got, want):
    """Largest rel_err over the (out, c2) pairs of two results (c2 may be None)."""
    return max(R.rel_err(g, w) for g, w in zip(got, want) if w is not None)
