"""Differentiable trunk blocks on the HIP kernels and the dynamics training forward composed from them.

`feedforward`, `space_attention`, `time_attention` and `cross_attention` are the reference FeedForward (dreamer4/dreamer4.py:2079-2116)
and Attention (dreamer4.py:1968-2075: within a frame, along time with rotary + causal mask, over a context) as
`torch.autograd.Function`s over the C-ABI operators `d4_ff_* / d4_space_attn_* / d4_time_attn_* / d4_cross_attn_*` (include/d4hip.h).
Parameters are passed in the reference's own layout (the tensors of its state_dict), gradients come back in the same layout.  BY DEFAULT the blocks
run as these plain `autograd.Function`s (less host dispatch time; not traceable by torch.compile); with D4_TRUNK_DISPATCHER=1 they go through
their dispatcher registrations `torch.ops.d4hip.{swiglu_ff, attn_block_space, attn_block_time, attn_block_cross}` (dreamer4_amd/ops.py: fake
implementations + registered autograd, same C-ABI operators, same results).  The bare RMSNorm + Linear pieces of the trunk always run on
`torch.ops.d4hip.{rmsnorm, linear}`.  By default a
block keeps the workspace its forward ran in and the backward (`*_backward_saved`) recomputes nothing; with D4_TRUNK_SAVE_FORWARD=0 the
backward recomputes the forward intermediates and nothing but the inputs is kept alive between the two passes.  `transformer` composes
the AxialSpaceTimeTransformer (dreamer4.py:2927-3267), `world_model_prediction` the dynamics model's `get_prediction`
(dreamer4.py:7156-7287), `dynamics_flow_losses` / `dynamics_agent_losses` the losses of the training forward (dreamer4.py:7335-7598), `tokenizer_latents` /
`tokenizer_losses` the VideoTokenizer's training forward (dreamer4.py:4239-4603) on the pixel-side operators of csrc/tok_train.hip.
fp32, HIP device only — there is no CPU fallback.  Not used by the imagination path."""
from __future__ import annotations

import ctypes as C

import torch

from dreamer4_amd import _lib
from dreamer4_amd import ops as _ops  # noqa: F401  (registers torch.ops.d4hip.*)


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _prep(*ts):
    out = []
    for t in ts:
        if t is None:
            out.append(None)
            continue
        if t.device.type != 'cuda':
            raise _lib.D4Error('trunk_ops run only on an MI355X (HIP) device: there is no CPU fallback')
        assert t.dtype == torch.float32, 'fp32 only'
        out.append(t.contiguous())
    return out


def save_forward_workspace():
    """D4_TRUNK_SAVE_FORWARD=0: the backward of every block recomputes its forward (nothing but the inputs is kept between the passes);
    default: each block keeps the workspace its forward ran in (normalised input, concatenated weight images, projections: 0.1-0.2 GB per
    block at 3840 token rows — 288 GB of HBM is what makes that the default) and the backward runs on it without recomputing anything."""
    import os
    return os.environ.get('D4_TRUNK_SAVE_FORWARD', '1') != '0'


def via_dispatcher():
    """D4_TRUNK_DISPATCHER=1: the blocks go through their `torch.ops.d4hip.*` registrations (dispatcher-visible, traceable by
    torch.compile); default: the same C entry points through plain `torch.autograd.Function`s — the dispatcher route costs ~9 % of a
    training step at cfg 2's architecture in host-side dispatch (20.9 vs 19.1 ms, same box), so eager training does not pay for it."""
    import os
    return os.environ.get('D4_TRUNK_DISPATCHER', '0') == '1'


ARITHS = ('fp32', 'bf16')
ATTN_PRODUCTS = ('fp32', 'bf16')


def arith_id(arith):
    """'fp32' -> 0, 'bf16' -> 1 (the `arith` argument of d4_train_arith_set); anything else is a ValueError."""
    if arith not in ARITHS:
        raise ValueError(f"training arithmetic must be one of {ARITHS}, got {arith!r}")
    return ARITHS.index(arith)


def products_id(attn_products):
    """'fp32' -> 0, 'bf16' -> 1 (the argument of d4_train_attn_products_set); anything else is a ValueError."""
    if attn_products not in ATTN_PRODUCTS:
        raise ValueError(f"attn_products must be one of {ATTN_PRODUCTS}, got {attn_products!r}")
    return ATTN_PRODUCTS.index(attn_products)


class _arith_mode:
    """The block arithmetic of libd4hip is process-wide: every forward / backward call of a block sets its own immediately before the C call
    (autograd runs the backward on another thread, and a saved workspace must meet the arithmetic it was written in) and puts the previous
    one back.  In bf16 mode the call also gets a scratch for its bf16 operand images (`scratch_bytes`), bound to this thread for the call and
    released with it: nothing of it is kept between the forward and the backward.
    `wide` (None: leave it alone) is the other process-wide switch, d4_train_wide_set, handled the same way for the same reason: the
    workspace size query, the forward and the backward of a space / cross block must all meet the setting the block was called with.
    `products` (None: leave it alone) is the third, d4_train_attn_products_set (the products of the tiled attention core: 0 fp32, 1 bf16,
    DESIGN.md 18), handled like `wide`: it changes the workspace size wherever the block takes the tiled core."""
    def __init__(self, lib, a, scratch_bytes=0, device=None, wide=None, products=None):
        self.lib, self.a, self.wide, self.products = lib, a, wide, products
        self.scratch = _workspace(scratch_bytes, device) if a else None

    def __enter__(self):
        self.prev = self.lib.d4_train_arith_set(self.a)
        if self.wide is not None:
            self.prev_wide = self.lib.d4_train_wide_set(self.wide)
        if self.products is not None:
            self.prev_products = self.lib.d4_train_attn_products_set(self.products)
        if self.scratch is not None:
            self.lib.d4_train_scratch_bind(self.scratch[1], self.scratch[0].numel() - 256)

    def __exit__(self, *exc):
        if self.scratch is not None:
            self.lib.d4_train_scratch_bind(None, 0)
        if self.products is not None:
            self.lib.d4_train_attn_products_set(self.prev_products)
        if self.wide is not None:
            self.lib.d4_train_wide_set(self.prev_wide)
        self.lib.d4_train_arith_set(self.prev)
        return False


def _no_dispatcher(arith, wide=False, attn_products='fp32'):
    if arith != 'fp32':
        arith_id(arith)
        raise NotImplementedError(f"D4_TRUNK_DISPATCHER=1 does not carry arith={arith!r}: the torch.ops.d4hip block registrations are fp32 only "
                                  "(run the bf16 training arithmetic on the default autograd.Function route)")
    if wide:
        raise NotImplementedError("D4_TRUNK_DISPATCHER=1 does not carry wide=True: the torch.ops.d4hip block registrations stop at 64 items per "
                                  "group (run wide frames on the default autograd.Function route)")
    if attn_products != 'fp32':
        products_id(attn_products)
        raise NotImplementedError(f"D4_TRUNK_DISPATCHER=1 does not carry attn_products={attn_products!r}: the torch.ops.d4hip block registrations "
                                  "run the attention cores' fp32 products only (use the default autograd.Function route)")


def _workspace(nbytes, device):
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    base = ws.data_ptr()
    return ws, C.c_void_p(base + (-base) % 256)


class _FeedForward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, norm_w, w_in, b_in, w_out, b_out, arith=0):
        x, norm_w, w_in, b_in, w_out, b_out = _prep(x, norm_w, w_in, b_in, w_out, b_out)
        D, inner = x.shape[-1], w_out.shape[1]
        assert w_in.shape == (2 * inner, D) and w_out.shape == (D, inner) and b_in.shape == (2 * inner,) and b_out.shape == (D,)
        rows = x.numel() // D
        lib = _lib.load()
        nbytes = lib.d4_ff_workspace_bytes(rows, D, inner)
        ws, wp = _workspace(nbytes, x.device)
        y = torch.empty_like(x)
        with _arith_mode(lib, arith, lib.d4_ff_bf16_scratch_bytes(rows, D, inner) if arith else 0, x.device):
            _lib.check(lib.d4_ff_forward(_lib.ptr(x), _lib.ptr(norm_w), _lib.ptr(w_in), _lib.ptr(b_in), _lib.ptr(w_out), _lib.ptr(b_out),
                                         rows, D, inner, _lib.ptr(y), wp, nbytes, _stream(x)))
        ctx.save_for_backward(x, norm_w, w_in, b_in, w_out)
        ctx.arith = arith
        ctx.fwd_ws = (ws, wp, nbytes) if save_forward_workspace() and any(ctx.needs_input_grad) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, norm_w, w_in, b_in, w_out = ctx.saved_tensors
        (dy,) = _prep(dy)
        D, inner = x.shape[-1], w_out.shape[1]
        rows = x.numel() // D
        lib = _lib.load()
        if ctx.fwd_ws is not None:
            (ws, wp, nbytes), fn = ctx.fwd_ws, lib.d4_ff_backward_saved
        else:
            nbytes = lib.d4_ff_workspace_bytes(rows, D, inner)
            (ws, wp), fn = _workspace(nbytes, x.device), lib.d4_ff_backward
        dx, dn, dwi, dbi, dwo = torch.empty_like(x), torch.empty_like(norm_w), torch.empty_like(w_in), torch.empty_like(b_in), torch.empty_like(w_out)
        dbo = torch.empty(D, device=x.device)
        with _arith_mode(lib, ctx.arith, lib.d4_ff_bf16_scratch_bytes(rows, D, inner) if ctx.arith else 0, x.device):
            _lib.check(fn(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(norm_w), _lib.ptr(w_in), _lib.ptr(b_in), _lib.ptr(w_out), rows, D, inner,
                          _lib.ptr(dx), _lib.ptr(dn), _lib.ptr(dwi), _lib.ptr(dbi), _lib.ptr(dwo), _lib.ptr(dbo), wp, nbytes, _stream(x)))
        return dx, dn, dwi, dbi, dwo, dbo, None


class _SpaceAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rv, norm_w, wq, wk, wv, wo, wg, wm, bm, gamma, softclamp, num_special, belief, arith=0, wide=0, products=0):
        x, rv, norm_w, wq, wk, wv, wo, wg, wm, bm, gamma = _prep(x, rv, norm_w, wq, wk, wv, wo, wg, wm, bm, gamma)
        assert x.ndim == 3, 'x must be (frames, tokens, dim)'
        F_, S, D = x.shape
        heads, dh = gamma.shape
        assert wq.shape == (heads * dh, D) and wo.shape == (D, heads * dh) and wg.shape == (heads, D)
        assert rv is None or rv.shape == (F_, S, heads, dh)
        lib = _lib.load()
        y = torch.empty_like(x)
        with _arith_mode(lib, arith, lib.d4_attn_bf16_scratch_bytes(F_ * S, D, heads, dh) if arith else 0, x.device, wide, products):
            nbytes = lib.d4_attn_workspace_bytes(F_, S, D, heads, dh)
            ws, wp = _workspace(nbytes, x.device)
            _lib.check(lib.d4_space_attn_forward(_lib.ptr(x), _lib.ptr(rv), _lib.ptr(norm_w), _lib.ptr(wq), _lib.ptr(wk), _lib.ptr(wv), _lib.ptr(wo),
                                                 _lib.ptr(wg), _lib.ptr(wm), _lib.ptr(bm), _lib.ptr(gamma), F_, S, D, heads, dh,
                                                 float(softclamp or 0.), int(num_special), int(bool(belief)), _lib.ptr(y), wp, nbytes, _stream(x)))
        ctx.arith, ctx.wide, ctx.products = arith, wide, products
        ctx.save_for_backward(x, rv, norm_w, wq, wk, wv, wo, wg, wm, bm, gamma)
        ctx.cfg = (float(softclamp or 0.), int(num_special), int(bool(belief)))
        ctx.fwd_ws = (ws, wp, nbytes) if save_forward_workspace() and any(ctx.needs_input_grad) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, rv, norm_w, wq, wk, wv, wo, wg, wm, bm, gamma = ctx.saved_tensors
        (dy,) = _prep(dy)
        F_, S, D = x.shape
        heads, dh = gamma.shape
        lib = _lib.load()
        e = torch.empty_like
        dx, dn, dq, dk, dv, do, dg, dgam = e(x), e(norm_w), e(wq), e(wk), e(wv), e(wo), e(wg), e(gamma)
        drv, dwm, dbm = (e(rv), e(wm), e(bm)) if rv is not None else (None, None, None)
        with _arith_mode(lib, ctx.arith, lib.d4_attn_bf16_scratch_bytes(F_ * S, D, heads, dh) if ctx.arith else 0, x.device, ctx.wide, ctx.products):
            if ctx.fwd_ws is not None:
                (ws, wp, nbytes), fn = ctx.fwd_ws, lib.d4_space_attn_backward_saved
            else:
                nbytes = lib.d4_attn_workspace_bytes(F_, S, D, heads, dh)
                (ws, wp), fn = _workspace(nbytes, x.device), lib.d4_space_attn_backward
            _lib.check(fn(
                _lib.ptr(x), _lib.ptr(rv), _lib.ptr(dy), _lib.ptr(norm_w), _lib.ptr(wq), _lib.ptr(wk), _lib.ptr(wv), _lib.ptr(wo), _lib.ptr(wg),
                _lib.ptr(wm), _lib.ptr(bm), _lib.ptr(gamma), F_, S, D, heads, dh, *ctx.cfg,
                _lib.ptr(dx), _lib.ptr(drv), _lib.ptr(dn), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(do), _lib.ptr(dg), _lib.ptr(dwm), _lib.ptr(dbm),
                _lib.ptr(dgam), wp, nbytes, _stream(x)))
        return dx, drv, dn, dq, dk, dv, do, dg, dwm, dbm, dgam, None, None, None, None, None, None


class _TimeAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rv, norm_w, wq, wk, wv, wo, wg, wm, bm, gamma, inv_freq, softclamp, belief, arith=0, products=0):
        x, rv, norm_w, wq, wk, wv, wo, wg, wm, bm, gamma, inv_freq = _prep(x, rv, norm_w, wq, wk, wv, wo, wg, wm, bm, gamma, inv_freq)
        assert x.ndim == 4, 'x must be (batch, frames, tokens, dim)'
        B, T, S, D = x.shape
        heads, dh = gamma.shape
        assert wq.shape == (heads * dh, D) and wo.shape == (D, heads * dh) and wg.shape == (heads, D) and inv_freq.shape == (dh // 2,)
        assert rv is None or rv.shape == (B, T, S, heads, dh)
        lib = _lib.load()
        y = torch.empty_like(x)
        with _arith_mode(lib, arith, lib.d4_attn_bf16_scratch_bytes(B * T * S, D, heads, dh) if arith else 0, x.device, None, products):
            nbytes = lib.d4_time_attn_workspace_bytes(B, T, S, D, heads, dh)
            ws, wp = _workspace(nbytes, x.device)
            _lib.check(lib.d4_time_attn_forward(_lib.ptr(x), _lib.ptr(rv), _lib.ptr(norm_w), _lib.ptr(wq), _lib.ptr(wk), _lib.ptr(wv), _lib.ptr(wo),
                                                _lib.ptr(wg), _lib.ptr(wm), _lib.ptr(bm), _lib.ptr(gamma), _lib.ptr(inv_freq), B, T, S, D, heads, dh,
                                                float(softclamp or 0.), int(bool(belief)), _lib.ptr(y), wp, nbytes, _stream(x)))
        ctx.arith, ctx.products = arith, products
        ctx.save_for_backward(x, rv, norm_w, wq, wk, wv, wo, wg, wm, bm, gamma, inv_freq)
        ctx.cfg = (float(softclamp or 0.), int(bool(belief)))
        ctx.fwd_ws = (ws, wp, nbytes) if save_forward_workspace() and any(ctx.needs_input_grad) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, rv, norm_w, wq, wk, wv, wo, wg, wm, bm, gamma, inv_freq = ctx.saved_tensors
        (dy,) = _prep(dy)
        B, T, S, D = x.shape
        heads, dh = gamma.shape
        lib = _lib.load()
        e = torch.empty_like
        dx, dn, dq, dk, dv, do, dg, dgam = e(x), e(norm_w), e(wq), e(wk), e(wv), e(wo), e(wg), e(gamma)
        drv, dwm, dbm = (e(rv), e(wm), e(bm)) if rv is not None else (None, None, None)
        with _arith_mode(lib, ctx.arith, lib.d4_attn_bf16_scratch_bytes(B * T * S, D, heads, dh) if ctx.arith else 0, x.device, None, ctx.products):
            if ctx.fwd_ws is not None:
                (ws, wp, nbytes), fn = ctx.fwd_ws, lib.d4_time_attn_backward_saved
            else:
                nbytes = lib.d4_time_attn_workspace_bytes(B, T, S, D, heads, dh)
                (ws, wp), fn = _workspace(nbytes, x.device), lib.d4_time_attn_backward
            _lib.check(fn(
                _lib.ptr(x), _lib.ptr(rv), _lib.ptr(dy), _lib.ptr(norm_w), _lib.ptr(wq), _lib.ptr(wk), _lib.ptr(wv), _lib.ptr(wo), _lib.ptr(wg),
                _lib.ptr(wm), _lib.ptr(bm), _lib.ptr(gamma), _lib.ptr(inv_freq), B, T, S, D, heads, dh, *ctx.cfg,
                _lib.ptr(dx), _lib.ptr(drv), _lib.ptr(dn), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(do), _lib.ptr(dg), _lib.ptr(dwm), _lib.ptr(dbm),
                _lib.ptr(dgam), wp, nbytes, _stream(x)))
        return dx, drv, dn, dq, dk, dv, do, dg, dwm, dbm, dgam, None, None, None, None, None


class _CrossAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx_, q_tokens, context, norm_w, norm_ctx_w, wq, wk, wv, wo, wg, gamma, item_major, softclamp, arith=0, wide=0, products=0):
        q_tokens, context, norm_w, norm_ctx_w, wq, wk, wv, wo, wg, gamma = _prep(q_tokens, context, norm_w, norm_ctx_w, wq, wk, wv, wo, wg, gamma)
        assert q_tokens.ndim == 3 and context.ndim == 3
        G, nq, D = q_tokens.shape
        nk, Dc = (context.shape[0], context.shape[2]) if item_major else (context.shape[1], context.shape[2])
        assert (context.shape[1] if item_major else context.shape[0]) == G, 'context groups do not match the queries'
        heads, dh = gamma.shape
        assert wq.shape == (heads * dh, D) and wk.shape == (heads * dh, Dc) and wv.shape == (heads * dh, Dc) and wo.shape == (D, heads * dh)
        lib = _lib.load()
        y = torch.empty_like(q_tokens)
        with _arith_mode(lib, arith, lib.d4_cross_attn_bf16_scratch_bytes(G, nq, nk, D, Dc, heads, dh) if arith else 0, q_tokens.device, wide, products):
            nbytes = lib.d4_cross_attn_workspace_bytes(G, nq, nk, D, Dc, heads, dh)
            ws, wp = _workspace(nbytes, q_tokens.device)
            _lib.check(lib.d4_cross_attn_forward(_lib.ptr(q_tokens), _lib.ptr(context), _lib.ptr(norm_w), _lib.ptr(norm_ctx_w), _lib.ptr(wq), _lib.ptr(wk),
                                                 _lib.ptr(wv), _lib.ptr(wo), _lib.ptr(wg), _lib.ptr(gamma), G, nq, nk, int(bool(item_major)), D, Dc, heads, dh,
                                                 float(softclamp or 0.), _lib.ptr(y), wp, nbytes, _stream(q_tokens)))
        ctx_.arith, ctx_.wide, ctx_.products = arith, wide, products
        ctx_.save_for_backward(q_tokens, context, norm_w, norm_ctx_w, wq, wk, wv, wo, wg, gamma)
        ctx_.cfg = (G, nq, nk, int(bool(item_major)), D, Dc, heads, dh, float(softclamp or 0.))
        ctx_.fwd_ws = (ws, wp, nbytes) if save_forward_workspace() and any(ctx_.needs_input_grad) else None
        return y

    @staticmethod
    def backward(ctx_, dy):
        q_tokens, context, norm_w, norm_ctx_w, wq, wk, wv, wo, wg, gamma = ctx_.saved_tensors
        (dy,) = _prep(dy)
        G, nq, nk, item_major, D, Dc, heads, dh, softclamp = ctx_.cfg
        lib = _lib.load()
        e = torch.empty_like
        dq_t, dc, dn, dq, dk, dv, do, dg, dgam = e(q_tokens), e(context), e(norm_w), e(wq), e(wk), e(wv), e(wo), e(wg), e(gamma)
        dnc = e(norm_ctx_w) if norm_ctx_w is not None else None
        with _arith_mode(lib, ctx_.arith, lib.d4_cross_attn_bf16_scratch_bytes(G, nq, nk, D, Dc, heads, dh) if ctx_.arith else 0, q_tokens.device, ctx_.wide, ctx_.products):
            if ctx_.fwd_ws is not None:
                (ws, wp, nbytes), fn = ctx_.fwd_ws, lib.d4_cross_attn_backward_saved
            else:
                nbytes = lib.d4_cross_attn_workspace_bytes(G, nq, nk, D, Dc, heads, dh)
                (ws, wp), fn = _workspace(nbytes, q_tokens.device), lib.d4_cross_attn_backward
            _lib.check(fn(
                _lib.ptr(q_tokens), _lib.ptr(context), _lib.ptr(dy), _lib.ptr(norm_w), _lib.ptr(norm_ctx_w), _lib.ptr(wq), _lib.ptr(wk), _lib.ptr(wv),
                _lib.ptr(wo), _lib.ptr(wg), _lib.ptr(gamma), G, nq, nk, item_major, D, Dc, heads, dh, softclamp,
                _lib.ptr(dq_t), _lib.ptr(dc), _lib.ptr(dn), _lib.ptr(dnc), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(do), _lib.ptr(dg), _lib.ptr(dgam),
                wp, nbytes, _stream(q_tokens)))
        return dq_t, dc, dn, dnc, dq, dk, dv, do, dg, dgam, None, None, None, None, None


def _dev(*ts):
    for t in ts:
        if t is not None and t.device.type != 'cuda':
            raise _lib.D4Error('trunk_ops run only on an MI355X (HIP) device: there is no CPU fallback')


def feedforward(x, norm_weight, proj_in_weight, proj_in_bias, proj_out_weight, proj_out_bias, *, arith='fp32'):
    """FeedForward.forward (dreamer4.py:2105-2116): proj_out(a * silu(g)), [a | g] = proj_in(RMSNorm(x)).  x (..., dim).
    With D4_TRUNK_DISPATCHER=1: torch.ops.d4hip.swiglu_ff (dreamer4_amd/ops.py: dispatcher-visible, autograd registered); default: the autograd.Function above."""
    _dev(x)
    if not via_dispatcher():
        return _FeedForward.apply(x, norm_weight, proj_in_weight, proj_in_bias, proj_out_weight, proj_out_bias, arith_id(arith))
    _no_dispatcher(arith)
    return torch.ops.d4hip.swiglu_ff(x, norm_weight, proj_in_weight, proj_in_bias, proj_out_weight, proj_out_bias)[0]


def space_attention(x, norm_weight, to_q, to_k, to_v, to_out, to_gates, k_gamma, *, residual_values=None, mix_weight=None, mix_bias=None,
                    softclamp_value=50., num_special=1, belief=True, arith='fp32', wide=False, attn_products='fp32'):
    """Attention.forward (dreamer4.py:1968-2075), self attention within each frame: x (frames, tokens, dim) -> (frames, tokens, dim).
    `residual_values` (frames, tokens, heads, dim_head) with `mix_weight` / `mix_bias` = to_learned_value_residual_mix.0 (every layer
    but the first); `num_special` trailing tokens are hidden from ordinary queries (dreamer4.py:1769-1783).  tokens <= 64; with `wide=True`
    <= 1024 (above 64 the tiled core of csrc/attn_tiled.hip; at <= 64 the same kernel and the same bits as without).
    `attn_products='bf16'`: where the block takes the tiled core, the core's products run on the bf16 matrix pipe.
    (D4_TRUNK_DISPATCHER=1: torch.ops.d4hip.attn_block_space, not with `wide` or bf16 products.)"""
    products_id(attn_products)
    _dev(x)
    assert x.ndim == 3, 'x must be (frames, tokens, dim)'
    if not via_dispatcher():
        return _SpaceAttention.apply(x, residual_values, norm_weight, to_q, to_k, to_v, to_out, to_gates, mix_weight, mix_bias, k_gamma,
                                     softclamp_value, num_special, belief, arith_id(arith), int(bool(wide)), products_id(attn_products))
    _no_dispatcher(arith, wide, attn_products)
    return torch.ops.d4hip.attn_block_space(x, residual_values, norm_weight, to_q, to_k, to_v, to_out, to_gates, mix_weight, mix_bias, k_gamma,
                                            float(softclamp_value or 0.), int(num_special), bool(belief))[0]


def time_attention(x, norm_weight, to_q, to_k, to_v, to_out, to_gates, k_gamma, inv_freq, *, residual_values=None, mix_weight=None,
                   mix_bias=None, softclamp_value=50., belief=True, arith='fp32', attn_products='fp32'):
    """The trunk's time layers (dreamer4.py:3176-3215): causal attention along time for every token column, rotary positions
    (`inv_freq` = time_rotary.inv_freq), no KV cache (the training form).  x (batch, frames, tokens, dim), frames <= 1024
    (above 64 frames the tiled core of csrc/attn_tiled.hip: workspace linear in the frames; with `attn_products='bf16'` its products run on
    the bf16 matrix pipe); `residual_values` (batch, frames, tokens, heads, dim_head).  (D4_TRUNK_DISPATCHER=1: torch.ops.d4hip.attn_block_time.)"""
    products_id(attn_products)
    _dev(x)
    assert x.ndim == 4, 'x must be (batch, frames, tokens, dim)'
    if not via_dispatcher():
        return _TimeAttention.apply(x, residual_values, norm_weight, to_q, to_k, to_v, to_out, to_gates, mix_weight, mix_bias, k_gamma, inv_freq,
                                    softclamp_value, belief, arith_id(arith), products_id(attn_products))
    _no_dispatcher(arith, False, attn_products)
    return torch.ops.d4hip.attn_block_time(x, residual_values, norm_weight, to_q, to_k, to_v, to_out, to_gates, mix_weight, mix_bias, k_gamma, inv_freq,
                                           float(softclamp_value or 0.), bool(belief))[0]


def cross_attention(q_tokens, context, norm_weight, norm_context_weight, to_q, to_k, to_v, to_out, to_gates, k_gamma, *,
                    context_item_major=False, softclamp_value=None, arith='fp32', wide=False, attn_products='fp32'):
    """Attention.forward with a context (dreamer4.py:1968-2075): q_tokens (groups, nq, dim); context (groups, nk, dim_ctx), or
    (nk, groups, dim_ctx) with `context_item_major` (the stack of layer hiddens of the AttentionPool).  nq, nk <= 64; with `wide=True`
    nq, nk <= 1024 (the tiled core of csrc/attn_tiled.hip as soon as either exceeds 64; otherwise the same kernel and bits).
    `attn_products='bf16'`: the tiled core's products on the bf16 matrix pipe.
    (D4_TRUNK_DISPATCHER=1: torch.ops.d4hip.attn_block_cross, not with `wide` or bf16 products.)"""
    products_id(attn_products)
    _dev(q_tokens)
    assert q_tokens.ndim == 3 and context.ndim == 3
    if not via_dispatcher():
        return _CrossAttention.apply(q_tokens, context, norm_weight, norm_context_weight, to_q, to_k, to_v, to_out, to_gates, k_gamma,
                                     context_item_major, softclamp_value, arith_id(arith), int(bool(wide)), products_id(attn_products))
    _no_dispatcher(arith, wide, attn_products)
    return torch.ops.d4hip.attn_block_cross(q_tokens, context, norm_weight, norm_context_weight, to_q, to_k, to_v, to_out, to_gates, k_gamma,
                                            bool(context_item_major), float(softclamp_value or 0.))[0]


def _norm_linear(x, norm_w, w, bias=None):
    """nn.Sequential(RMSNorm, Linear) of the reference on the HIP operators (torch.ops.d4hip.rmsnorm / linear, autograd registered)."""
    eps = torch.finfo(torch.float32).eps
    return torch.ops.d4hip.linear(torch.ops.d4hip.rmsnorm(x, norm_w, eps), w, bias, None, 0, 0.)


# ------------------------------------------------------------------------------------------------ the trunk, composed
def _attn_w(W, pre):
    return (W[pre + 'norm.weight'], W[pre + 'to_q.weight'], W[pre + 'to_k.weight'], W[pre + 'to_v.weight'], W[pre + 'to_out.weight'],
            W[pre + 'to_gates.0.weight'], W[pre + 'k_heads_rmsnorm.gamma'])


def _ff(W, pre, x, arith='fp32'):
    return feedforward(x, W[pre + 'norm.weight'], W[pre + 'proj_in.weight'], W[pre + 'proj_in.bias'], W[pre + 'proj_out.weight'], W[pre + 'proj_out.bias'],
                       arith=arith)


def _pool(W, pre, x, hiddens, arith='fp32', wide=False, attn_products='fp32'):
    """Residual(AttentionPool) (dreamer4.py:2143-2177 + 1869): one query per token over the stack of layer hiddens.
    hiddens: a list of layer hiddens, or the stack itself (L, rows, D) — `transformer` grows ONE stack by concatenation, so that in the
    backward every pool's context gradient meets the previous pools' as one (L, rows, D) sum instead of L per-hidden sums per pool."""
    shape = x.shape
    ctx = hiddens if torch.is_tensor(hiddens) else torch.stack([h.reshape(-1, shape[-1]) for h in hiddens], dim=0)     # (L, rows, D): item major
    p = pre + 'fn.attn.'
    nw, wq, wk, wv, wo, wg, gam = _attn_w(W, p)
    out = cross_attention(x.reshape(-1, 1, shape[-1]), ctx, nw, W[p + 'norm_context.weight'], wq, wk, wv, wo, wg, gam, context_item_major=True, arith=arith, wide=wide, attn_products=attn_products)
    return x + out.reshape(shape)


def transformer(W, tokens, *, is_time, softclamp_value=50., num_special=1, pre='transformer.', arith='fp32', wide=False, attn_products='fp32'):
    """AxialSpaceTimeTransformer.forward (dreamer4.py:2927-3267, defaults: value residual, attention pools, final special cross
    attention; final RMSNorm when the weights hold one) for training: no KV cache, every block a HIP forward + backward operator;
    only the residual adds, reshapes and the two bare RMSNorm + Linear pieces (value residual projection, final norm) are torch ops.
    W: the reference's trunk parameters by state_dict key (with the prefix `pre`); tokens (batch, frames, tokens, dim); is_time: per
    layer.  Differentiable with respect to tokens and every parameter.  `wide=True`: up to 1024 tokens per frame and pooled hiddens (space
    blocks, attention pools and the final special cross attention take `wide`).  `attn_products='bf16'`: every attention
    that takes the tiled core (time layers above 64 frames; with `wide`, the others above 64 items) runs its products on the bf16 pipe."""
    from torch.nn import functional as F
    products_id(attn_products)
    b, t, s, d = tokens.shape
    gamma0 = W[pre + 'layers.0.2.fn.k_heads_rmsnorm.gamma']
    h, dh = gamma0.shape
    eps = torch.finfo(torch.float32).eps
    vres = _norm_linear(tokens, W[pre + 'to_value_residual.0.weight'], W[pre + 'to_value_residual.1.weight'])
    vres = vres.reshape(b, t, s, h, dh)
    hiddens = tokens.reshape(1, -1, d)                    # the growing stack (L, rows, D) of layer hiddens
    depth = len(is_time)
    for i, tl in enumerate(is_time):
        ap = f'{pre}layers.{i}.2.fn.'
        nw, wq, wk, wv, wo, wg, gam = _attn_w(W, ap)
        mw, mb = W[ap + 'to_learned_value_residual_mix.0.weight'], W[ap + 'to_learned_value_residual_mix.0.bias']
        if tl:
            out = time_attention(tokens, nw, wq, wk, wv, wo, wg, gam, W[pre + 'time_rotary.inv_freq'], residual_values=vres, mix_weight=mw,
                                 mix_bias=mb, softclamp_value=softclamp_value, arith=arith, attn_products=attn_products)
        else:
            out = space_attention(tokens.reshape(b * t, s, d), nw, wq, wk, wv, wo, wg, gam, residual_values=vres.reshape(b * t, s, h, dh),
                                  mix_weight=mw, mix_bias=mb, softclamp_value=softclamp_value, num_special=num_special, arith=arith, wide=wide,
                                  attn_products=attn_products).reshape(b, t, s, d)
        tokens = tokens + out
        after_attn = tokens
        tokens = tokens + _ff(W, f'{pre}layers.{i}.3.fn.', tokens, arith)
        hiddens = torch.cat((hiddens, after_attn.reshape(1, -1, d), tokens.reshape(1, -1, d)), dim=0)
        if i != depth - 1:
            tokens = _pool(W, f'{pre}attn_pools.{i}.', tokens, hiddens, arith, wide, attn_products)
    # the special tokens cross-attend the ordinary tokens of their frame, then their own feedforward   dreamer4.py:3227-3238
    non_special, special = tokens[:, :, :-num_special], tokens[:, :, -num_special:]
    cp = pre + 'final_special_cross_attn.fn.'
    nw, wq, wk, wv, wo, wg, gam = _attn_w(W, cp)
    out = cross_attention(special.reshape(b * t, num_special, d), non_special.reshape(b * t, s - num_special, d), nw, W[cp + 'norm_context.weight'],
                          wq, wk, wv, wo, wg, gam, arith=arith, wide=wide, attn_products=attn_products)
    special = special + out.reshape(b, t, num_special, d)
    special = special + _ff(W, pre + 'final_special_ff.fn.', special, arith)
    tokens = torch.cat((non_special, special), dim=2)
    tokens = _pool(W, pre + 'final_attn_pool.', tokens, hiddens, arith, wide, attn_products)
    if pre + 'final_norm.weight' in W:
        tokens = torch.ops.d4hip.rmsnorm(tokens, W[pre + 'final_norm.weight'], eps)
    return tokens


# ------------------------------------------------------------------------------------------------ the dynamics model, training form
def _lq_pool(W, pre, x, arith='fp32', wide=False, attn_products='fp32'):
    """LearnedQueriesAttentionPool (dreamer4.py:2179-2210): x (..., n, d_ctx) -> (..., num_queries, dim)."""
    lead = x.shape[:-2]
    ctx = x.reshape(-1, *x.shape[-2:])
    queries = W[pre + 'queries']
    q = queries[None].expand(ctx.shape[0], -1, -1)
    p = pre + 'attn.'
    nw, wq, wk, wv, wo, wg, gam = _attn_w(W, p)
    out = cross_attention(q, ctx, nw, W[p + 'norm_context.weight'], wq, wk, wv, wo, wg, gam, arith=arith, wide=wide, attn_products=attn_products)
    return out.reshape(*lead, *out.shape[-2:])


def world_model_prediction(W, noised_latents, signal_levels, step_sizes_log2, *, is_time, num_spatial_tokens, num_register_tokens,
                           num_discrete_actions=(), discrete_actions=None, continuous_actions=None, tasks=None, softclamp_value=50., arith='fp32',
                           wide=False, attn_products='fp32'):
    """DynamicsWorldModel's `get_prediction` (dreamer4.py:7156-7287) for training: noised latents (b, t, n, dl), signal_levels (b, t),
    step_sizes_log2 (b,) -> (latent prediction (b, t, n, dl), agent embedding (b, t, dim)).  Token packing, embeddings and the bare
    RMSNorm + Linear of the latent head are torch ops; the trunk and the learned-query pools are the HIP forward + backward blocks.
    W: the model's parameters by reference state_dict key.  Actions are the ones paired with each frame's NEXT transition
    (`shift_action_tokens=True`): (b, t, na) or (b, t-1, na); frame 0 gets a zero action token."""
    from torch.nn import functional as F
    b, t, n, dl = noised_latents.shape
    d = W['signal_levels_embed.weight'].shape[1] * 2
    eps = torch.finfo(torch.float32).eps
    dev = noised_latents.device
    has_actions = 'action_learned_embed' in W and (len(num_discrete_actions) > 0 or W.get('action_embedder.continuous_action_embed.weight', torch.empty(0)).numel() > 0)
    if num_spatial_tokens == n:
        space = torch.ops.d4hip.linear(noised_latents, W['latents_to_spatial_tokens.weight'], W['latents_to_spatial_tokens.bias'], None, 0, 0.)
    else:
        space = _lq_pool(W, 'latents_to_spatial_tokens.', noised_latents, arith, wide, attn_products)
    sig = W['signal_levels_embed.weight'][signal_levels]
    stp = W['step_size_embed.weight'][step_sizes_log2][:, None].expand(b, t, -1)
    flow_tok = torch.cat((sig, stp), dim=-1)[:, :, None]
    regs = W['register_tokens'].expand(b, t, -1, -1) if num_register_tokens > 0 else noised_latents.new_zeros(b, t, 0, d)
    agent = W['agent_learned_embed'].expand(b, -1, -1)
    if tasks is not None:
        agent = agent + W['task_embed.weight'][tasks][:, None]
    agent = agent[:, None].expand(b, t, -1, -1)
    parts = [flow_tok, space, regs]
    if has_actions:
        emb = None
        if discrete_actions is not None and discrete_actions.shape[1] > 0:
            offs = _action_offsets(tuple(num_discrete_actions), dev)
            emb = W['action_embedder.discrete_action_embed.weight'][discrete_actions + offs].sum(dim=-2)
        if continuous_actions is not None and continuous_actions.shape[1] > 0:
            c = (W['action_embedder.continuous_action_embed.weight'] * continuous_actions[..., None]).sum(dim=-2)
            emb = c if emb is None else emb + c
        if emb is None:
            act = noised_latents.new_zeros(b, t, d)
        else:
            emb = emb + W['action_learned_embed']
            if emb.shape[1] == t:
                emb = emb[:, :-1]
            act = F.pad(emb, (0, 0, 1, 0), value=0.)
        parts.append(act[:, :, None])
    parts.append(agent)
    tokens = transformer(W, torch.cat(parts, dim=2), is_time=is_time, softclamp_value=softclamp_value, arith=arith, wide=wide,
                         attn_products=attn_products)
    space_out, agent_embed = tokens[:, :, 1:1 + num_spatial_tokens], tokens[:, :, -1]
    x = torch.ops.d4hip.rmsnorm(space_out, W['to_latent_pred.0.weight'], eps)
    if num_spatial_tokens != n:
        x = _lq_pool(W, 'to_latent_pred.1.', x, arith, wide, attn_products)
    return torch.ops.d4hip.linear(x, W['to_latent_pred.2.weight'], None, None, 0, 0.), agent_embed


_OFFSETS = {}


def _action_offsets(sizes, dev):
    """First embedding row of each discrete action type; kept per (sizes, device) so that a step uploads nothing (and can be captured)."""
    key = (sizes, str(dev))
    if key not in _OFFSETS:
        acc, offs = 0, []
        for n in sizes:
            offs.append(acc); acc += n
        _OFFSETS[key] = torch.tensor(offs, device=dev)
    return _OFFSETS[key]


def dynamics_flow_losses(W, latents, noise, signal_levels, step_sizes_log2, shortcut_train, *, max_steps, return_agent_embed=False, lens=None, **model):
    """The flow and shortcut-consistency losses of the dynamics training forward (dreamer4.py:6990-7003, 7335-7431; x-space prediction,
    ramp loss weight, no proprio / variable lengths / loss normalisers: the reference defaults).  `model`: the keyword arguments of
    `world_model_prediction` (among them `arith='fp32' | 'bf16'`, the arithmetic of the blocks' Linears in all three predictions, and `wide=True`
    for more than 64 tokens per frame, latents or pooled hiddens, and `attn_products='fp32' | 'bf16'`, the products of the tiled attention core).  Returns (flow_loss, shortcut_loss[, agent_embed of the main prediction]); backward runs through the HIP blocks."""
    from torch.nn import functional as F
    times = signal_levels.float() / max_steps
    tt = times[:, :, None, None]
    noised = noise.lerp(latents, tt)
    pred, agent_embed = world_model_prediction(W, noised, signal_levels, step_sizes_log2, **model)
    flow_losses = F.mse_loss(pred, latents, reduction='none') * (0.9 * times + 0.1)[:, :, None, None]
    if lens is not None:                                  # variable lengths: frames past a trajectory's length leave the means (dreamer4.py:7418-7426)
        lm = torch.arange(latents.shape[1], device=latents.device)[None, :] < lens[:, None]
        sel = lambda x: x[lm]
    else:
        sel = lambda x: x
    if not shortcut_train:
        fl = sel(flow_losses).mean()
        return (fl, latents.new_zeros(()), agent_embed) if return_agent_embed else (fl, latents.new_zeros(()))
    with torch.no_grad():
        half_log2 = step_sizes_log2 - 1
        half = 2 ** half_log2
        first, _ = world_model_prediction(W, noised, signal_levels, half_log2, **model)
        first_flow = (first - noised) / (1. - tt)
        denoised = noised + first_flow * (half[:, None, None, None] / max_steps)
        sig2 = signal_levels + half[:, None]
        second, _ = world_model_prediction(W, denoised, sig2, half_log2, **model)
        second_flow = (second - denoised) / (1. - (sig2.float() / max_steps)[:, :, None, None])
        target = (first_flow + second_flow) / 2
    shortcut_pred = (pred - noised) / (1. - tt)
    shortcut_losses = F.mse_loss(shortcut_pred, target, reduction='none') * (1. - tt) ** 2
    fl, sh = sel(flow_losses).mean(), sel(shortcut_losses).mean()
    return (fl, sh, agent_embed) if return_agent_embed else (fl, sh)


# ------------------------------------------------------------------------------------------------ the video tokenizer, training form
def _lin(x, w, b=None):
    return torch.ops.d4hip.linear(x, w, b, None, 0, 0.)


# The pixel-side operators (csrc/tok_train.hip) on the route the blocks take: plain autograd.Functions over the implementations of dreamer4_amd/ops.py
# by default, their `torch.ops.d4hip.*` registrations with D4_TRUNK_DISPATCHER=1 (same C entry points, same results).
class _LayerNormNoBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        ctx.save_for_backward(x, weight)
        ctx.eps = eps
        return _ops.layernorm_nobias_impl(x, weight, eps)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx, dw = _ops.layernorm_nobias_backward_impl(x, dy, weight, ctx.eps)
        return dx, dw, None


class _MaskRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tokens, mask, token):
        ctx.save_for_backward(mask)
        return _ops.mask_rows_impl(tokens, mask, token)

    @staticmethod
    def backward(ctx, dy):
        dx, dtok = _ops.mask_rows_backward_impl(dy, ctx.saved_tensors[0])
        return dx, None, dtok


class _ReconLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, recon_rows, video, noise, times, patch_size, v_space):
        loss, d_rows = _ops.recon_loss_impl(recon_rows, video, noise, times, patch_size, v_space)
        ctx.save_for_backward(d_rows)
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        return ctx.saved_tensors[0] * d_loss, None, None, None, None, None


def video_to_patches(video, patch_size):
    """'b c t (h p1) (w p2) -> b t h w (p1 p2 c)' (dreamer4.py:3838-3844, 3896); data, no gradient."""
    return torch.ops.d4hip.video_to_patches(video, patch_size) if via_dispatcher() else _ops.video_to_patches_impl(video, patch_size)


def flow_noised_patches(video, noise, times, patch_size):
    """Patch rows of noise.lerp(video, times[b]) in one pass (dreamer4.py:4457 + 3896); data, no gradient."""
    return torch.ops.d4hip.flow_noised_patches(video, noise, times, patch_size) if via_dispatcher() else _ops.flow_noised_patches_impl(video, noise, times, patch_size)


def layernorm_nobias(x, weight, eps=1e-5):
    """nn.LayerNorm(dim, bias=False) (dreamer4.py:114), differentiable in x and weight."""
    return torch.ops.d4hip.layernorm_nobias(x, weight, eps) if via_dispatcher() else _LayerNormNoBias.apply(x, weight, eps)


def mask_rows(tokens, mask, token):
    """Rows of `tokens` whose `mask` entry is set replaced by `token` (dreamer4.py:4344), differentiable in tokens and token."""
    return torch.ops.d4hip.mask_rows(tokens, mask, token) if via_dispatcher() else _MaskRows.apply(tokens, mask, token)


def recon_loss(recon_rows, video, noise, times, patch_size, v_space=True):
    """The reconstruction loss on the decoder's patch rows (dreamer4.py:4469-4474, 4516), differentiable in recon_rows."""
    if via_dispatcher():
        return torch.ops.d4hip.recon_loss(recon_rows, video, noise, times, patch_size, bool(v_space))[0]
    return _ReconLoss.apply(recon_rows, video, noise, times, patch_size, bool(v_space))


class _LossWithGrad(torch.autograd.Function):
    """An operator that returns (loss, d loss / d x) for a unit upstream gradient: the gradient is saved and scaled by the incoming one."""
    @staticmethod
    def forward(ctx, x, impl, *args):
        loss, dx = impl(x, *args)
        ctx.save_for_backward(dx)
        ctx.n_args = len(args)
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        return (ctx.saved_tensors[0] * d_loss, None) + (None,) * ctx.n_args


def sigreg(x, projs, domain=_ops.SIGREG_DOMAIN, num_knots=_ops.SIGREG_KNOTS):
    """sigreg(x) without a mask (dreamer4.py:728-767) on x (k, ..., d) with the raw normal draw `projs` (num_slices, d), differentiable in x."""
    lo, hi = float(domain[0]), float(domain[1])
    if via_dispatcher():
        return torch.ops.d4hip.sigreg(x, projs, lo, hi, int(num_knots))[0]
    return _LossWithGrad.apply(x, _ops.sigreg_impl, projs, lo, hi, int(num_knots))


def latent_ortho(x):
    """orthogonal_loss(x) (dreamer4.py:389-402) on x (..., n, d), differentiable in x."""
    return torch.ops.d4hip.latent_ortho(x)[0] if via_dispatcher() else _LossWithGrad.apply(x, _ops.latent_ortho_impl)


def _decoder_pos_embedding(W, nh, nw, n_layers, recipe, dev):
    """to_decoder_pos_emb on the linspace(-1, 1) grid of patch coordinates (dreamer4.py:3617-3625): (nh * nw, dim).  Parameter-sized work: the
    2-wide input of the first layer is normalised elementwise and zero-padded to the 4-float granularity of the HIP Linear."""
    from torch.nn import functional as F
    eps = torch.finfo(torch.float32).eps
    pre = 'decoder.to_decoder_pos_emb.'
    gy, gx = torch.meshgrid(torch.linspace(-1., 1., nh, device=dev), torch.linspace(-1., 1., nw, device=dev), indexing='ij')
    x = torch.stack((gy, gx), dim=-1).reshape(nh * nw, 2)
    pad_lin = lambda t, w, b: _lin(F.pad(t, (0, 2)), F.pad(w, (0, 2)), b)
    for i in range(n_layers):
        last, lin = i == n_layers - 1, (pad_lin if i == 0 else _lin)
        if recipe == 'pre_rms':
            nw_ = W[f'{pre}layers.{i}.0.weight']
            x = x * torch.rsqrt(x.square().mean(dim=-1, keepdim=True) + eps) * nw_ if i == 0 else torch.ops.d4hip.rmsnorm(x, nw_, eps)
            x = lin(x, W[f'{pre}layers.{i}.1.weight'], W[f'{pre}layers.{i}.1.bias'])
            if not last:
                x = F.silu(x)
        elif last:
            x = lin(x, W[f'{pre}layers.{i}.weight'], W[f'{pre}layers.{i}.bias'])
        else:
            x = lin(x, W[f'{pre}layers.{i}.0.weight'], W[f'{pre}layers.{i}.0.bias'])
            x = F.silu(F.layer_norm(x, x.shape[-1:], W[f'{pre}layers.{i}.1.weight'], W[f'{pre}layers.{i}.1.bias'], 1e-5))
    return x


def tokenizer_latents(W, video, *, patch_size, num_latent_tokens, encoder_is_time, patch_mask=None, wide=False, rows=None, return_pre_tanh=False):
    """The encoder half of VideoTokenizer.forward (dreamer4.py:4309-4425) for training: video (b, c, t, H, W) -> latents (b, t, n, dim_latent) in
    (-1, 1), differentiable in every encoder parameter.  `patch_mask` (b, t, nh, nw) bool: those patch tokens are replaced by `mask_token`.
    `rows` (b, t, nh, nw, p1 p2 c), with `video` None: the patch rows themselves, which may carry a gradient (the consistency pass feeds the decoder's
    rows: the patch permutation of their un-patchified video gives them back bit for bit).  `return_pre_tanh`: (latents, encoded_to_latents' output
    before the tanh), what the SIGReg term reads (dreamer4.py:4416-4425)."""
    if rows is None:
        rows = video_to_patches(video, patch_size)
    b, t = rows.shape[:2]
    x = layernorm_nobias(_lin(rows, W['patch_to_tokens.1.weight'], W['patch_to_tokens.1.bias']), W['patch_to_tokens.2.weight'], 1e-5)
    if patch_mask is not None:
        x = mask_rows(x, patch_mask, W['mask_token'])
    d = x.shape[-1]
    tokens = torch.cat((x.reshape(b, t, -1, d), W['latent_tokens'].expand(b, t, -1, -1)), dim=2)                 # [patches | latents]  dreamer4.py:4375
    tokens = transformer(W, tokens, is_time=encoder_is_time, num_special=num_latent_tokens, pre='encoder_transformer.', wide=wide)
    pre = _lin(tokens[:, :, -num_latent_tokens:], W['encoded_to_latents.weight'])
    return (pre.tanh(), pre) if return_pre_tanh else pre.tanh()


# the encoder's parameters by state_dict key prefix (what the encoder engine binds); with the training-only mask token, encoder_parameters() of dreamer4.py:4060-4067
ENCODER_KEYS = ('latent_tokens', 'patch_to_tokens.', 'encoder_transformer.', 'encoded_to_latents.')


def tokenizer_losses(W, video, *, draws, patch_size, num_latent_tokens, encoder_is_time, decoder_is_time, decoder_flow_steps, decoder_pos_mlp_depth,
                     head_mlp_recipe='pre_rms', v_space=True, wide=False, return_recon_video=False, sigreg_kwargs=None, ortho=False, consistency=False):
    """The losses of VideoTokenizer.forward (dreamer4.py:4309-4542: flow decoder, no LPIPS) with backward through both trunks.  W: the tokenizer's
    parameters by reference state_dict key; video (b, c, t, H, W); draws = dict(patch_mask (b, t, nh, nw) bool or None, time_indices (b,) in
    [0, decoder_flow_steps), noise like the video; with `sigreg_kwargs`, sigreg_projs (num_slices, dim_latent), the raw normal draw).  The passes over
    pixels are the operators of csrc/tok_train.hip: patch rows of the video and of noise.lerp(video, t), the LayerNorm of both patch embeddings, the mask
    rows, and the fused loss, which reads the video through the patch permutation (nothing is un-patchified).
    The latent regularisers, each only when asked for (none of them: the launches of the reconstruction loss alone):
      sigreg_kwargs = dict(domain=, num_knots=)   sigreg of encoded_to_latents' output before the tanh, per clip over (frames, latents)   dreamer4.py:4416-4423
      ortho                                       orthogonal_loss of the tanh'ed latents of every frame                                  dreamer4.py:4541
      consistency                                 mse(encoder(decoder output), latents.detach()) with the encoder's parameters frozen: a second encoder pass
                                                  on the decoder's patch rows under the same patch mask                               dreamer4.py:4493-4507
    Returns (recon_loss, latents, recon_video or None, dict(sigreg=, ortho=, consistency=) with None for a term that was not asked for)."""
    b, c, t, H, Wd = video.shape
    nh, nw = H // patch_size, Wd // patch_size
    enc = dict(patch_size=patch_size, num_latent_tokens=num_latent_tokens, encoder_is_time=encoder_is_time, patch_mask=draws.get('patch_mask'), wide=wide)
    regs = dict(sigreg=None, ortho=None, consistency=None)
    if sigreg_kwargs is not None:
        latents, pre = tokenizer_latents(W, video, return_pre_tanh=True, **enc)
        regs['sigreg'] = sigreg(pre, draws['sigreg_projs'], **sigreg_kwargs)
    else:
        latents = tokenizer_latents(W, video, **enc)
    time_indices, noise = draws['time_indices'], draws['noise']
    times = time_indices.float() / decoder_flow_steps
    lat = _lin(latents, W['latents_to_decoder.weight']) + W['time_embed.weight'][time_indices][:, None, None]      # dreamer4.py:4151-4157
    rows = flow_noised_patches(video, noise, times, patch_size)
    img = layernorm_nobias(_lin(rows, W['noised_patch_to_tokens.1.weight'], W['noised_patch_to_tokens.1.bias']),
                                           W['noised_patch_to_tokens.2.weight'], 1e-5)
    pos = _decoder_pos_embedding(W, nh, nw, decoder_pos_mlp_depth + 2, head_mlp_recipe, video.device)
    d = img.shape[-1]
    tokens = torch.cat((img.reshape(b, t, nh * nw, d) + pos, lat), dim=2)                                         # [patches | latents]  dreamer4.py:3654
    tokens = transformer(W, tokens, is_time=decoder_is_time, num_special=1, pre='decoder.transformer.', wide=wide)
    recon_rows = _lin(tokens[:, :, :nh * nw], W['decoder.tokens_to_patch.0.weight'], W['decoder.tokens_to_patch.0.bias']).reshape(b, t, nh, nw, -1)
    loss = recon_loss(recon_rows, video, noise, times, patch_size, v_space)
    if consistency:
        frozen = {k: (v.detach() if k.startswith(ENCODER_KEYS + ('mask_token',)) else v) for k, v in W.items()}
        regs['consistency'] = (tokenizer_latents(frozen, None, rows=recon_rows, **enc) - latents.detach()).square().mean()
    if ortho:
        regs['ortho'] = latent_ortho(latents)
    recon_video = _ops.patches_to_video_impl(recon_rows.detach(), c, patch_size) if return_recon_video else None
    return loss, latents, recon_video, regs


# ------------------------------------------------------------------------------------------------ agent-token losses of the training forward
def _head_mlp(W, pre, x, n_layers, recipe):
    """The heads' normed MLP (x_mlps_pytorch.create_mlp stand-in): 'pre_rms' or 'post_layer'.  Linear and RMSNorm are the
    differentiable HIP operators (torch.ops.d4hip.linear / rmsnorm: d4_gemm, d4_gemm_tn, d4_rmsnorm_backward) — no vendor BLAS on the path."""
    from torch.nn import functional as F
    eps = torch.finfo(torch.float32).eps
    lin = lambda t, w, b: torch.ops.d4hip.linear(t, w, b, None, 0, 0.)
    for i in range(n_layers):
        last = i == n_layers - 1
        if recipe == 'pre_rms':
            x = lin(torch.ops.d4hip.rmsnorm(x, W[f'{pre}layers.{i}.0.weight'], eps), W[f'{pre}layers.{i}.1.weight'], W[f'{pre}layers.{i}.1.bias'])
            if not last:
                x = F.silu(x)
        elif last:
            x = lin(x, W[f'{pre}layers.{i}.weight'], W[f'{pre}layers.{i}.bias'])
        else:
            x = lin(x, W[f'{pre}layers.{i}.0.weight'], W[f'{pre}layers.{i}.0.bias'])
            x = F.silu(F.layer_norm(x, x.shape[-1:], W[f'{pre}layers.{i}.1.weight'], W[f'{pre}layers.{i}.1.bias'], 1e-5))
    return x


def _mtp_targets(t, steps):
    """create_multi_token_prediction_targets (dreamer4.py:530-552)."""
    n = t.shape[1]
    idx = torch.arange(n, device=t.device)[:, None] + torch.arange(steps, device=t.device)[None, :]
    mask = idx < n
    idx = idx.masked_fill(~mask, 0)
    return t[:, idx], mask[None].expand(t.shape[0], -1, -1)


def hl_gauss_probs(values, vrange, num_bins, sigma_to_bin_ratio=2., eps=1e-10):
    """HL-Gauss soft targets (Farebrother et al. 2024; hl_gauss_pytorch stand-in)."""
    support = torch.linspace(vrange[0], vrange[1], num_bins + 1, device=values.device)
    sigma = sigma_to_bin_ratio * (vrange[1] - vrange[0]) / num_bins
    cdf = torch.special.erf((support - values.clamp(vrange[0], vrange[1])[..., None]) / (2. ** 0.5 * sigma))
    z = cdf[..., -1] - cdf[..., 0]
    return (cdf[..., 1:] - cdf[..., :-1]) / z.clamp(min=eps)[..., None]


def dynamics_agent_losses(W, agent_embed, latents, *, multi_token_pred_len, num_discrete_actions, reward_range, reward_num_bins,
                          policy_head_mlp_depth, terminal_mlp_depth, head_mlp_recipe='pre_rms', continuous_beta_param='softplus_p1', gae_discount_factor=0.997,
                          hl_sigma_ratio=2., hl_eps=1e-10, rewards=None, discrete_actions=None, terminals=None, lens=None,
                          continuous_actions=None):
    """The agent-token losses of the training forward (dreamer4.py:7432-7598): multi-token-prediction reward cross entropy against HL-Gauss
    soft targets, terminal BCE with label smoothing, behaviour-cloning log-likelihood of the discrete actions (multi-token prediction,
    `shift_action_tokens=True`).  Every Linear / RMSNorm runs on the differentiable HIP operators (torch.ops.d4hip.linear / rmsnorm: no vendor
    BLAS); the loss algebra on their outputs (log-softmax, masks, means) is elementwise torch on the device; gradients reach the
    trunk through `agent_embed`.  Returns a dict of the terms that were asked for: rewards (mtp,), terminals (), discrete_actions (mtp,), continuous_actions (mtp,)."""
    from torch.nn import functional as F
    out = {}
    mtp = multi_token_pred_len
    eps = torch.finfo(torch.float32).eps
    t = agent_embed.shape[1]
    lm = (torch.arange(t, device=agent_embed.device)[None, :] < lens[:, None]) if lens is not None else None     # dreamer4.py:7418-7423
    if rewards is not None:
        two_hot = hl_gauss_probs(rewards, reward_range, reward_num_bins, hl_sigma_ratio, hl_eps)
        x = agent_embed[:, :-1]
        # the ensemble of mtp [RMSNorm -> Linear] members as ONE HIP GEMM: the members' norm gains are folded into their weights (as the engine
        # does at prepare), so a single unit-gain normalisation of the rows feeds a [mtp * bins][D] weight            dreamer4.py:7440-7450
        g_, w_ = W['to_reward_pred.params.0'], W['to_reward_pred.params.1']                                    # [mtp][D], [mtp][bins][D]
        xhat = torch.ops.d4hip.rmsnorm(x.contiguous(), torch.ones_like(g_[0]), eps)
        pred = torch.ops.d4hip.linear(xhat, (w_ * g_[:, None, :]).reshape(-1, w_.shape[-1]), None, None, 0, 0.).unflatten(-1, (mtp, w_.shape[1]))
        tgt, mask = _mtp_targets(two_hot[:, 1:], mtp)
        losses = -(tgt * pred.log_softmax(dim=-1)).sum(dim=-1).masked_fill(~mask, 0.)
        out['rewards'] = losses[lm[:, :-1]].mean(dim=0) if lm is not None else losses.mean(dim=(0, 1))
    if terminals is not None:
        pooled = latents[:, 1:].mean(dim=-2)
        logit = _head_mlp(W, 'to_state_terminal_pred.0.', pooled, terminal_mlp_depth + 2, head_mlp_recipe).squeeze(-1)
        e = 1. - gae_discount_factor
        tl = F.binary_cross_entropy_with_logits(logit, terminals[:, 1:].float().clamp(min=e, max=1. - e), reduction='none')
        out['terminals'] = tl[lm[:, :-1]].mean() if lm is not None else tl.mean()
    if (discrete_actions is not None or continuous_actions is not None) and t > 1:
        pe = _head_mlp(W, 'policy_head.', agent_embed, policy_head_mlp_depth + 2, head_mlp_recipe)
    if continuous_actions is not None and t > 1:
        # Beta log-likelihood (dreamer4.py:7566-7597); alpha = link(raw0) + 1, beta = link(raw1) + 1 with the link named by
        # `continuous_beta_param` (world_model.BETA_PARAMS: the stand-in's softplus, or exp)
        padded = F.pad(continuous_actions, (0, 0, 1, 0), value=0.)
        tgt, mask = _mtp_targets(padded, mtp)
        tgt, mask = tgt[:, 1:].clamp(1e-5, 1. - 1e-5), mask[:, 1:]
        wc = W['action_embedder.continuous_action_unembed']                                                    # [nc][mtp][4 D][2]
        nc_ = wc.shape[0]
        # every member's (alpha, beta) rows in one HIP GEMM: weight [mtp][nc][2][4 D], member-major
        params = torch.ops.d4hip.linear(pe, wc.permute(1, 0, 3, 2).reshape(-1, wc.shape[2]), None, None, 0, 0.).unflatten(-1, (mtp, nc_, 2))       # (b, t, mtp, nc, 2)
        link = torch.exp if continuous_beta_param == 'exp_p1' else F.softplus
        a, b_ = link(params[..., 0]) + 1., link(params[..., 1]) + 1.
        lp = (a - 1.) * torch.log(tgt) + (b_ - 1.) * torch.log1p(-tgt) + torch.lgamma(a + b_) - torch.lgamma(a) - torch.lgamma(b_)
        nl = (-lp).masked_fill(~mask[..., None], 0.)                                                            # (b, t, mtp, nc)
        out['continuous_actions'] = nl[lm].mean(dim=(0, 2)) if lm is not None else nl.mean(dim=(0, 1, 3))
    if discrete_actions is not None and t > 1:
        padded = F.pad(discrete_actions, (0, 0, 1, 0), value=-1)
        tgt, mask = _mtp_targets(padded, mtp)
        tgt, mask = tgt[:, 1:].clamp(min=0), mask[:, 1:]
        # all mtp members in ONE HIP GEMM ([mtp * A][4 D] weight, member-major) and one pass of the loss algebra over (b, t, member): the per-member
        # python loop was ~10 tiny launches per member and action type                                              dreamer4.py:7520-7560
        un = W['action_embedder.discrete_action_unembed']                                                           # [A][mtp][4 D]
        logits = torch.ops.d4hip.linear(pe, un.transpose(0, 1).reshape(-1, un.shape[-1]), None, None, 0, 0.).unflatten(-1, (mtp, un.shape[0]))   # (b, t, mtp, A)
        lps, o = [], 0
        for a, n in enumerate(num_discrete_actions):
            lp = logits[..., o:o + n].log_softmax(dim=-1)
            lps.append(lp.gather(-1, tgt[..., a:a + 1]).squeeze(-1))
            o += n
        nl = (-torch.stack(lps, dim=-1)).masked_fill(~mask[..., None], 0.)                                          # (b, t, mtp, na)
        out['discrete_actions'] = nl[lm].mean(dim=(0, 2)) if lm is not None else nl.mean(dim=(0, 1, 3))
    return out
