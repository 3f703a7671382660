"""Shapes, inputs and oracle evaluations shared by tests/test_gpu_wide_frames.py (GPU) and tests/test_wide_frames_host.py (CPU): the space
and cross attention operators above 64 items per side (`wide=True`, csrc/attn_tiled.hip)."""
import functools

import torch

from oracle import restate

# (F, S, D, heads, dh, has_rv, num_special, clamp, belief)
SPACE_WIDE = [(2, 65, 64, 2, 64, True, 1, 50., True),          # the special token alone in the second tile
              (2, 100, 64, 3, 32, False, 6, 50., True),        # the special block straddles a 16-key boundary; no residual; three heads
              (1, 130, 128, 2, 64, True, 4, 50., True),        # the special block straddles the 128 boundary
              (1, 128, 64, 2, 16, True, 0, 3., False),         # exact tiles, no specials, tight clamp, no belief, dh 16
              (1, 96, 64, 2, 32, True, 40, 50., True),         # encoder-like: the special block spans the 64 boundary
              (1, 1024, 64, 1, 16, False, 1, 50., True)]       # the cap
# the shapes of test_gpu_backward.py::test_space_attention_* (<= 64 tokens: the LDS kernel's ground, here under the forcing hook)
SPACE_SHORT = [(5, 9, 64, 2, 64, True, 1, 50., True), (3, 30, 128, 3, 32, False, 6, 50., True), (4, 12, 64, 5, 16, True, 0, 2., False),
               (130, 15, 512, 8, 64, True, 1, 50., True), (3, 64, 64, 2, 64, True, 2, 50., True), (2, 41, 64, 2, 32, True, 1, 50., True)]
# (G, nq, nk, D, Dc, heads, dh, item_major, ctx_norm, clamp)
CROSS_WIDE = [(6, 1, 74, 64, 64, 2, 32, False, True, None),    # final special cross attention at 75 tokens per frame
              (3, 4, 256, 128, 8, 3, 16, False, True, 5.),     # learned-query pool over 256 latents
              (2, 130, 5, 64, 32, 2, 64, False, False, None),  # many queries, few keys, context not normalised
              (2, 65, 65, 64, 64, 2, 64, False, True, None),   # both sides just past one tile
              (5, 1, 70, 64, 64, 4, 64, True, True, None),     # item-major
              (1, 1, 1024, 64, 64, 1, 16, False, True, None)]  # the cap
# the shapes of test_gpu_backward.py::test_cross_attention_*
CROSS_SHORT = [(37, 1, 7, 64, 64, 4, 64, True, True, None), (6, 3, 20, 64, 64, 2, 32, False, True, None), (5, 4, 64, 128, 8, 3, 16, False, True, 5.),
               (9, 64, 5, 64, 32, 2, 64, False, False, None)]


@functools.lru_cache(maxsize=None)
def space_problem(F_, S, D, heads, dh, has_rv):
    from test_gpu_backward import _attn_params
    g = torch.Generator().manual_seed(7)
    W = _attn_params(D, heads, dh, g)
    x = torch.randn(F_, S, D, generator=g) * 1.5
    rv = torch.randn(F_, S, heads, dh, generator=g) if has_rv else None
    dy = torch.randn(F_, S, D, generator=g)
    return W, x, rv, dy


def space_oracle_run(shape, dtype=torch.float64, nudge=0.):
    F_, S, D, heads, dh, has_rv, ns, clamp, belief = shape
    W, x, rv, dy = space_problem(F_, S, D, heads, dh, has_rv)
    Wd = {k: (v.to(dtype) * (1. + nudge)).requires_grad_() for k, v in W.items()}
    xd = (x.to(dtype) * (1. + nudge)).requires_grad_()
    rvd = (rv.to(dtype) * (1. + nudge)).requires_grad_() if has_rv else None
    mask = restate.special_token_mask(S, ns) if ns > 0 else None
    ref, _ = restate.attention(Wd, '', xd, heads=heads, dim_head=dh, residual_values=rvd, softclamp_value=clamp, mask=mask, belief=belief)
    ref.backward(dy.to(dtype))
    out = {'y': ref.detach(), 'dx': xd.grad}
    if has_rv:
        out['d residual_values'] = rvd.grad
    out.update({'d ' + k: Wd[k].grad for k in W if has_rv or 'value_residual_mix' not in k})
    return out


@functools.lru_cache(maxsize=None)
def space_oracle(shape):
    """float64 reference of one shape: computed once, shared by every test of the shape, never written to."""
    return space_oracle_run(shape)


@functools.lru_cache(maxsize=None)
def cross_problem(G, nq, nk, D, Dc, heads, dh):
    g = torch.Generator().manual_seed(13)
    r = lambda *s_, k=1.: torch.randn(*s_, generator=g) * k
    hd = heads * dh
    W = {'norm.weight': 1. + r(D, k=.1), 'norm_context.weight': 1. + r(Dc, k=.1), 'to_q.weight': r(hd, D, k=3. * D ** -.5), 'to_k.weight': r(hd, Dc, k=Dc ** -.5),
         'to_v.weight': r(hd, Dc, k=Dc ** -.5), 'to_out.weight': r(D, hd, k=hd ** -.5), 'to_gates.0.weight': r(heads, D, k=D ** -.5),
         'k_heads_rmsnorm.gamma': r(heads, dh, k=.3)}
    return W, r(G, nq, D, k=1.5), r(G, nk, Dc, k=1.5), r(G, nq, D)


def cross_oracle_run(shape, dtype=torch.float64):
    G, nq, nk, D, Dc, heads, dh, item_major, ctx_norm, clamp = shape
    W, q, c, dy = cross_problem(G, nq, nk, D, Dc, heads, dh)
    Wd = {k: v.to(dtype).clone().requires_grad_() for k, v in W.items()}        # (clone: the cached problem stays as it is)
    qd, cd = q.to(dtype).clone().requires_grad_(), c.to(dtype).clone().requires_grad_()
    ref, _ = restate.attention(Wd, '', qd, heads=heads, dim_head=dh, context=cd, belief=True, has_ctx_norm=ctx_norm, softclamp_value=clamp)
    ref.backward(dy.to(dtype))
    out = {'y': ref.detach(), 'dq_tokens': qd.grad, 'dcontext': cd.grad}
    out.update({'d ' + k: Wd[k].grad for k in W if ctx_norm or k != 'norm_context.weight'})
    return out


@functools.lru_cache(maxsize=None)
def cross_oracle(shape):
    return cross_oracle_run(shape)
