"""GPU: wide frames in the training path (`wide=True`, `DynamicsWorldModel(train_wide_frames=True)`) — the within-frame and
cross geometries of the tiled attention core (csrc/attn_tiled.hip) at 65 .. 1024 items per side, and, under the test hooks
d4_debug_switch("space_attn_tiled" / "cross_attn_tiled", 1), at the shapes the whole-problem-in-LDS kernels also handle.  Every operator
check is against the float64 oracle (oracle/restate.py) at the bounds of the tests these follow (tests/test_gpu_backward.py,
tests/test_gpu_long_clips.py: 2e-4 of each tensor's scale for an operator, 5e-4 for a whole trunk's gradients, 1e-3 for the training
forward's gradients, 1e-5 on the losses).  The oracle evaluated in fp32 stays within 2.3e-6 of scale of its float64 evaluation at every new
operator shape (worst: space (1, 130, 128, ...) 2.29e-6, cross (2, 65, 65, ...) 1.41e-6; the two cap shapes 1.30e-6 and 7.7e-7;
tests/test_wide_frames_host.py asserts <= 2e-5, a tenth of the bound), so the bounds hide nothing."""
import functools

import pytest
import torch

from dreamer4_amd import _lib, trunk_ops
from oracle import restate
from test_gpu_backward import _attn_params, close  # noqa: F401  (_attn_params: the parameters of wide_frames_cases.space_problem)
from wide_frames_cases import (CROSS_SHORT, CROSS_WIDE, SPACE_SHORT, SPACE_WIDE, cross_oracle, cross_problem, space_oracle, space_oracle_run,
                               space_problem)

pytestmark = pytest.mark.gpu


def _space_gpu(shape, **kw):
    F_, S, D, heads, dh, has_rv, ns, clamp, belief = shape
    W, x, rv, dy = space_problem(F_, S, D, heads, dh, has_rv)
    Wg = {k: v.cuda().requires_grad_() for k, v in W.items()}
    xg = x.cuda().requires_grad_()
    rvg = rv.cuda().requires_grad_() if has_rv else None
    y = trunk_ops.space_attention(xg, Wg['norm.weight'], Wg['to_q.weight'], Wg['to_k.weight'], Wg['to_v.weight'], Wg['to_out.weight'],
                                  Wg['to_gates.0.weight'], Wg['k_heads_rmsnorm.gamma'], residual_values=rvg,
                                  mix_weight=Wg['to_learned_value_residual_mix.0.weight'] if has_rv else None,
                                  mix_bias=Wg['to_learned_value_residual_mix.0.bias'] if has_rv else None,
                                  softclamp_value=clamp, num_special=ns, belief=belief, **kw)
    y.backward(dy.cuda())
    out = {'y': y.detach(), 'dx': xg.grad}
    if has_rv:
        out['d residual_values'] = rvg.grad
    out.update({'d ' + k: Wg[k].grad for k in W if has_rv or 'value_residual_mix' not in k})
    return out


def _cross_gpu(shape, **kw):
    G, nq, nk, D, Dc, heads, dh, item_major, ctx_norm, clamp = shape
    W, q, c, dy = cross_problem(G, nq, nk, D, Dc, heads, dh)
    Wg = {k: v.cuda().requires_grad_() for k, v in W.items()}
    qg, cg = q.cuda().requires_grad_(), c.cuda().requires_grad_()
    cin = cg.transpose(0, 1).contiguous() if item_major else cg            # (nk, G, Dc) for the stack-of-hiddens layout
    y = trunk_ops.cross_attention(qg, cin, Wg['norm.weight'], Wg['norm_context.weight'] if ctx_norm else None, Wg['to_q.weight'], Wg['to_k.weight'],
                                  Wg['to_v.weight'], Wg['to_out.weight'], Wg['to_gates.0.weight'], Wg['k_heads_rmsnorm.gamma'],
                                  context_item_major=item_major, softclamp_value=clamp, **kw)
    y.backward(dy.cuda())
    out = {'y': y.detach(), 'dq_tokens': qg.grad, 'dcontext': cg.grad}
    out.update({'d ' + k: Wg[k].grad for k in W if ctx_norm or k != 'norm_context.weight'})
    return out


def _check(ref, got):
    assert set(got) == set(ref)
    for k in ref:
        close(got[k], ref[k], k)


def _hook(name):
    lib = _lib.load()
    assert lib.d4_debug_switch(name, 1) == 0
    try:
        yield
    finally:
        lib.d4_debug_switch(name, 0)


@pytest.fixture
def forced_space():
    yield from _hook(b'space_attn_tiled')


@pytest.fixture
def forced_cross():
    yield from _hook(b'cross_attn_tiled')


# ------------------------------------------------------------------------------------------------ the operators above 64 items
@pytest.mark.parametrize('save_forward', ['1', '0'])
@pytest.mark.parametrize('shape', SPACE_WIDE[:3])
def test_wide_space_attention_vs_oracle_saved_and_recomputed(shape, save_forward, monkeypatch):
    monkeypatch.setenv('D4_TRUNK_SAVE_FORWARD', save_forward)
    _check(space_oracle(shape), _space_gpu(shape, wide=True))


@pytest.mark.parametrize('shape', SPACE_WIDE[3:])
def test_wide_space_attention_vs_oracle(shape):
    _check(space_oracle(shape), _space_gpu(shape, wide=True))


@pytest.mark.parametrize('shape', CROSS_WIDE)
def test_wide_cross_attention_vs_oracle(shape):
    _check(cross_oracle(shape), _cross_gpu(shape, wide=True))


@pytest.mark.parametrize('save_forward', ['1', '0'])
def test_wide_cross_attention_vs_oracle_saved_and_recomputed(save_forward, monkeypatch):
    monkeypatch.setenv('D4_TRUNK_SAVE_FORWARD', save_forward)
    _check(cross_oracle(CROSS_WIDE[3]), _cross_gpu(CROSS_WIDE[3], wide=True))


# ------------------------------------------------------------------------------------------------ the forced tiled core at the LDS kernels' shapes
@pytest.mark.parametrize('shape', SPACE_SHORT)
def test_forced_tiled_core_at_the_short_space_shapes_vs_oracle(shape, forced_space):
    _check(space_oracle(shape), _space_gpu(shape))


@pytest.mark.parametrize('shape', CROSS_SHORT)
def test_forced_tiled_core_at_the_short_cross_shapes_vs_oracle(shape, forced_cross):
    _check(cross_oracle(shape), _cross_gpu(shape))


@pytest.mark.parametrize('name,run,shape', [(b'space_attn_tiled', _space_gpu, SPACE_SHORT[4]), (b'cross_attn_tiled', _cross_gpu, CROSS_SHORT[1])])
def test_the_hooks_really_switch_the_core(name, run, shape):
    """At <= 64 items the default is the LDS kernel: forcing the tiled core changes the bits (another summation order), not the values."""
    lib = _lib.load()
    dx = 'dx' if run is _space_gpu else 'dq_tokens'
    a = run(shape)
    assert lib.d4_debug_switch(name, 1) == 0
    try:
        b = run(shape)
    finally:
        assert lib.d4_debug_switch(name, 0) == 1
    assert not torch.equal(a[dx], b[dx])
    close(b[dx], a[dx], dx, tol=2e-4)


# ------------------------------------------------------------------------------------------------ refusals, and what the opt-in leaves alone
def test_more_than_1024_tokens_per_frame_is_refused_and_leaves_no_damage():
    with pytest.raises(_lib.D4Error, match='1024'):
        _space_gpu((1, 1025, 64, 1, 16, False, 1, 50., True), wide=True)
    torch.cuda.synchronize()
    _check(space_oracle(SPACE_WIDE[0]), _space_gpu(SPACE_WIDE[0], wide=True))


@pytest.mark.parametrize('nq,nk', [(1, 1025), (1025, 1)])
def test_more_than_1024_keys_or_queries_is_refused_and_leaves_no_damage(nq, nk):
    with pytest.raises(_lib.D4Error, match='1024'):
        _cross_gpu((1, nq, nk, 64, 64, 1, 16, False, True, None), wide=True)
    torch.cuda.synchronize()
    _check(cross_oracle(CROSS_WIDE[3]), _cross_gpu(CROSS_WIDE[3], wide=True))


def test_without_wide_more_than_64_tokens_is_refused_as_ever():
    with pytest.raises(_lib.D4Error, match='items per group'):
        _space_gpu((2, 70, 64, 2, 64, True, 1, 50., True))
    with pytest.raises(_lib.D4Error, match='items per group'):
        _space_gpu((2, 70, 64, 2, 64, True, 1, 50., True), wide=False)


def test_without_wide_more_than_64_keys_is_refused_as_ever():
    with pytest.raises(_lib.D4Error, match='queries / .* keys per group'):
        _cross_gpu((6, 1, 70, 64, 64, 2, 32, False, True, None))
    with pytest.raises(_lib.D4Error, match='queries / .* keys per group'):
        _cross_gpu((6, 70, 3, 64, 64, 2, 32, False, True, None), wide=False)


def test_the_opt_in_leaves_no_trace_up_to_64_items():
    for run, shape in ((_space_gpu, SPACE_SHORT[5]), (_cross_gpu, CROSS_SHORT[1])):
        a, b = run(shape, wide=False), run(shape, wide=True)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (shape, k)
    assert _lib.load().d4_train_wide_set(0) == 0                 # every call put the switch back


def test_wide_attention_is_deterministic():
    for run, shape in ((_space_gpu, SPACE_WIDE[1]), (_cross_gpu, CROSS_WIDE[1])):
        a, b = run(shape, wide=True), run(shape, wide=True)
        for k in a:
            assert torch.equal(a[k], b[k]), (shape, k)


def test_wide_is_refused_on_the_dispatcher_route(monkeypatch):
    monkeypatch.setenv('D4_TRUNK_DISPATCHER', '1')
    with pytest.raises(NotImplementedError, match='autograd.Function route'):
        _space_gpu(SPACE_WIDE[0], wide=True)
    with pytest.raises(NotImplementedError, match='autograd.Function route'):
        _cross_gpu(CROSS_WIDE[0], wide=True)


def test_wide_space_attention_bf16_vs_oracle_envelope():
    """The bf16 training mode changes the projections around the core (the core itself stays fp32): the envelope rule of
    tests/test_gpu_train_bf16.py (3 E_max + 2e-4, and at least three tensors moved beyond fp32 noise)."""
    from test_gpu_train_bf16 import _check_block
    shape = SPACE_WIDE[1]
    moved = _check_block(lambda nudge: space_oracle_run(shape, nudge=nudge), lambda: _space_gpu(shape, wide=True, arith='bf16'))
    assert moved >= 3, 'the bf16 arithmetic left no trace: the block ran in fp32'


# ------------------------------------------------------------------------------------------------ the trunk and the world model
TRUNK_KW = dict(dim=64, dim_latent=8, num_latent_tokens=4, depth=4, time_block_every=2, attn_heads=2, attn_dim_head=32, num_discrete_actions=4)


@functools.lru_cache(maxsize=None)
def _trunk_oracle(b, t, s):
    from dreamer4_amd import DynamicsWorldModel
    from util import oracle_config, randomize_weights
    torch.manual_seed(1)
    m = randomize_weights(DynamicsWorldModel(**TRUNK_KW))
    cfg = oracle_config(m)
    W = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith('transformer.')}
    g = torch.Generator().manual_seed(2)
    tokens = torch.randn(b, t, s, cfg.dim, generator=g)
    dy = torch.randn(b, t, s, cfg.dim, generator=g)
    isf = lambda k: W[k].is_floating_point() and 'inv_freq' not in k
    Wd = {k: (v.double().requires_grad_() if isf(k) else v.double()) for k, v in W.items()}
    xd = tokens.double().requires_grad_()
    ref, _ = restate.transformer(cfg, Wd, xd)
    ref.backward(dy.double())
    grads = {k: Wd[k].grad for k in W if isf(k) and Wd[k].grad is not None}
    return cfg, W, tokens, dy, ref.detach(), xd.grad, grads


@pytest.mark.parametrize('b,t,s', [(1, 3, 71), (2, 2, 130)])
def test_trunk_on_wide_frames_vs_oracle_autograd(b, t, s):
    cfg, W, tokens, dy, ref, dtokens, grads = _trunk_oracle(b, t, s)
    isf = lambda k: W[k].is_floating_point() and 'inv_freq' not in k
    Wg = {k: (v.cuda().requires_grad_() if isf(k) else v.cuda()) for k, v in W.items()}
    xg = tokens.cuda().requires_grad_()
    y = trunk_ops.transformer(Wg, xg, is_time=cfg.is_time, softclamp_value=cfg.attn_softclamp_value, wide=True)
    close(y, ref, 'trunk output')
    y.backward(dy.cuda())
    close(xg.grad, dtokens, 'd tokens', tol=5e-4)
    checked = 0
    for k, gr in grads.items():
        assert Wg[k].grad is not None, k
        close(Wg[k].grad, gr, 'd ' + k, tol=5e-4)
        checked += 1
    assert checked >= 20 * cfg.depth


WM_KW = dict(dim=64, dim_latent=8, num_latent_tokens=72, num_spatial_tokens=66, num_register_tokens=8, depth=4, time_block_every=2, attn_heads=2,
             attn_dim_head=32, num_discrete_actions=4)


def _wm_inputs(m, B, T):
    from math import log2
    g = torch.Generator().manual_seed(11)
    lat = torch.randn(B, T, *m.latent_shape, generator=g)
    actions = torch.stack([torch.randint(0, n, (B, T), generator=g) for n in tuple(m.num_discrete_actions)], dim=-1)
    n_log2 = int(log2(m.max_steps))
    step_log2 = torch.randint(1, n_log2, (B,), generator=g)
    nss = (2 ** step_log2)[:, None]
    sig = torch.randint(0, m.max_steps, (B, T), generator=g) // nss * nss
    noise = torch.randn(lat.shape, generator=g)
    return lat, actions, step_log2, sig, noise


def test_world_model_training_forward_on_77_token_frames_vs_oracle():
    """DynamicsWorldModel(train_wide_frames=True): both learned-query pools (66 x 72 and 72 x 66), every space block at 77 tokens per frame and
    the final special cross attention at 76 keys, the draws made here as _training_forward makes them and injected on both sides: flow and
    shortcut losses and the gradient of their sum against the oracle's dynamics_flow_losses (in fp32, as in the test this one follows)."""
    from dreamer4_amd import DynamicsWorldModel
    from util import oracle_config, randomize_weights
    torch.manual_seed(5)
    m = randomize_weights(DynamicsWorldModel(**WM_KW, train_wide_frames=True))
    assert m.train_wide_frames is True
    cfg = oracle_config(m)
    W = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    B, T = 1, 3
    lat, actions, step_log2, sig, noise = _wm_inputs(m, B, T)
    m = m.cuda()
    own = dict(m.named_parameters())
    Wd = {k: (v.clone().requires_grad_() if k in own and v.is_floating_point() else v) for k, v in W.items()}
    rfl, rsl = restate.dynamics_flow_losses(cfg, Wd, lat, noise, sig, step_log2, True, actions=actions)
    (rfl + rsl).backward()

    draws = dict(shortcut_train=True, step_sizes_log2=step_log2, signal_levels=sig, noise=noise)
    total, (fl, sl, *_) = m(latents=lat, discrete_actions=actions, return_all_losses=True, draws=draws, add_autoregressive_action_loss=False)
    print(f'\nflow {fl.item():.8f} (oracle {rfl.item():.8f})  shortcut {sl.item():.8f} (oracle {rsl.item():.8f})')
    close(fl, rfl, 'flow loss', tol=1e-5)
    assert abs(sl.item() - rsl.item()) <= 1e-5 * max(rsl.item(), 1e-3)
    total.backward()
    n = 0
    for k, v in Wd.items():
        if v.requires_grad and v.grad is not None:
            assert own[k].grad is not None, k
            close(own[k].grad, v.grad, 'd ' + k, tol=1e-3); n += 1
    assert n >= 90


def test_world_model_without_train_wide_frames_refuses_77_token_frames():
    from dreamer4_amd import DynamicsWorldModel
    from util import randomize_weights
    torch.manual_seed(5)
    m = randomize_weights(DynamicsWorldModel(**WM_KW))
    assert m.train_wide_frames is False
    lat, actions, step_log2, sig, noise = _wm_inputs(m, 1, 3)
    m = m.cuda()
    draws = dict(shortcut_train=True, step_sizes_log2=step_log2, signal_levels=sig, noise=noise)
    with pytest.raises(_lib.D4Error, match='per group'):
        m(latents=lat, discrete_actions=actions, return_all_losses=True, draws=draws, add_autoregressive_action_loss=False)
