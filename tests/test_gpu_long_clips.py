"""GPU: the tiled time-attention core of the training path (csrc/attn_tiled.hip) — clips of 65 .. 1024 frames, and, under the test hook
d4_debug_switch("time_attn_tiled", 1), the shapes the whole-problem-in-LDS kernel also handles.  Every check is against the float64 oracle
(oracle/restate.py) at the tolerances of the tests these were copied from (tests/test_gpu_backward.py: 2e-4 of each tensor's scale for an
operator, 5e-4 for a whole trunk's gradients, 1e-3 for the training forward's).  The oracle evaluated in fp32 stays <= 5.2e-6 of scale
from float64 up to 256 frames and at 1.5e-5 at 1024, so the bounds hide nothing."""
import functools

import pytest
import torch

from dreamer4_amd import _lib, trunk_ops
from oracle import restate
from test_gpu_backward import _attn_params, close

pytestmark = pytest.mark.gpu

LONG = [(1, 65, 2, 64, 2, 64, True, 50.),          # one full tile plus one key
        (2, 100, 3, 64, 3, 32, False, 50.),        # ragged tail, no residual, three heads
        (1, 130, 2, 128, 2, 16, True, 3.),         # tight clamp, dh 16
        (1, 128, 2, 64, 2, 64, True, 50.),         # exact tile multiple
        (1, 192, 1, 64, 1, 64, True, 50.),
        (2, 80, 15, 128, 2, 64, True, 50.),        # cfg-2 token count
        (1, 1024, 1, 64, 1, 16, True, 50.)]        # the cap
SHORT = [(2, 7, 5, 64, 2, 64, True, 50.), (1, 32, 3, 64, 3, 32, False, 50.), (3, 16, 15, 128, 2, 16, True, 3.), (1, 64, 2, 64, 2, 64, True, 50.),
         (2, 48, 3, 64, 1, 32, False, 50.)]


@functools.lru_cache(maxsize=None)
def _problem(B, T, S, D, heads, dh, has_rv):
    g = torch.Generator().manual_seed(9)
    W = _attn_params(D, heads, dh, g)
    x = torch.randn(B, T, S, D, generator=g) * 1.5
    rv = torch.randn(B, T, S, heads, dh, generator=g) if has_rv else None
    dy = torch.randn(B, T, S, D, generator=g)
    inv_freq = 1.0 / (10000. ** (torch.arange(0, dh, 2).float() / dh))
    return W, x, rv, dy, inv_freq


def _oracle_run(shape, nudge=0.):
    from einops import rearrange
    B, T, S, D, heads, dh, has_rv, clamp = shape
    W, x, rv, dy, inv_freq = _problem(B, T, S, D, heads, dh, has_rv)
    Wd = {k: (v.double() * (1. + nudge)).requires_grad_() for k, v in W.items()}
    xd = (x.double() * (1. + nudge)).requires_grad_()
    rvd = (rv.double() * (1. + nudge)).requires_grad_() if has_rv else None
    # the reference runs the time layers on 'b t s d -> (b s) t d' (dreamer4.py:3178), causal, rotary positions 0..T-1
    rot = restate.rotary_freqs(restate.Config(dim=D, dim_latent=4, num_latent_tokens=1, attn_dim_head=dh), T, 0, inv_freq.double())
    ref, _ = restate.attention(Wd, '', rearrange(xd, 'b t s d -> (b s) t d'), heads=heads, dim_head=dh, rot=rot, causal=True,
                               residual_values=rearrange(rvd, 'b t s h d -> (b s) t h d') if has_rv else None, softclamp_value=clamp)
    ref = rearrange(ref, '(b s) t d -> b t s d', b=B)
    ref.backward(dy.double())
    out = {'y': ref.detach(), 'dx': xd.grad}
    if has_rv:
        out['d residual_values'] = rvd.grad
    out.update({'d ' + k: Wd[k].grad for k in W if has_rv or 'value_residual_mix' not in k})
    return out


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """float64 reference of one shape: computed once, shared by every test of the shape, never written to."""
    return _oracle_run(shape)


def _gpu(shape, **kw):
    B, T, S, D, heads, dh, has_rv, clamp = shape
    W, x, rv, dy, inv_freq = _problem(B, T, S, D, heads, dh, has_rv)
    Wg = {k: v.cuda().requires_grad_() for k, v in W.items()}
    xg = x.cuda().requires_grad_()
    rvg = rv.cuda().requires_grad_() if has_rv else None
    y = trunk_ops.time_attention(xg, Wg['norm.weight'], Wg['to_q.weight'], Wg['to_k.weight'], Wg['to_v.weight'], Wg['to_out.weight'],
                                 Wg['to_gates.0.weight'], Wg['k_heads_rmsnorm.gamma'], inv_freq.cuda(), residual_values=rvg,
                                 mix_weight=Wg['to_learned_value_residual_mix.0.weight'] if has_rv else None,
                                 mix_bias=Wg['to_learned_value_residual_mix.0.bias'] if has_rv else None, softclamp_value=clamp, **kw)
    y.backward(dy.cuda())
    out = {'y': y.detach(), 'dx': xg.grad}
    if has_rv:
        out['d residual_values'] = rvg.grad
    out.update({'d ' + k: Wg[k].grad for k in W if has_rv or 'value_residual_mix' not in k})
    return out


def _check(shape):
    ref, got = _oracle(shape), _gpu(shape)
    assert set(got) == set(ref)
    for k in ref:
        close(got[k], ref[k], k)


@pytest.fixture
def forced_tiled():
    lib = _lib.load()
    assert lib.d4_debug_switch(b'time_attn_tiled', 1) == 0
    try:
        yield
    finally:
        lib.d4_debug_switch(b'time_attn_tiled', 0)


@pytest.mark.parametrize('save_forward', ['1', '0'])
@pytest.mark.parametrize('shape', LONG[:4])
def test_long_time_attention_vs_oracle_saved_and_recomputed(shape, save_forward, monkeypatch):
    monkeypatch.setenv('D4_TRUNK_SAVE_FORWARD', save_forward)
    _check(shape)


@pytest.mark.parametrize('shape', LONG[4:])
def test_long_time_attention_vs_oracle(shape):
    _check(shape)


@pytest.mark.parametrize('shape', SHORT)
def test_forced_tiled_core_at_the_short_shapes_vs_oracle(shape, forced_tiled):
    _check(shape)


def test_the_hook_really_switches_the_core():
    """At <= 64 frames the default is the LDS kernel: forcing the tiled core changes the bits (another summation order), not the values."""
    lib = _lib.load()
    a = _gpu(SHORT[3])
    assert lib.d4_debug_switch(b'time_attn_tiled', 1) == 0
    try:
        b = _gpu(SHORT[3])
    finally:
        assert lib.d4_debug_switch(b'time_attn_tiled', 0) == 1
    assert lib.d4_debug_switch(b'no_such_switch', 1) == -1
    assert not torch.equal(a['dx'], b['dx'])
    close(b['dx'], a['dx'], 'dx', tol=2e-4)


def test_long_time_attention_is_deterministic():
    a, b = _gpu(LONG[1]), _gpu(LONG[1])
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_more_than_1024_frames_is_refused_and_leaves_no_damage():
    with pytest.raises(_lib.D4Error, match='1024'):
        _gpu((1, 1025, 1, 64, 1, 16, False, 50.))
    torch.cuda.synchronize()
    _check(LONG[0])


def test_long_time_attention_bf16_vs_oracle_envelope():
    """The bf16 training mode changes the projections around the core (the core itself stays fp32): the envelope rule of
    tests/test_gpu_train_bf16.py (3 E_max + 2e-4, and at least three tensors moved beyond fp32 noise)."""
    from test_gpu_train_bf16 import _check_block
    shape = LONG[1]
    moved = _check_block(lambda nudge: _oracle_run(shape, nudge), lambda: _gpu(shape, arith='bf16'))
    assert moved >= 3, 'the bf16 arithmetic left no trace: the block ran in fp32'


TRUNK_KW = dict(dim=64, dim_latent=8, num_latent_tokens=4, depth=4, time_block_every=2, attn_heads=2, attn_dim_head=32, num_discrete_actions=4)


@functools.lru_cache(maxsize=None)
def _trunk_oracle(b, t):
    from dreamer4_amd import DynamicsWorldModel
    from util import oracle_config, randomize_weights
    torch.manual_seed(1)
    m = randomize_weights(DynamicsWorldModel(**TRUNK_KW))
    cfg = oracle_config(m)
    W = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith('transformer.')}
    s = 1 + cfg.num_spatial_tokens + cfg.num_register_tokens + 1 + 1            # flow | spatial | registers | action | agent
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


@pytest.mark.parametrize('dispatcher', ['0', '1'])
@pytest.mark.parametrize('b,t', [(1, 70), (2, 130)])
def test_trunk_on_long_clips_vs_oracle_autograd(b, t, dispatcher, monkeypatch):
    monkeypatch.setenv('D4_TRUNK_DISPATCHER', dispatcher)
    cfg, W, tokens, dy, ref, dtokens, grads = _trunk_oracle(b, t)
    isf = lambda k: W[k].is_floating_point() and 'inv_freq' not in k
    Wg = {k: (v.cuda().requires_grad_() if isf(k) else v.cuda()) for k, v in W.items()}
    xg = tokens.cuda().requires_grad_()
    y = trunk_ops.transformer(Wg, xg, is_time=cfg.is_time, softclamp_value=cfg.attn_softclamp_value)
    close(y, ref, 'trunk output')
    y.backward(dy.cuda())
    close(xg.grad, dtokens, 'd tokens', tol=5e-4)
    checked = 0
    for k, gr in grads.items():
        assert Wg[k].grad is not None, k
        close(Wg[k].grad, gr, 'd ' + k, tol=5e-4)
        checked += 1
    assert checked >= 20 * cfg.depth


def test_world_model_training_forward_on_a_72_frame_clip_vs_oracle():
    """DynamicsWorldModel's training forward on a clip longer than the LDS core's 64 frames, the draws made here as _training_forward makes
    them and injected on both sides: flow and shortcut losses and the gradient of their sum against the oracle's dynamics_flow_losses
    (in fp32, as the fixture of the test this one follows was made; it stays within 2.5e-8 on the loss and 1.5e-6 of scale on the worst
    gradient of its float64 evaluation)."""
    from math import log2
    from util import golden_model, golden_oracle
    cfg, W = golden_oracle('weights_train.npz')
    m = golden_model('weights_train.npz').cuda()
    B, T = 2, 72
    g = torch.Generator().manual_seed(11)
    lat = torch.randn(B, T, *m.latent_shape, generator=g)
    nda = cfg.num_discrete_actions
    nda = (nda,) if isinstance(nda, int) else tuple(nda)
    actions = torch.stack([torch.randint(0, n, (B, T), generator=g) for n in nda], dim=-1)
    n_log2 = int(log2(m.max_steps))
    step_log2 = torch.randint(1, n_log2, (B,), generator=g)
    nss = (2 ** step_log2)[:, None]
    sig = torch.randint(0, m.max_steps, (B, T), generator=g) // nss * nss
    noise = torch.randn(lat.shape, generator=g)

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
