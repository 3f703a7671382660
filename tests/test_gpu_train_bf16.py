"""GPU: the bf16 training arithmetic of the dynamics trunk (`DynamicsWorldModel(train_matmul_dtype='bf16')`, `trunk_ops.*(arith='bf16')`,
DESIGN.md 8): the weight-gradient kernel d4_gemm_tn_bf16 against float64 of the same bf16 operands, bit reproducibility, the four blocks and
the whole training forward against the ORACLE'S OWN bf16 noise envelope (tests/bf16_emulation.py: bounds come from oracle/restate.py and the
fixtures alone, never from the code under test), a short optimisation, and the fp32 path left bit-identical.

Block bound: per tensor, in the fp32 block tests' own metric (max |a - b| / max |b| against the float64 oracle), 3 x the largest distance of
the oracle's four bf16 variants + 2e-4 (the fp32 tests' tolerance in that metric).  Model bound: the table in `bf16_emulation.check_model`."""
import hashlib
import os
import subprocess
import sys

import pytest
import torch

import bf16_emulation as emu
from dreamer4_amd import _lib, trunk_ops
from oracle import restate

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def stream():
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ 1. the kernel
CFG2_K, CFG5_K = 3840, 1792
TN_SHAPES = [(512, 512, CFG2_K), (1536, 512, CFG2_K), (2730, 512, CFG2_K), (512, 1365, CFG2_K),               # config 2's weight gradients
             (1024, 1024, CFG5_K), (5460, 1024, CFG5_K), (1024, 2730, 2048),                                   # config 5's
             (45, 388, 100), (45, 388, 17), (130, 70, 1), (7, 300, 333), (200, 5, 64), (3, 2, 40), (128, 128, 32), (129, 257, 4097)]


@pytest.mark.parametrize('M,N,K', TN_SHAPES)
@pytest.mark.parametrize('slices', [0, 3])
def test_gemm_tn_bf16_kernel(M, N, K, slices):
    """C = A^T B over the operands' rows, bf16 images in, fp32 out: against float64 of the SAME bf16 operands at the tolerance of the project's
    bf16 kernel tests; ragged M, N, K; leading dimensions wider than the matrices; C pre-filled with NaN and untouched outside M x N."""
    lib = _lib.load()
    g = torch.Generator(device='cuda').manual_seed(M * 7 + N * 3 + K)
    lda, ldb, ldc = (M + 7) // 8 * 8 + 8, (N + 7) // 8 * 8, N + 3
    A = torch.randn(K, lda, device='cuda', generator=g).to(torch.bfloat16).contiguous()
    B = torch.randn(K, ldb, device='cuda', generator=g).to(torch.bfloat16).contiguous()
    A[:, M:] = float('nan'); B[:, N:] = float('nan')                       # columns past the matrix must not leak into it
    C_ = torch.full((M + 2, ldc), float('nan'), device='cuda')
    part = torch.empty(max(slices, 16) * M * N if slices else 8 << 20, device='cuda')
    _lib.check(lib.d4_gemm_tn_bf16(_lib.ptr(A), lda, _lib.ptr(B), ldb, _lib.ptr(C_), ldc, M, N, K, _lib.ptr(part), part.numel(), slices, stream()))
    torch.cuda.synchronize()
    ref = A[:, :M].double().t() @ B[:, :N].double()
    assert torch.isnan(C_[M:]).all() and torch.isnan(C_[:, N:]).all(), 'wrote outside M x N'
    err = (C_[:M, :N].double() - ref).abs().max().item()
    tol = 3e-6 * max(1., ref.abs().max().item()) * max(1., K / 256) ** 0.5
    assert err <= tol, f'M{M} N{N} K{K} slices{slices}: err {err:.3e} > {tol:.3e}'
    # without scratch: one slice, same contract
    C1 = torch.full((M, ldc), float('nan'), device='cuda')
    _lib.check(lib.d4_gemm_tn_bf16(_lib.ptr(A), lda, _lib.ptr(B), ldb, _lib.ptr(C1), ldc, M, N, K, None, 0, 0, stream()))
    assert (C1[:, :N].double() - ref).abs().max().item() <= tol
    # 2. the same call twice: the same bits
    C2 = torch.full((M + 2, ldc), float('nan'), device='cuda')
    _lib.check(lib.d4_gemm_tn_bf16(_lib.ptr(A), lda, _lib.ptr(B), ldb, _lib.ptr(C2), ldc, M, N, K, _lib.ptr(part), part.numel(), slices, stream()))
    assert torch.equal(C2[:M, :N], C_[:M, :N])


def test_gemm_tn_bf16_rejects_bad_images():
    lib = _lib.load()
    A = torch.zeros(16, 12, device='cuda', dtype=torch.bfloat16)
    C_ = torch.zeros(12, 12, device='cuda')
    with pytest.raises(_lib.D4Error, match='multiples of 8'):
        _lib.check(lib.d4_gemm_tn_bf16(_lib.ptr(A), 12, _lib.ptr(A), 12, _lib.ptr(C_), 12, 12, 12, 16, None, 0, 0, stream()))


# ------------------------------------------------------------------------------------------------ 3. the blocks
def _check_block(run_oracle, run_gpu, tol=2e-4):
    ref = {k: v.detach().clone() for k, v in run_oracle(0.).items()}
    E = emu.envelope(emu.run_variants(run_oracle), ref, emu.scaled_max)
    got = run_gpu()
    assert set(got) == set(ref)
    bad, moved = [], 0
    print('\n--- block ' + os.environ.get('PYTEST_CURRENT_TEST', '').split('::')[-1])
    for k in ref:
        d = emu.scaled_max(got[k], ref[k])
        print(f'  {k}: {d:.3e}  (E_max {E[k]:.3e}, bound {3 * E[k] + tol:.3e})')
        moved += d > tol
        if not d <= 3. * E[k] + tol:
            bad.append((k, d, E[k]))
    assert not bad, bad
    return moved


def _leaves(W, nudge):
    return {k: (v.double() * (1. + nudge)).requires_grad_() for k, v in W.items()}


def _cuda_leaves(W):
    return {k: v.cuda().requires_grad_() for k, v in W.items()}


@pytest.mark.parametrize('save_forward', ['1', '0'])
@pytest.mark.parametrize('lead,D,inner', [((37,), 64, 170), ((3, 100), 512, 1365), ((1,), 32, 85)])
def test_feedforward_bf16_vs_oracle_envelope(lead, D, inner, save_forward, monkeypatch):
    from test_gpu_backward import _ff_params
    monkeypatch.setenv('D4_TRUNK_SAVE_FORWARD', save_forward)
    g = torch.Generator().manual_seed(3)
    W = _ff_params(D, inner, g)
    x = torch.randn(*lead, D, generator=g) * 1.5
    dy = torch.randn(*lead, D, generator=g)

    def oracle(nudge):
        Wd, xd = _leaves(W, nudge), (x.double() * (1. + nudge)).requires_grad_()
        y = restate.feedforward(Wd, '', xd)
        y.backward(dy.double())
        return {'y': y, 'dx': xd.grad, **{'d ' + k: Wd[k].grad for k in W}}

    def gpu():
        Wg, xg = _cuda_leaves(W), x.cuda().requires_grad_()
        y = trunk_ops.feedforward(xg, Wg['norm.weight'], Wg['proj_in.weight'], Wg['proj_in.bias'], Wg['proj_out.weight'], Wg['proj_out.bias'], arith='bf16')
        y.backward(dy.cuda())
        return {'y': y, 'dx': xg.grad, **{'d ' + k: Wg[k].grad for k in W}}
    moved = _check_block(oracle, gpu)
    assert moved >= 3, 'the bf16 arithmetic left no trace: the block ran in fp32'


SPACE = [(5, 9, 64, 2, 64, True, 1, 50., True), (3, 30, 128, 3, 32, False, 6, 50., True), (4, 12, 64, 5, 16, True, 0, 2., False),
         (130, 15, 512, 8, 64, True, 1, 50., True), (3, 64, 64, 2, 64, True, 2, 50., True), (2, 41, 64, 2, 32, True, 1, 50., True)]


def _attn_kw(Wg, has_rv):
    return dict(mix_weight=Wg['to_learned_value_residual_mix.0.weight'] if has_rv else None,
                mix_bias=Wg['to_learned_value_residual_mix.0.bias'] if has_rv else None)


def _attn_grads(W, Wl, has_rv):
    return {'d ' + k: Wl[k].grad for k in W if has_rv or 'value_residual_mix' not in k}


@pytest.mark.parametrize('save_forward', ['1', '0'])
@pytest.mark.parametrize('F_,S,D,heads,dh,has_rv,ns,clamp,belief', SPACE)
def test_space_attention_bf16_vs_oracle_envelope(F_, S, D, heads, dh, has_rv, ns, clamp, belief, save_forward, monkeypatch):
    from test_gpu_backward import _attn_params
    monkeypatch.setenv('D4_TRUNK_SAVE_FORWARD', save_forward)
    g = torch.Generator().manual_seed(7)
    W = _attn_params(D, heads, dh, g)
    x = torch.randn(F_, S, D, generator=g) * 1.5
    rv = torch.randn(F_, S, heads, dh, generator=g) if has_rv else None
    dy = torch.randn(F_, S, D, generator=g)
    mask = restate.special_token_mask(S, ns) if ns > 0 else None

    def oracle(nudge):
        Wd, xd = _leaves(W, nudge), (x.double() * (1. + nudge)).requires_grad_()
        rvd = (rv.double() * (1. + nudge)).requires_grad_() if has_rv else None
        y, _ = restate.attention(Wd, '', xd, heads=heads, dim_head=dh, residual_values=rvd, softclamp_value=clamp, mask=mask, belief=belief)
        y.backward(dy.double())
        out = {'y': y, 'dx': xd.grad, **_attn_grads(W, Wd, has_rv)}
        if has_rv:
            out['d rv'] = rvd.grad
        return out

    def gpu():
        Wg, xg = _cuda_leaves(W), x.cuda().requires_grad_()
        rvg = rv.cuda().requires_grad_() if has_rv else None
        y = trunk_ops.space_attention(xg, Wg['norm.weight'], Wg['to_q.weight'], Wg['to_k.weight'], Wg['to_v.weight'], Wg['to_out.weight'],
                                      Wg['to_gates.0.weight'], Wg['k_heads_rmsnorm.gamma'], residual_values=rvg, **_attn_kw(Wg, has_rv),
                                      softclamp_value=clamp, num_special=ns, belief=belief, arith='bf16')
        y.backward(dy.cuda())
        out = {'y': y, 'dx': xg.grad, **_attn_grads(W, Wg, has_rv)}
        if has_rv:
            out['d rv'] = rvg.grad
        return out
    assert _check_block(oracle, gpu) >= 3


@pytest.mark.parametrize('save_forward', ['1', '0'])
@pytest.mark.parametrize('B,T,S,D,heads,dh,has_rv,clamp', [(2, 7, 5, 64, 2, 64, True, 50.), (1, 32, 3, 64, 3, 32, False, 50.), (3, 16, 15, 128, 2, 16, True, 3.),
                                                           (1, 64, 2, 64, 2, 64, True, 50.), (2, 48, 3, 64, 1, 32, False, 50.)])
def test_time_attention_bf16_vs_oracle_envelope(B, T, S, D, heads, dh, has_rv, clamp, save_forward, monkeypatch):
    from einops import rearrange
    from test_gpu_backward import _attn_params
    monkeypatch.setenv('D4_TRUNK_SAVE_FORWARD', save_forward)
    g = torch.Generator().manual_seed(9)
    W = _attn_params(D, heads, dh, g)
    x = torch.randn(B, T, S, D, generator=g) * 1.5
    rv = torch.randn(B, T, S, heads, dh, generator=g) if has_rv else None
    dy = torch.randn(B, T, S, D, generator=g)
    inv_freq = 1.0 / (10000. ** (torch.arange(0, dh, 2).float() / dh))
    rot = restate.rotary_freqs(restate.Config(dim=D, dim_latent=4, num_latent_tokens=1, attn_dim_head=dh), T, 0, inv_freq.double())

    def oracle(nudge):
        Wd, xd = _leaves(W, nudge), (x.double() * (1. + nudge)).requires_grad_()
        rvd = (rv.double() * (1. + nudge)).requires_grad_() if has_rv else None
        y, _ = restate.attention(Wd, '', rearrange(xd, 'b t s d -> (b s) t d'), heads=heads, dim_head=dh, rot=rot, causal=True,
                                 residual_values=rearrange(rvd, 'b t s h d -> (b s) t h d') if has_rv else None, softclamp_value=clamp)
        y = rearrange(y, '(b s) t d -> b t s d', b=B)
        y.backward(dy.double())
        out = {'y': y, 'dx': xd.grad, **_attn_grads(W, Wd, has_rv)}
        if has_rv:
            out['d rv'] = rvd.grad
        return out

    def gpu():
        Wg, xg = _cuda_leaves(W), x.cuda().requires_grad_()
        rvg = rv.cuda().requires_grad_() if has_rv else None
        y = trunk_ops.time_attention(xg, Wg['norm.weight'], Wg['to_q.weight'], Wg['to_k.weight'], Wg['to_v.weight'], Wg['to_out.weight'],
                                     Wg['to_gates.0.weight'], Wg['k_heads_rmsnorm.gamma'], inv_freq.cuda(), residual_values=rvg, **_attn_kw(Wg, has_rv),
                                     softclamp_value=clamp, arith='bf16')
        y.backward(dy.cuda())
        out = {'y': y, 'dx': xg.grad, **_attn_grads(W, Wg, has_rv)}
        if has_rv:
            out['d rv'] = rvg.grad
        return out
    assert _check_block(oracle, gpu) >= 3


@pytest.mark.parametrize('save_forward', ['1', '0'])
@pytest.mark.parametrize('G,nq,nk,D,Dc,heads,dh,item_major,ctx_norm,clamp', [
    (37, 1, 7, 64, 64, 4, 64, True, True, None), (6, 3, 20, 64, 64, 2, 32, False, True, None), (5, 4, 64, 128, 8, 3, 16, False, True, 5.),
    (9, 64, 5, 64, 32, 2, 64, False, False, None)])
def test_cross_attention_bf16_vs_oracle_envelope(G, nq, nk, D, Dc, heads, dh, item_major, ctx_norm, clamp, save_forward, monkeypatch):
    monkeypatch.setenv('D4_TRUNK_SAVE_FORWARD', save_forward)
    g = torch.Generator().manual_seed(13)
    r = lambda *s_, k=1.: torch.randn(*s_, generator=g) * k
    hd = heads * dh
    W = {'norm.weight': 1. + r(D, k=.1), 'norm_context.weight': 1. + r(Dc, k=.1), 'to_q.weight': r(hd, D, k=3. * D ** -.5), 'to_k.weight': r(hd, Dc, k=Dc ** -.5),
         'to_v.weight': r(hd, Dc, k=Dc ** -.5), 'to_out.weight': r(D, hd, k=hd ** -.5), 'to_gates.0.weight': r(heads, D, k=D ** -.5),
         'k_heads_rmsnorm.gamma': r(heads, dh, k=.3)}
    q, c, dy = r(G, nq, D, k=1.5), r(G, nk, Dc, k=1.5), r(G, nq, D)
    used = [k for k in W if ctx_norm or k != 'norm_context.weight']

    def oracle(nudge):
        Wd = _leaves(W, nudge)
        qd, cd = (q.double() * (1. + nudge)).requires_grad_(), (c.double() * (1. + nudge)).requires_grad_()
        y, _ = restate.attention(Wd, '', qd, heads=heads, dim_head=dh, context=cd, belief=True, has_ctx_norm=ctx_norm, softclamp_value=clamp)
        y.backward(dy.double())
        return {'y': y, 'dq': qd.grad, 'dc': cd.grad, **{'d ' + k: Wd[k].grad for k in used}}

    def gpu():
        Wg, qg, cg = _cuda_leaves(W), q.cuda().requires_grad_(), c.cuda().requires_grad_()
        cin = cg.transpose(0, 1).contiguous() if item_major else cg
        y = trunk_ops.cross_attention(qg, cin, Wg['norm.weight'], Wg['norm_context.weight'] if ctx_norm else None, Wg['to_q.weight'], Wg['to_k.weight'],
                                      Wg['to_v.weight'], Wg['to_out.weight'], Wg['to_gates.0.weight'], Wg['k_heads_rmsnorm.gamma'],
                                      context_item_major=item_major, softclamp_value=clamp, arith='bf16')
        y.backward(dy.cuda())
        return {'y': y, 'dq': qg.grad, 'dc': cg.grad, **{'d ' + k: Wg[k].grad for k in used}}
    assert _check_block(oracle, gpu) >= 3


# ------------------------------------------------------------------------------------------------ 4. the model
def _train_step(m, g, name='shortcut', **kw):
    from util import t
    draws = dict(shortcut_train=name == 'shortcut', step_sizes_log2=t(g[name + '_step_sizes_log2']), signal_levels=t(g[name + '_signal_levels']),
                 noise=t(g[name + '_noise']))
    m.zero_grad(set_to_none=True)
    total, (fl, sl, *_) = m(latents=t(g['latents']), discrete_actions=t(g['actions']), return_all_losses=True, draws=draws, add_autoregressive_action_loss=False, **kw)
    total.backward()
    return total, fl, sl


@pytest.mark.parametrize('name', ['shortcut', 'plain'])
def test_training_forward_bf16_inside_the_oracle_envelope_train_npz(name):
    """train.npz with the fixture's draws injected: both loss terms and the >= 90 gradient tensors the fp32 test counts, none left out."""
    from util import golden_model, load_golden
    run, ref = emu.train_fixture(name)
    E, G, L, _ = emu.model_envelope(run, ref)
    g = load_golden('train.npz')
    m = golden_model('weights_train.npz', train_matmul_dtype='bf16').cuda()
    total, fl, sl = _train_step(m, g, name)
    own = dict(m.named_parameters())
    got = {'loss/flow': fl, 'loss/shortcut': sl}
    for k in ref:
        if k.startswith('grad/'):
            assert own[k[5:]].grad is not None, k
            got[k] = own[k[5:]].grad
    assert sum(k.startswith('grad/') for k in ref) >= 90
    report = []
    bad = emu.check_model(got, ref, E, G, L, report)
    print(f'\n--- train.npz ({name}) bf16 training arithmetic vs the oracle envelope'); print('\n'.join(report))
    assert not bad, bad
    # the mode is really on: the gradients differ from the fixture by bf16 noise, not fp32 noise
    assert emu.global_rel_l2(got, ref, [k for k in ref if k.startswith('grad/')]) > 1e-3


def test_training_forward_bf16_inside_the_oracle_envelope_train_agent_npz():
    """train_agent.npz (rewards, terminals, two action types): every loss term, the total and the 134 gradient tensors."""
    from util import golden_model, load_golden, t
    run, ref = emu.train_agent_fixture()
    E, G, L, _ = emu.model_envelope(run, ref)
    g = load_golden('train_agent.npz')
    m = golden_model('weights_train_agent.npz', train_matmul_dtype='bf16').cuda()
    draws = dict(shortcut_train=True, step_sizes_log2=t(g['step_sizes_log2']), signal_levels=t(g['signal_levels']), noise=t(g['noise']))
    total, Ls = m(latents=t(g['latents']), discrete_actions=t(g['actions']), rewards=t(g['rewards']), terminals=t(g['terminals']),
                  return_all_losses=True, draws=draws)
    total.backward()
    own = dict(m.named_parameters())
    got = {'loss/flow': Ls.flow, 'loss/shortcut': Ls.shortcut, 'loss/rewards': Ls.rewards, 'loss/terminals': Ls.terminals,
           'loss/discrete_actions': Ls.discrete_actions, 'loss/total': total}
    n = 0
    for k in ref:
        if k.startswith('grad/'):
            assert own[k[5:]].grad is not None, k
            got[k] = own[k[5:]].grad; n += 1
    assert n >= 130
    report = []
    bad = emu.check_model(got, ref, E, G, L, report)
    print('\n--- train_agent.npz bf16 training arithmetic vs the oracle envelope'); print('\n'.join(report))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 2. reproducibility
def _step_digest():
    """sha256 over the loss and every gradient of one bf16-mode training step on train.npz (fixture draws)."""
    from util import golden_model, load_golden
    g = load_golden('train.npz')
    m = golden_model('weights_train.npz', train_matmul_dtype='bf16').cuda()
    total, _, _ = _train_step(m, g)
    h = hashlib.sha256(total.detach().cpu().numpy().tobytes())
    n = 0
    for k, p in sorted(m.named_parameters()):
        if p.grad is not None:
            h.update(k.encode()); h.update(p.grad.detach().cpu().numpy().tobytes()); n += 1
    assert n >= 90
    return h.hexdigest()


def test_a_bf16_training_step_is_reproducible_bit_for_bit():
    a, b = _step_digest(), _step_digest()
    assert a == b
    env = dict(os.environ, D4_GEMM_AUTOTUNE='0')
    code = f'import sys; sys.path[:0] = [{HERE!r}, {os.path.dirname(HERE)!r}]; import test_gpu_train_bf16 as t; print("DIGEST", t._step_digest())'
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    child = [l.split()[1] for l in out.stdout.splitlines() if l.startswith('DIGEST')]
    assert child == [a], (child, a)


# ------------------------------------------------------------------------------------------------ 5. it trains
def test_bf16_training_reduces_the_loss():
    """The 40-step AdamW run of test_world_model_training_forward_matches_the_fixture_and_trains in bf16 mode, same criterion on fixed draws."""
    from util import golden_model, load_golden, t
    g = load_golden('train.npz')
    m = golden_model('weights_train.npz', train_matmul_dtype='bf16').cuda()
    _train_step(m, g)
    trunk = [p for k, p in m.named_parameters() if p.grad is not None]
    assert all(p.grad.dtype == torch.float32 and p.dtype == torch.float32 for p in trunk)          # fp32 gradients on fp32 master weights
    opt = torch.optim.AdamW(trunk, lr=3e-3, weight_decay=0.)
    gen = torch.Generator(device='cuda').manual_seed(3)
    lat = t(g['latents']).cuda()
    B_, T_ = lat.shape[:2]
    fixed = dict(shortcut_train=False, step_sizes_log2=torch.zeros(B_, dtype=torch.long), signal_levels=torch.randint(0, m.max_steps, (B_, T_), generator=torch.Generator().manual_seed(5)),
                 noise=torch.randn(lat.shape, generator=torch.Generator().manual_seed(6)))
    probe = lambda: m(latents=lat, discrete_actions=t(g['actions']), draws=fixed, add_autoregressive_action_loss=False).item()
    with torch.no_grad():
        first = probe()
    for step in range(40):
        opt.zero_grad(set_to_none=True)
        loss = m(latents=lat, discrete_actions=t(g['actions']), generator=gen, add_autoregressive_action_loss=False)
        loss.backward()
        opt.step()
        m.invalidate_prepared()
    with torch.no_grad():
        last = probe()
    assert last < 0.85 * first, (first, last)


# ------------------------------------------------------------------------------------------------ 6. nothing else moved
def test_fp32_mode_is_bit_identical_and_its_workspaces_unchanged():
    from util import golden_model, load_golden
    lib = _lib.load()
    g = load_golden('train.npz')
    res = []
    for extra in ({}, dict(train_matmul_dtype='fp32')):
        m = golden_model('weights_train.npz', **extra).cuda()
        assert m.train_matmul_dtype == 'fp32'
        total, fl, sl = _train_step(m, g)
        res.append((total.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    # a bf16 step in between must not leak into a later fp32 step (the arithmetic switch is process-wide)
    _train_step(golden_model('weights_train.npz', train_matmul_dtype='bf16').cuda(), g)
    assert lib.d4_train_arith_get() == 0
    m = golden_model('weights_train.npz').cuda()
    total, _, _ = _train_step(m, g)
    res.append((total.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    for tot, grads in res[1:]:
        assert torch.equal(tot, res[0][0]) and grads.keys() == res[0][1].keys()
        for k in grads:
            assert torch.equal(grads[k], res[0][1][k]), k
    assert len(res[0][1]) >= 90
    # the blocks' workspaces are the fp32 ones in both arithmetics; the bf16 images live in a scratch of their own that only lives for a call
    W = {k: v.cuda().requires_grad_() for k, v in __import__('test_gpu_backward')._ff_params(512, 1365, torch.Generator().manual_seed(0)).items()}
    x = torch.randn(3840, 512, device='cuda')
    held = {}
    for arith in ('fp32', 'bf16'):
        torch.cuda.synchronize(); before = torch.cuda.memory_allocated()
        y = trunk_ops.feedforward(x, *W.values(), arith=arith)
        torch.cuda.synchronize(); held[arith] = torch.cuda.memory_allocated() - before
        del y
    assert held['bf16'] == held['fp32'], held          # nothing of the bf16 scratch is kept alive for the backward
    assert lib.d4_ff_bf16_scratch_bytes(3840, 512, 1365) > 0 and lib.d4_attn_bf16_scratch_bytes(3840, 512, 8, 64) > 0
    assert lib.d4_cross_attn_bf16_scratch_bytes(3840, 1, 13, 512, 512, 8, 64) > 0


# ------------------------------------------------------------------------------------------------ 7. bad values
def test_bad_arithmetic_names_raise(monkeypatch):
    from dreamer4_amd import DynamicsWorldModel
    from test_gpu_backward import _ff_params
    with pytest.raises(ValueError, match='train_matmul_dtype'):
        DynamicsWorldModel(dim=64, dim_latent=8, num_latent_tokens=4, depth=2, attn_heads=2, train_matmul_dtype='fp8')
    W = {k: v.cuda() for k, v in _ff_params(64, 170, torch.Generator().manual_seed(0)).items()}
    x = torch.zeros(2, 64, device='cuda')
    with pytest.raises(ValueError, match='arithmetic'):
        trunk_ops.feedforward(x, *W.values(), arith='fp8')
    # a bf16-mode call without its scratch bound is refused (no silent fp32, no overrun)
    lib = _lib.load()
    ws = torch.empty(lib.d4_ff_workspace_bytes(2, 64, 170) + 256, dtype=torch.uint8, device='cuda')
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    y = torch.empty_like(x)
    prev = lib.d4_train_arith_set(1)
    try:
        rc = lib.d4_ff_forward(_lib.ptr(x), *[_lib.ptr(v) for v in W.values()], 2, 64, 170, _lib.ptr(y), base, lib.d4_ff_workspace_bytes(2, 64, 170), stream())
    finally:
        lib.d4_train_arith_set(prev)
    assert rc != 0 and 'd4_train_scratch_bind' in lib.d4_last_error().decode()
    # ... and so is the other mismatch: a caller that bound its bf16 scratch but finds the switch at fp32 (never a silent fp32 result)
    sc = torch.empty(lib.d4_ff_bf16_scratch_bytes(2, 64, 170) + 256, dtype=torch.uint8, device='cuda')
    lib.d4_train_scratch_bind(sc.data_ptr() + (-sc.data_ptr()) % 256, sc.numel() - 256)
    try:
        assert lib.d4_train_arith_get() == 0
        rc = lib.d4_ff_forward(_lib.ptr(x), *[_lib.ptr(v) for v in W.values()], 2, 64, 170, _lib.ptr(y), base, lib.d4_ff_workspace_bytes(2, 64, 170), stream())
    finally:
        lib.d4_train_scratch_bind(None, 0)
    assert rc != 0 and 'arithmetic is fp32' in lib.d4_last_error().decode()
    # the dispatcher route does not carry the mode: it says so
    monkeypatch.setenv('D4_TRUNK_DISPATCHER', '1')
    with pytest.raises(NotImplementedError, match='bf16'):
        trunk_ops.feedforward(x, *W.values(), arith='bf16')
    from test_gpu_backward import _attn_params
    Wa = {k: v.cuda() for k, v in _attn_params(64, 2, 32, torch.Generator().manual_seed(0)).items()}
    with pytest.raises(NotImplementedError, match='bf16'):
        trunk_ops.space_attention(torch.zeros(2, 5, 64, device='cuda'), Wa['norm.weight'], Wa['to_q.weight'], Wa['to_k.weight'], Wa['to_v.weight'],
                                  Wa['to_out.weight'], Wa['to_gates.0.weight'], Wa['k_heads_rmsnorm.gamma'], arith='bf16')
