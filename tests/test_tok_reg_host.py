"""CPU: the yardsticks of the tokenizer's latent regularisers.  The float64 restatement of the training forward with the three terms
(tests/tok_reg_ref.py) reproduces the reference fixture tok_reg.npz under the recorded draws, terms, total, normaliser states and gradients; the
operator restatements agree with autograd, the SIGReg one also with the reference's complex formulation written out here; the recorded E32 of every
family is what the float32 evaluation measures here; the symbols are bound and declared, the dispatcher operators have fake implementations and no CPU
fallback; the constructor records the new arguments and leaves a default tokenizer as it was."""
import math
import os
import tempfile

import pytest
import torch

import tok_reg_cases as RC
import tok_reg_ref as R
import tok_train_cases as TC
import tok_train_ref as TR
from dreamer4_amd import _lib
from dreamer4_amd.tokenizer import VideoTokenizer


def close(a, b, name, tol):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f'{name}: max abs diff {err:.3e} vs scale {scale:.3e}'


# ----------------------------------------------------------------------------- the fixture
@pytest.fixture(scope='module')
def fix():
    return RC.fixture()


def _check_case(kw, reg, W, g, name, states):
    tc = TR.tokenizer_config(kw)
    Wd = TR.double_weights(W)
    weights = dict(latent_sigreg=reg['latent_sigreg_loss_weight'], latent_ortho=reg['latent_ortho_loss_weight'],
                   latent_consistency=reg['latent_consistency_loss_weight'])
    sk = {k: v for k, v in reg['latent_sigreg_loss_kwargs'].items() if k != 'num_slices'}
    out = R.training_forward(tc, Wd, torch.from_numpy(g[f'{name}_video']).double(), RC.case_draws(g, name), weights=weights, sigreg_kwargs=sk,
                             norm_states=states)
    out['total'].backward()
    for f in RC.TERMS:
        close(out[f], g[f'{name}_{f}'], f, RC.LOSS_TOL)
    close(out['total'], g[f'{name}_total'], 'total', RC.LOSS_TOL)
    close(out['latents'], g[f'{name}_latents'], 'latents', RC.VALUE_TOL)
    close(out['recon_video'], g[f'{name}_recon_video'], 'recon_video', RC.VALUE_TOL)
    grads = TC.case_grads(g, name)
    params = [k for k, v in W.items() if v.is_floating_point() and 'inv_freq' not in k]
    assert set(grads) == {k for k in params if TC.has_gradient(k, kw, 3)}, 'the fixture holds every gradient'
    for k, ref in grads.items():
        close(Wd[k].grad, ref, 'd ' + k, RC.GRAD_TOL)
    return len(grads)


def test_restatement_reproduces_the_fixture(fix):
    kw, reg, W, g = fix
    assert g['reg_sigreg_projs'].shape == (256, kw['dim_latent']) and g['reg_video'].shape == (2, 3, 3, 16, 24)
    states = {f: torch.ones(1, dtype=torch.float64) for f in RC.TERMS}
    for name in ('reg', 'reg2'):                                        # the second call carries the first one's four states
        for f in RC.TERMS:
            close(states[f], g[f'{name}_norm_before/{f}'], f'{f} state before {name}', RC.STATE_TOL)
        assert _check_case(kw, reg, W, g, name, states) == 132
        for f in RC.TERMS:
            close(states[f], g[f'{name}_norm_after/{f}'], f'{f} state after {name}', RC.STATE_TOL)
    assert _check_case(kw, reg, W, g, 'reg_nonorm', None) == 132
    for name in RC.REG_CASES:
        assert g[f'{name}_time_indices'].any() and all(float(g[f'{name}_{f}']) > 0. for f in RC.TERMS), name
    for f in os.listdir(TC.GOLDEN):
        if f.startswith('tok_reg'):
            assert os.path.getsize(os.path.join(TC.GOLDEN, f)) < (1 << 20), f


# ----------------------------------------------------------------------------- operator restatements
def complex_sigreg(x, projs, lo, hi, num_knots):
    """The reference's formulation from the mathematics: ecf = mean_n exp(i t <x_n, u_m>), err = |ecf - phi|^2 phi, trapezoid, mean"""
    u = projs / projs.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    t = torch.linspace(lo, hi, num_knots, dtype=x.dtype)
    phi = (-0.5 * t.square()).exp()
    x_t = torch.einsum('knd,md->knm', x.reshape(x.shape[0], -1, x.shape[-1]), u)[..., None] * t
    ecf = torch.exp(1j * x_t).mean(dim=1)
    return torch.trapz((ecf - phi).abs().square() * phi, t, dim=-1).mean()


def test_sigreg_restatement_agrees_with_the_complex_formulation_and_autograd():
    for c in RC.SIGREG_CASES:
        if c['N'] * c['M'] > 80000:
            continue
        d = RC.sigreg_inputs(c)
        x, p = d['x'].double().requires_grad_(), d['projs'].double()
        loss = complex_sigreg(x, p, c['lo'], c['hi'], c['knots'])
        loss.backward()
        l, dx = R.sigreg_ref(d['x'], d['projs'], c['lo'], c['hi'], c['knots'])
        close(l, loss, c['name'] + ' loss', 1e-12); close(dx, x.grad, c['name'] + ' dx', 1e-11)
        close(R.sigreg_loss(d['x'].double(), p, c['lo'], c['hi'], c['knots']), loss, c['name'] + ' differentiable form', 1e-12)


def test_one_row_has_a_closed_form():
    """N = 1: |exp(i t p) - phi|^2 = 1 - 2 phi cos(t p) + phi^2"""
    c = RC.SIGREG_CASES[0]
    assert (c['K'], c['N'], c['M']) == (1, 1, 1)
    d = RC.sigreg_inputs(c)
    x, u = d['x'].double()[0, 0], d['projs'].double()[0]
    p = float(x @ (u / u.norm()))
    t = torch.linspace(c['lo'], c['hi'], c['knots'], dtype=torch.float64)
    phi = (-0.5 * t.square()).exp()
    want = torch.trapz((1. - 2. * phi * (t * p).cos() + phi.square()) * phi, t)
    close(R.sigreg_ref(d['x'], d['projs'], c['lo'], c['hi'], c['knots'])[0], want, 'closed form', 1e-12)


def test_ortho_restatement_agrees_with_autograd_and_the_special_frames():
    for c in RC.ORTHO_CASES:
        d = RC.ortho_inputs(c)
        x = d['x'].double().requires_grad_()
        loss = R.ortho_loss(x)
        l, dx = R.latent_ortho_ref(d['x'])
        close(l, loss, c['name'] + ' loss', 1e-12)
        if c['name'] in RC.EXACT_ZERO:
            for dt in (torch.float32, torch.float64):
                l, dx = R.latent_ortho_ref(d['x'], dtype=dt)
                assert l.item() == 0. and not dx.any() and torch.isfinite(dx).all(), c['name']
        else:
            loss.backward()
            close(dx, x.grad, c['name'] + ' dx', 1e-8)
    d = RC.ortho_inputs(next(c for c in RC.ORTHO_CASES if c['kind'] == 'orthonormal'))
    y = d['x'].double()
    y = y / y.norm(dim=-1, keepdim=True)
    G = (y @ y.transpose(-1, -2)).masked_fill(torch.eye(4, dtype=torch.bool), 0.)
    assert 1e-7 < G.square().sum(dim=(-1, -2)).max().item() < 1e-4, 'the rows themselves are orthonormal to the noise'
    assert R.latent_ortho_ref(d['x'])[0].item() >= 4. / 3. - 1e-9, 'centred rows are not: the loss is at least n / (n - 1)'


def measured_e32():
    worst = {f: 0. for f in RC.E32}
    for c in RC.SIGREG_CASES:
        d = RC.sigreg_inputs(c)
        a = R.sigreg_ref(d['x'], d['projs'], c['lo'], c['hi'], c['knots'], dtype=torch.float32)
        b = R.sigreg_ref(d['x'], d['projs'], c['lo'], c['hi'], c['knots'])
        worst[c['family']] = max(worst[c['family']], TC.rel_err(a[0].reshape(1), b[0].reshape(1)), TC.rel_err(a[1], b[1]))
    for c in RC.ORTHO_CASES:
        if c['name'] in RC.EXACT_ZERO:
            continue
        d = RC.ortho_inputs(c)
        a, b = R.latent_ortho_ref(d['x'], dtype=torch.float32), R.latent_ortho_ref(d['x'])
        worst[c['family']] = max(worst[c['family']], TC.rel_err(a[0].reshape(1), b[0].reshape(1)))
        if c['name'] == RC.ZERO_GRADIENT:                              # true gradient 0: the absolute bound, which the float32 evaluation meets too
            assert not b[1].abs().max().item() > 1e-13 and a[1].abs().max().item() <= RC.two_rows_grad_bound(d['x'])
        else:
            worst[c['grad_family']] = max(worst[c['grad_family']], TC.rel_err(a[1], b[1]))
    return worst


def test_recorded_e32_is_the_measured_float32_error_with_a_quarter_of_headroom():
    worst = measured_e32()
    for f, e in worst.items():
        print(f'{f}: measured E32 {e:.3e}, recorded {RC.E32[f]:.3e}, GPU bound {RC.BOUND[f]:.3e}')
    for f, e in worst.items():
        assert e <= RC.E32[f] <= 1.3 * e, (f, e, RC.E32[f])


def test_the_bounds_see_a_dropped_row_and_a_wrong_knot():
    c = RC.SIGREG_CASES[2]
    d = RC.sigreg_inputs(c)
    good = R.sigreg_ref(d['x'], d['projs'], c['lo'], c['hi'], c['knots'])
    short = R.sigreg_ref(d['x'][:, :-1], d['projs'], c['lo'], c['hi'], c['knots'])
    assert TC.rel_err(short[0].reshape(1), good[0].reshape(1)) > 10 * RC.BOUND['sigreg']
    moved = R.sigreg_ref(d['x'], d['projs'], c['lo'], c['hi'] * (1. + 1e-2), c['knots'])
    assert TC.rel_err(moved[1], good[1]) > 10 * RC.BOUND['sigreg']
    c = RC.ORTHO_CASES[3]
    d = RC.ortho_inputs(c)
    good, short = R.latent_ortho_ref(d['x']), R.latent_ortho_ref(d['x'][:, :-1])
    assert TC.rel_err(short[0].reshape(1), good[0].reshape(1)) > 100 * RC.BOUND['ortho_loss']
    for c in RC.ORTHO_CASES:                                           # a gradient 1 % too long, or without the centring's backward, is outside every case's bound
        if c['name'] in RC.EXACT_ZERO or c['name'] == RC.ZERO_GRADIENT:
            continue
        x = RC.ortho_inputs(c)['x']
        dx = R.latent_ortho_ref(x)[1]
        assert TC.rel_err(dx * 1.01, dx) > 10 * RC.BOUND[c['grad_family']], c['name']
        xd = x.double().requires_grad_()
        y = R.unit_rows(xd - xd.mean(dim=-2, keepdim=True).detach())
        G = (y @ y.transpose(-1, -2)).masked_fill(torch.eye(c['n'], dtype=torch.bool), 0.)
        G.square().sum(dim=(-1, -2)).mean().backward()
        assert TC.rel_err(xd.grad, dx) > 10 * RC.BOUND[c['grad_family']], c['name']


def test_case_tables_cover_what_they_should():
    sig = {c['name']: c for c in RC.SIGREG_CASES}
    assert [(c['K'], c['N'], c['d'], c['M']) for c in RC.SIGREG_CASES[:6]] == [(1, 1, 4, 1), (2, 77, 8, 64), (2, 300, 32, 256), (1, 40, 6, 5), (1, 16, 64, 1024),
                                                                             (1, 16, 128, 64)]
    assert sig['row_blocks']['N'] > RC.ROWS_PER_BLOCK and sig['ragged']['N'] % RC.ROWS_PER_BLOCK and sig['odd_dim']['d'] % 4 and sig['odd_dim']['M'] < 64
    assert sig['dim_128']['d'] == RC.MAX_DIM and sig['knots_2']['knots'] == 2 and sig['knots_16']['knots'] == 16
    assert 0. not in torch.linspace(-5., 5., 16).tolist() and (sig['asymmetric']['lo'], sig['asymmetric']['hi'], sig['asymmetric']['knots']) == (0., 3., 4)
    d = RC.sigreg_inputs(sig['scaled_20'])
    assert (d['x'] @ (d['projs'] / d['projs'].norm(dim=-1, keepdim=True)).t()).abs().max().item() * 5. > 200., 'angles of hundreds of radians'
    assert (sig['floor']['K'], sig['floor']['N'], sig['floor']['d'], sig['floor']['M']) == (1, 2048, 8, 16)
    assert [(c['F'], c['n'], c['d']) for c in RC.ORTHO_CASES] == [(3, 1, 8), (2, 2, 4), (6, 6, 8), (2, 64, 16), (1, 65, 32), (1, 256, 8), (1, 130, 128), (2, 4, 16),
                                                                   (1, 8, 16)]
    assert {c['name'] for c in RC.ORTHO_CASES} >= set(RC.EXACT_ZERO)
    assert [c['d'] for c in RC.REFUSED_SIGREG][0] == RC.MAX_DIM + 1 and RC.REFUSED_SIGREG[1]['knots'] == 1 and RC.REFUSED_SIGREG[2]['M'] == RC.MAX_SLICES + 1
    assert RC.REFUSED_ORTHO[0]['d'] == RC.MAX_DIM + 1 and RC.REFUSED_ORTHO[1]['n'] == RC.ORTHO_MAX_ROWS + 1
    names = [c['name'] for c in RC.SIGREG_CASES + RC.ORTHO_CASES]
    assert len(names) == len(set(names))


def test_workspace_does_not_scale_with_rows_times_slices():
    """d4_sigreg_part_floats stays below K M knots 2 (blocks of rows + 1): the partial sums of the characteristic function and what the final
    reduction needs, nothing per (row, slice).  The query is host code of libd4hip."""
    lib = _lib.load()
    for K_, N, M, T in [(c['K'], c['N'], c['M'], c['knots']) for c in RC.SIGREG_CASES] + [(32, 1024, 256, 17), (1, 1, 1, 2), (3, 65, 4096, 64)]:
        n = lib.d4_sigreg_part_floats(K_, N, M, T)
        blocks = -(-N // RC.ROWS_PER_BLOCK)
        assert n == RC.sigreg_part_floats(K_, N, M, T) and 0 < n < K_ * M * T * 2 * (blocks + 1), (K_, N, M, T, n)
    assert lib.d4_sigreg_part_floats(32, 1024, 256, 17) < 32 * 1024 * 256, 'far below one float per (row, slice)'
    assert lib.d4_latent_ortho_part_floats(7) == 7


# ----------------------------------------------------------------------------- bindings
NEW_SYMBOLS = ('d4_sigreg_part_floats', 'd4_sigreg_fwd_bwd', 'd4_latent_ortho_part_floats', 'd4_latent_ortho_fwd_bwd')


def test_new_symbols_are_bound_and_declared():
    header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'd4hip.h')).read()
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS and s + '(' in header and hasattr(lib, s), s
    import dreamer4_amd.ops  # noqa: F401
    assert hasattr(torch.ops.d4hip, 'sigreg') and hasattr(torch.ops.d4hip, 'latent_ortho')


def test_operators_have_fake_implementations_and_no_cpu_fallback():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import dreamer4_amd.ops  # noqa: F401
    from dreamer4_amd import trunk_ops
    with FakeTensorMode():
        x = torch.empty(2, 3, 6, 8)
        loss, dx = torch.ops.d4hip.sigreg(x, torch.empty(256, 8), -5., 5., 17)
        assert loss.shape == () and dx.shape == x.shape and dx.dtype == torch.float32
        loss, dx = torch.ops.d4hip.latent_ortho(x)
        assert loss.shape == () and dx.shape == x.shape
    x = torch.zeros(1, 4, 8)
    for call in (lambda: torch.ops.d4hip.sigreg(x, torch.ones(4, 8), -5., 5., 17), lambda: torch.ops.d4hip.latent_ortho(x),
                 lambda: trunk_ops.sigreg(x, torch.ones(4, 8)), lambda: trunk_ops.latent_ortho(x)):
        with pytest.raises(_lib.D4Error, match='no CPU fallback'):
            call()


# ----------------------------------------------------------------------------- constructor
KW = dict(dim=32, dim_latent=8, patch_size=4, image_height=16, image_width=24, num_latent_tokens=6, encoder_depth=1, decoder_depth=1, attn_heads=2)
KEYS = RC.NORMALIZER_KEYS


def test_defaults_are_the_references_and_change_nothing():
    plain = VideoTokenizer(**KW)
    cfg = plain._config[1]
    assert cfg['latent_sigreg_loss_weight'] == 0. and cfg['latent_ortho_loss_weight'] == 0. and cfg['latent_consistency_loss_weight'] == 0.
    assert cfg['latent_sigreg_loss_kwargs'] == dict(num_slices=256)
    assert [k for k, _ in plain.named_buffers() if 'loss_normalizer' in k] == [KEYS['recon']]
    assert not any('loss_normalizer' in k for k in plain.state_dict())
    torch.manual_seed(0); a = VideoTokenizer(**KW)
    torch.manual_seed(0); b = VideoTokenizer(**KW, latent_sigreg_loss_weight=0.3, latent_ortho_loss_weight=0.2, latent_consistency_loss_weight=0.1)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), 'the state_dict does not know about the regularisers'


def test_normaliser_state_exists_only_for_a_positive_weight():
    for f in ('latent_sigreg', 'latent_ortho', 'latent_consistency'):
        tok = VideoTokenizer(**KW, **{f + '_loss_weight': 0.1})
        bufs = dict(tok.named_buffers())
        assert {k for k in bufs if 'loss_normalizer' in k} == {KEYS['recon'], KEYS[f]}, f
        assert bufs[KEYS[f]].shape == (1,) and bufs[KEYS[f]].item() == 1.
        assert not any('loss_normalizer' in k for k in tok.state_dict()), 'not persistent'
        assert not any('loss_normalizer' in k for mode in (1, 2) for k in tok._engine_tensors(mode))
        assert getattr(tok, f + '_loss_weight') == 0.1
    tok = VideoTokenizer(**KW, latent_ortho_loss_weight=0.1, use_loss_normalization=False)
    assert not any('loss_normalizer' in k for k, _ in tok.named_buffers())


def test_a_reference_checkpoints_normaliser_keys_are_accepted():
    tok = VideoTokenizer(**KW, latent_sigreg_loss_weight=0.1, latent_ortho_loss_weight=0.1, latent_consistency_loss_weight=0.1)
    sd = tok.state_dict()
    for i, f in enumerate(RC.TERMS):
        sd[KEYS[f]] = torch.tensor([2. + i])
    tok.load_state_dict(sd)
    for i, f in enumerate(RC.TERMS):
        assert tok.get_buffer(KEYS[f]).item() == 2. + i, f
    plain = VideoTokenizer(**KW)                                      # trains without the terms: their state is dropped, not refused
    plain.load_state_dict(sd)
    assert plain.get_buffer(KEYS['recon']).item() == 2.


def test_config_round_trip_through_a_checkpoint():
    kwargs = dict(latent_sigreg_loss_weight=0.25, latent_sigreg_loss_kwargs=dict(num_slices=64, domain=(-4., 4.), num_knots=9), latent_ortho_loss_weight=0.5,
                  latent_consistency_loss_weight=0.125)
    tok = VideoTokenizer(**KW, **kwargs)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'tok.pt')
        tok.save(path)
        back = VideoTokenizer.init_and_load(path)
    for k, v in kwargs.items():
        assert back._config[1][k] == v, k
    assert back.loss_weights == dict(latent_sigreg=0.25, latent_ortho=0.5, latent_consistency=0.125) and back.latent_sigreg_loss_kwargs == kwargs['latent_sigreg_loss_kwargs']
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in tok.state_dict().items())


def test_what_stays_outside_the_subset_is_still_refused():
    with pytest.raises(NotImplementedError):
        VideoTokenizer(**KW, latent_sigreg_loss_kwargs=dict(mask=None))
    for kw in (dict(latent_ar_loss_weight=0.1), dict(latent_ar_sigreg_loss_weight=0.1), dict(encoder_add_decorr_aux_loss=True), dict(has_byol=True)):
        with pytest.raises(NotImplementedError):
            VideoTokenizer(**KW, **kw)
    tok = VideoTokenizer(**KW, lpips_loss_weight=0., latent_ortho_loss_weight=0.1)
    with pytest.raises(NotImplementedError, match='time_lens'):
        tok(torch.zeros(1, 3, 2, 16, 24), time_lens=torch.tensor([2]))
    with pytest.raises(_lib.D4Error, match='no CPU fallback'):
        tok(torch.zeros(1, 3, 2, 16, 24))
    assert math.isclose(tok.latent_ortho_loss_weight, 0.1)
