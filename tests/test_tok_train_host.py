"""CPU: the yardsticks of the tokenizer's training forward.  The float64 restatement (tests/tok_train_ref.py, composed from oracle/restate.py)
reproduces both reference fixtures, losses and gradients, under the recorded draws; the operator references agree with autograd; the recorded E32
of every numeric family is what the float32 evaluation measures here; the case tables respect the launchers' size rules; the new symbols are bound;
the constructor and `forward` refuse what is outside the subset."""
import os

import pytest
import torch

import tok_train_cases as TC
import tok_train_ref as R
from dreamer4_amd import _lib
from dreamer4_amd.tokenizer import TokenizerLosses, VideoTokenizer
from oracle import restate


def close(a, b, name, tol):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f'{name}: max abs diff {err:.3e} vs scale {scale:.3e}'


@pytest.fixture(scope='module')
def narrow():
    return TC.fixture()


def _restated_case(kw, W, g, name, norm_state, **opts):
    tc = R.tokenizer_config(kw)
    Wd = R.double_weights(W)
    video = torch.from_numpy(g[f'{name}_video']).double()
    if video.ndim == 4:
        video = video.unsqueeze(2)
    out = R.training_forward(tc, Wd, video, TC.case_draws(g, name), norm_state=norm_state, **opts)
    out['total'].backward()
    return out, Wd


def _check_case(kw, W, g, name, norm_state, **opts):
    out, Wd = _restated_case(kw, W, g, name, norm_state, **opts)
    close(out['recon'], g[f'{name}_recon'], 'recon', TC.LOSS_TOL); close(out['total'], g[f'{name}_total'], 'total', TC.LOSS_TOL)
    close(out['latents'], g[f'{name}_latents'], 'latents', TC.VALUE_TOL)
    rv = out['recon_video'].squeeze(2) if g[f'{name}_video'].ndim == 4 else out['recon_video']
    close(rv, g[f'{name}_recon_video'], 'recon_video', TC.VALUE_TOL)
    grads = TC.case_grads(g, name)
    frames = 1 if g[f'{name}_video'].ndim == 4 else g[f'{name}_video'].shape[2]
    params = [k for k, v in W.items() if v.is_floating_point() and 'inv_freq' not in k]
    assert set(grads) == {k for k in params if TC.has_gradient(k, kw, frames)}, 'the fixture holds every gradient'
    for k, ref in grads.items():
        close(Wd[k].grad, ref, 'd ' + k, TC.GRAD_TOL)
    gmax = max(v.abs().max().item() for v in grads.values())
    for k in params:
        if frames == 1 and TC.time_attention(k, kw):
            assert Wd[k].grad.abs().max().item() <= TC.NOISE_FLOOR * gmax, k
    return len(grads)


def test_restatement_reproduces_the_narrow_fixture(narrow):
    kw, W, g = narrow
    state = torch.ones(1, dtype=torch.float64)
    for name in ('train', 'train2'):                                  # the second call carries the first one's normaliser state
        close(state, g[f'{name}_norm_before'], 'state before ' + name, TC.STATE_TOL)
        assert _check_case(kw, W, g, name, state) == 132
        close(state, g[f'{name}_norm_after'], 'state after ' + name, TC.STATE_TOL)
    _check_case(kw, W, g, 'nonorm', None)
    _check_case(kw, W, g, 'xspace', torch.from_numpy(g['xspace_norm_before']).double(), v_space=False)
    assert _check_case(kw, W, g, 'image', torch.from_numpy(g['image_norm_before']).double()) == 114   # but the 18 of the two time layers' attention blocks
    lat = R.encoder_latents(R.tokenizer_config(kw), {k: v.double() for k, v in W.items()}, torch.from_numpy(g['latents_video']).double(),
                            torch.from_numpy(g['latents_patch_mask']))
    close(lat, g['latents_latents'], 'latents under a given patch mask', TC.VALUE_TOL)


def test_restatement_reproduces_the_wide_fixture():
    kw, W, g = TC.fixture(wide=True)
    assert kw['image_height'] // kw['patch_size'] * (kw['image_width'] // kw['patch_size']) + kw['num_latent_tokens'] == 85
    assert _check_case(kw, W, g, 'train', torch.ones(1, dtype=torch.float64)) == 132


def test_fixture_draws_exercise_what_they_should(narrow):
    for g, names in ((narrow[2], TC.NARROW_CASES), (TC.fixture(wide=True)[2], ('train',))):
        for name in names:
            assert g[f'{name}_time_indices'].any(), name
            pm = torch.from_numpy(g[f'{name}_patch_mask']).flatten(2)
            assert pm.any()
            if pm.shape[1] > 1:
                assert (~pm.any(-1)).any(1).all() and (pm.float().mean(-1) >= 0.5).any(1).all(), name
    for f in os.listdir(TC.GOLDEN):
        if 'tok_train' in f:
            assert os.path.getsize(os.path.join(TC.GOLDEN, f)) < (1 << 20), f


# ----------------------------------------------------------------------------- operator references
def test_operator_references_agree_with_autograd():
    c = TC.LN_CASES[3]
    d = TC.ln_inputs(c)
    x, gm = d['x'].double().requires_grad_(), d['g'].double().requires_grad_()
    restate.layernorm(x, gm, 0., TC.LN_EPS).backward(d['dy'].double())
    dx, dg = R.layernorm_rows_bwd_ref(d['x'], d['dy'], d['g'], TC.LN_EPS)
    close(dx, x.grad, 'dx', 1e-12); close(dg, gm.grad, 'dg', 1e-12)
    for c in TC.LOSS_CASES[:2] + TC.LOSS_CASES[-2:]:
        d = TC.geom_inputs(c)
        rows = d['recon_rows'].double().requires_grad_()
        v, n = d['video'].double(), d['noise'].double()
        tt = d['times'].double()[:, None, None, None, None]
        rv = R.rows_to_video(rows, c['C'], c['ps'])
        assert torch.equal(R.patch_rows(rv, c['ps']), rows), 'the two permutations are inverses'
        noised = torch.lerp(n, v, tt)
        loss = (((rv - noised) / (1. - tt) - (v - n)) if c['v_space'] else (rv - v)).pow(2).mean()
        loss.backward()
        l, dr = R.recon_loss_ref(d['recon_rows'], d['video'], d['noise'], d['times'], c['ps'], c['v_space'])
        close(l, loss, 'loss', 1e-12); close(dr, rows.grad, 'd rows', 1e-12)
    d = TC.mask_inputs(TC.MASK_CASES[2])
    x, tok = d['x'].double().requires_grad_(), d['token'].double().requires_grad_()
    R.mask_rows_fwd_ref(x, d['mask'], tok).backward(d['dy'].double())
    dx, dt = R.mask_rows_bwd_ref(d['dy'], d['mask'])
    close(dx, x.grad, 'dx', 0.); close(dt, tok.grad, 'd token', 1e-12)
    d = TC.geom_inputs(TC.FLOW_CASES[0])
    assert torch.equal(R.flow_noised_patches_ref(d['video'], d['noise'], torch.ones(2), 4, dtype=torch.float32), R.patch_rows(d['video'], 4)), 't = 1: the video itself'
    assert torch.equal(R.flow_noised_patches_ref(d['video'], d['noise'], torch.zeros(2), 4, dtype=torch.float32), R.patch_rows(d['noise'], 4)), 't = 0: the noise itself'


def measured_e32():
    worst = {f: 0. for f in TC.E32}
    up = lambda f, *pairs: worst.__setitem__(f, max(worst[f], *[TC.rel_err(a, b) for a, b in pairs]))
    f32 = torch.float32
    for c in TC.FLOW_CASES:
        d = TC.geom_inputs(c)
        up('flow_noised_patches', (R.flow_noised_patches_ref(d['video'], d['noise'], d['times'], c['ps'], dtype=f32),
                                   R.flow_noised_patches_ref(d['video'], d['noise'], d['times'], c['ps'])))
    for c in TC.LN_CASES:
        d = TC.ln_inputs(c)
        a, b = R.layernorm_rows_bwd_ref(d['x'], d['dy'], d['g'], TC.LN_EPS, dtype=f32), R.layernorm_rows_bwd_ref(d['x'], d['dy'], d['g'], TC.LN_EPS)
        up('layernorm_rows_bwd', *zip(a, b))
    for c in TC.MASK_CASES:
        d = TC.mask_inputs(c)
        if d['mask'].any():
            up('mask_rows_bwd', (R.mask_rows_bwd_ref(d['dy'], d['mask'], dtype=f32)[1], R.mask_rows_bwd_ref(d['dy'], d['mask'])[1]))
    for c in TC.LOSS_CASES:
        d = TC.geom_inputs(c)
        a = R.recon_loss_ref(d['recon_rows'], d['video'], d['noise'], d['times'], c['ps'], c['v_space'], dtype=f32)
        b = R.recon_loss_ref(d['recon_rows'], d['video'], d['noise'], d['times'], c['ps'], c['v_space'])
        up('recon_loss', (a[0].reshape(1), b[0].reshape(1)), (a[1], b[1]))
    return worst


def test_recorded_e32_is_the_measured_float32_error_with_a_quarter_of_headroom():
    worst = measured_e32()
    for f, e in worst.items():
        print(f'{f}: measured E32 {e:.3e}, recorded {TC.E32[f]:.3e}, GPU bound {TC.BOUND[f]:.3e}')
    for f, e in worst.items():
        assert e <= TC.E32[f] <= 1.3 * e, (f, e, TC.E32[f])


def test_the_bounds_see_a_dropped_row_and_a_wrong_time():
    """What the GPU bound must be able to see: a row missing from a column sum, a clip read with its neighbour's time."""
    d = TC.ln_inputs(TC.LN_CASES[2])
    dg = R.layernorm_rows_bwd_ref(d['x'], d['dy'], d['g'], TC.LN_EPS)[1]
    dg_short = R.layernorm_rows_bwd_ref(d['x'][:-1], d['dy'][:-1], d['g'], TC.LN_EPS)[1]
    assert TC.rel_err(dg_short, dg) > 100 * TC.BOUND['layernorm_rows_bwd']
    c = TC.LOSS_CASES[0]
    d = TC.geom_inputs(c)
    good = R.recon_loss_ref(d['recon_rows'], d['video'], d['noise'], d['times'], c['ps'], 1)
    bad = R.recon_loss_ref(d['recon_rows'], d['video'], d['noise'], d['times'].flip(0), c['ps'], 1)
    assert TC.rel_err(bad[1], good[1]) > 100 * TC.BOUND['recon_loss']
    assert TC.rel_err(R.flow_noised_patches_ref(d['video'], d['noise'], d['times'].flip(0), c['ps']),
                      R.flow_noised_patches_ref(d['video'], d['noise'], d['times'], c['ps'])) > 100 * TC.BOUND['flow_noised_patches']


def test_case_tables_respect_the_launchers_size_rules():
    for c in TC.FLOW_CASES + TC.LOSS_CASES:
        assert (c['C'] * c['ps'] ** 2) % 4 == 0 and c['B'] == len(c['times']) and all(0. <= t < 1. for t in c['times']), c['name']
    assert {(c['ps'], c['C']) for c in TC.FLOW_CASES} == {(4, 3), (2, 1)} and {c['T'] for c in TC.FLOW_CASES} == {1, 3}
    assert {(c['nh'], c['nw']) for c in TC.LOSS_CASES} == {(4, 6), (1, 1)} and {c['v_space'] for c in TC.LOSS_CASES} == {0, 1}
    assert any(0. in c['times'] and len(set(c['times'])) > 1 for c in TC.FLOW_CASES)
    for c in TC.REFUSED_GEOMS:
        assert (c['C'] * c['ps'] ** 2) % 4 != 0
    for c in TC.LN_CASES + TC.MASK_CASES:
        assert c['rows'] >= 1 and c['D'] % 4 == 0 and 4 <= c['D'] <= TC.MAX_DIM and c.get('pad', 0) % 4 == 0, c['name']
    assert {c['D'] for c in TC.LN_CASES} == {32, 96} and {1, 144} <= {c['rows'] for c in TC.LN_CASES}
    assert any(c['rows'] % TC.ROW_TILE for c in TC.LN_CASES if c['rows'] > TC.ROW_TILE) and any(c['rows'] > TC.ROW_TILE for c in TC.MASK_CASES)
    assert {c['kind'] for c in TC.MASK_CASES} == {'none', 'all', 'mixed'}
    assert TC.part_floats(1, 32) == 32 and TC.part_floats(144, 96) == 18 * 96 and TC.part_floats(77, 4) == 10 * 4
    names = [c['name'] for t in (TC.FLOW_CASES, TC.LOSS_CASES, TC.LN_CASES, TC.MASK_CASES) for c in t]
    assert len(names) == len(set(names))


NEW_SYMBOLS = ('d4_flow_noised_patches', 'd4_tok_rows_part_floats', 'd4_layernorm_rows_bwd', 'd4_mask_rows_fwd', 'd4_mask_rows_bwd', 'd4_recon_loss_fwd_bwd')


def test_new_symbols_are_bound_and_declared():
    header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'd4hip.h')).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS and s + '(' in header, s
    for op in ('video_to_patches', 'patches_to_video', 'flow_noised_patches', 'layernorm_nobias', 'mask_rows', 'recon_loss'):
        import dreamer4_amd.ops  # noqa: F401
        assert hasattr(torch.ops.d4hip, op), op


def test_operators_have_fake_implementations_and_no_cpu_fallback():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        v = torch.empty(2, 3, 3, 16, 24)
        rows = torch.ops.d4hip.flow_noised_patches(v, v, torch.empty(2), 4)
        assert rows.shape == (2, 3, 4, 6, 48) and torch.ops.d4hip.video_to_patches(v, 4).shape == rows.shape
        assert torch.ops.d4hip.patches_to_video(rows, 3, 4).shape == v.shape
        x = torch.empty(5, 7, 32)
        assert torch.ops.d4hip.layernorm_nobias(x, torch.empty(32), 1e-5).shape == x.shape
        assert torch.ops.d4hip.mask_rows(x, torch.empty(5, 7, dtype=torch.bool), torch.empty(32)).shape == x.shape
        loss, d_rows = torch.ops.d4hip.recon_loss(rows, v, v, torch.empty(2), 4, True)
        assert loss.shape == () and d_rows.shape == rows.shape
    v = torch.zeros(1, 1, 1, 4, 4)
    for call in (lambda: torch.ops.d4hip.flow_noised_patches(v, v, torch.zeros(1), 2), lambda: torch.ops.d4hip.video_to_patches(v, 2),
                 lambda: torch.ops.d4hip.layernorm_nobias(torch.zeros(2, 8), torch.ones(8), 1e-5),
                 lambda: torch.ops.d4hip.mask_rows(torch.zeros(2, 8), torch.zeros(2, dtype=torch.bool), torch.ones(8)),
                 lambda: torch.ops.d4hip.recon_loss(torch.zeros(1, 1, 2, 2, 4), v, v, torch.zeros(1), 2, True)):
        with pytest.raises(_lib.D4Error, match='no CPU fallback'):
            call()


# ----------------------------------------------------------------------------- constructor and arguments
KW = dict(dim=32, dim_latent=8, patch_size=4, image_height=16, image_width=24, num_latent_tokens=6, encoder_depth=1, decoder_depth=1, attn_heads=2)


def test_constructor_records_the_new_arguments_and_keeps_the_state_dict():
    tok = VideoTokenizer(**KW, train_wide_frames=True, lpips_loss_weight=0., decoder_v_space_loss=False)
    cfg = tok._config[1]
    assert cfg['train_wide_frames'] is True and cfg['lpips_loss_weight'] == 0. and cfg['decoder_v_space_loss'] is False
    assert tok.train_wide_frames and not tok.decoder_v_space_loss and tok.use_loss_normalization
    plain = VideoTokenizer(**KW)
    assert plain.lpips_loss_weight == 0.2 and not plain.train_wide_frames and plain.decoder_v_space_loss, 'the reference defaults; any lpips weight constructs'
    sd = plain.state_dict()
    assert not any('loss_normalizer' in k for k in sd), 'the running mean square is not persistent'
    assert 'recon_loss_normalizer.exp_avg_sq' in dict(plain.named_buffers())
    assert not any('loss_normalizer' in k for mode in (1, 2) for k in plain._engine_tensors(mode))
    # a reference checkpoint carries the key: it is taken, not refused
    sd['recon_loss_normalizer.exp_avg_sq'] = torch.tensor([2.5])
    plain.load_state_dict(sd)
    assert plain.recon_loss_normalizer.exp_avg_sq.item() == 2.5
    assert not hasattr(VideoTokenizer(**KW, use_loss_normalization=False), 'recon_loss_normalizer')
    with pytest.raises(NotImplementedError):
        VideoTokenizer(**KW, separate_flow_decoder=True)
    with pytest.raises(NotImplementedError):
        VideoTokenizer(**KW, latent_receive_grad_frac=0.5)
    assert TokenizerLosses._fields == ('recon', 'flow_recon', 'lpips', 'time_decorr', 'space_decorr', 'latent_ortho', 'latent_ar', 'latent_ar_sigreg',
                                       'latent_consistency', 'latent_sigreg', 'h_net', 'byol')


def test_forward_refuses_what_is_outside_the_subset():
    video = torch.zeros(1, 3, 2, 16, 24)
    with pytest.raises(NotImplementedError, match='lpips_loss_weight'):
        VideoTokenizer(**KW, lpips_loss_weight=0.2)(video)
    tok = VideoTokenizer(**KW, lpips_loss_weight=0.)
    for kw in (dict(time_lens=torch.tensor([2])), dict(time_cache=(None,) * 4), dict(return_time_cache=True), dict(aug_id=1),
               dict(byol_target_latents=torch.zeros(1, 2, 6, 8))):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            tok(video, **kw)
    with pytest.raises(_lib.D4Error, match='no CPU fallback'):
        tok(video)
    with pytest.raises(_lib.D4Error, match='no CPU fallback'):
        tok(video, return_latents=True)
