"""GPU: VideoTokenizer.forward with the latent SIGReg, orthogonality and consistency terms against tok_reg.npz, the fixture frozen from the reference
under its own recorded draws (tools/gen_tok_reg_golden.py; tests/test_tok_reg_host.py pins the float64 restatement to the same file).  Tolerances are
those of tests/test_gpu_tok_train.py: every loss term and the total within 1e-5, latents and the reconstructed video within 2e-4, every recorded
parameter gradient within 1e-3 of its scale, the normaliser states within 1e-4.  Both operator routes agree bit for bit, and a tokenizer with the
three weights at 0 is the tokenizer without the arguments, bit for bit."""
import pytest
import torch

import tok_reg_cases as RC
import tok_train_cases as TC
from dreamer4_amd.tokenizer import TokenizerLosses, VideoTokenizer

pytestmark = pytest.mark.gpu


def close(a, b, name, tol):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f'{name}: max abs diff {err:.3e} vs scale {scale:.3e}'


def mirror(kw, W, **extra):
    tok = VideoTokenizer(**kw, lpips_loss_weight=0., **extra)
    missing, unexpected = tok.load_state_dict(W, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return tok.cuda().train()


@pytest.fixture(scope='module')
def fix():
    return RC.fixture()


def set_states(tok, g, name):
    with torch.no_grad():
        for f, s in RC.norm_states(g, name, 'before').items():
            tok.get_buffer(RC.NORMALIZER_KEYS[f]).copy_(s)


def run_case(tok, kw, g, name):
    t = lambda k: torch.from_numpy(g[f'{name}_{k}'])
    video = t('video').cuda()
    tok.zero_grad(set_to_none=True)
    total, (losses, recon_video) = tok(video, return_intermediates=True, draws=RC.case_draws(g, name))
    assert isinstance(losses, TokenizerLosses)
    for f in losses._fields:
        if f in RC.TERMS:
            close(getattr(losses, f), t(f), f, RC.LOSS_TOL)
        else:
            assert float(getattr(losses, f)) == 0., f
    close(total, t('total'), 'total', RC.LOSS_TOL)
    close(recon_video, t('recon_video'), 'recon_video', RC.VALUE_TOL)
    with torch.no_grad():
        close(tok(video, return_latents=True, patch_mask=t('patch_mask')), t('latents'), 'latents', RC.VALUE_TOL)
    total.backward()
    grads, own = TC.case_grads(g, name), dict(tok.named_parameters())
    assert set(grads) == {k for k in own if TC.has_gradient(k, kw, 3)}, 'the fixture holds the complete set'
    for k, ref in grads.items():
        assert own[k].grad is not None, k
        close(own[k].grad, ref, 'd ' + k, RC.GRAD_TOL)
    return len(grads)


@pytest.mark.parametrize('name', ['reg', 'reg2'])
def test_three_terms_vs_reference_fixture(fix, name):
    kw, reg, W, g = fix
    tok = mirror(kw, W, **reg)
    set_states(tok, g, name)
    assert run_case(tok, kw, g, name) == 132
    for f, s in RC.norm_states(g, name, 'after').items():
        close(tok.get_buffer(RC.NORMALIZER_KEYS[f]), s, f + ' normaliser state', RC.STATE_TOL)


def test_three_terms_without_loss_normalisation(fix):
    kw, reg, W, g = fix
    tok = mirror(kw, W, use_loss_normalization=False, **reg)
    assert not any('loss_normalizer' in k for k, _ in tok.named_buffers())
    assert run_case(tok, kw, g, 'reg_nonorm') == 132


def test_second_call_carries_the_four_normaliser_states(fix):
    kw, reg, W, g = fix
    tok = mirror(kw, W, **reg)
    for name in ('reg', 'reg2'):                                       # the states are NOT reset in between
        for f, s in RC.norm_states(g, name, 'before').items():
            close(tok.get_buffer(RC.NORMALIZER_KEYS[f]), s, f'{f} state before {name}', RC.STATE_TOL)
        total = tok(torch.from_numpy(g[f'{name}_video']).cuda(), draws=RC.case_draws(g, name))
        close(total, g[f'{name}_total'], 'total of ' + name, RC.LOSS_TOL)
    before = {f: tok.get_buffer(k).clone() for f, k in RC.NORMALIZER_KEYS.items()}
    tok(torch.from_numpy(g['reg_video']).cuda(), draws=RC.case_draws(g, 'reg'), update_loss_ema=False)
    assert all(torch.equal(tok.get_buffer(k), before[f]) for f, k in RC.NORMALIZER_KEYS.items()), 'update_loss_ema=False leaves the states alone'


def test_each_term_alone_and_a_drawn_projection(fix):
    """One weight at a time: only that term is non-zero, and it is the recorded value (the terms do not depend on each other); without
    draws['sigreg_projs'] the projections come from the generator, reproducibly."""
    kw, reg, W, g = fix
    video, draws = torch.from_numpy(g['reg_nonorm_video']).cuda(), RC.case_draws(g, 'reg_nonorm')
    for f in RC.TERMS[1:]:
        extra = {f + '_loss_weight': 0.1}
        if f == 'latent_sigreg':
            extra['latent_sigreg_loss_kwargs'] = reg['latent_sigreg_loss_kwargs']
        tok = mirror(kw, W, use_loss_normalization=False, **extra)
        total, (losses, _) = tok(video, return_intermediates=True, draws=draws)
        close(getattr(losses, f), g[f'reg_nonorm_{f}'], f, RC.LOSS_TOL)
        assert all(float(getattr(losses, o)) == 0. for o in losses._fields if o not in ('recon', f)), f
        close(total, float(g['reg_nonorm_recon']) + 0.1 * float(g[f'reg_nonorm_{f}']), 'total with ' + f, RC.LOSS_TOL)
    tok = mirror(kw, W, use_loss_normalization=False, latent_sigreg_loss_weight=0.1)
    no_projs = {k: v for k, v in draws.items() if k != 'sigreg_projs'}
    a = tok(video, return_intermediates=True, draws=no_projs, generator=torch.Generator(device='cuda').manual_seed(5))[1].losses.latent_sigreg
    b = tok(video, return_intermediates=True, draws=no_projs, generator=torch.Generator(device='cuda').manual_seed(5))[1].losses.latent_sigreg
    c = tok(video, return_intermediates=True, draws=no_projs, generator=torch.Generator(device='cuda').manual_seed(6))[1].losses.latent_sigreg
    assert torch.equal(a, b) and not torch.equal(a, c) and a.item() > 0.


def test_both_operator_routes_agree_bit_for_bit(fix, monkeypatch):
    kw, reg, W, g = fix
    video = torch.from_numpy(g['reg_video']).cuda()
    got = []
    for route in ('0', '1'):
        monkeypatch.setenv('D4_TRUNK_DISPATCHER', route)
        tok = mirror(kw, W, **reg)
        total, (losses, _) = tok(video, return_intermediates=True, draws=RC.case_draws(g, 'reg'))
        total.backward()
        got.append([total, losses.latent_sigreg, losses.latent_ortho, losses.latent_consistency, tok.encoded_to_latents.weight.grad, tok.mask_token.grad,
                    tok.decoder.tokens_to_patch._modules['0'].weight.grad])
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_zero_weights_are_the_tokenizer_without_the_arguments(fix):
    kw, reg, W, _ = fix
    g = TC.fixture()[2]
    video, draws = torch.from_numpy(g['train_video']).cuda(), TC.case_draws(g, 'train')
    got = []
    for extra in ({}, dict(latent_sigreg_loss_weight=0., latent_sigreg_loss_kwargs=dict(num_slices=256), latent_ortho_loss_weight=0.,
                           latent_consistency_loss_weight=0.)):
        tok = mirror(kw, W, **extra)
        assert [k for k, _ in tok.named_buffers() if 'loss_normalizer' in k] == [RC.NORMALIZER_KEYS['recon']]
        total, (losses, recon_video) = tok(video, return_intermediates=True, draws=draws)
        total.backward()
        assert all(float(getattr(losses, f)) == 0. for f in losses._fields if f != 'recon')
        got.append((total, recon_video, {k: p.grad for k, p in tok.named_parameters() if p.grad is not None}))
    close(got[0][0], g['train_total'], 'the existing train case', TC.LOSS_TOL)
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and set(got[0][2]) == set(got[1][2])
    assert all(torch.equal(v, got[1][2][k]) for k, v in got[0][2].items())
