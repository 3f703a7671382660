"""GPU: VideoTokenizer.forward, the training forward of the tokenizer mirror (dreamer4.py:4239-4603 for the supported subset), against the fixtures
frozen from the reference under its own recorded draws (tools/gen_tok_train_golden.py; tests/test_tok_train_host.py pins the float64 restatement to
the same files).  Tolerances are the ones tests/test_gpu_backward.py holds the dynamics training forward to against train.npz, and
tests/test_gpu_wide_frames.py its model-level comparison on wide frames: every loss term and the total within 1e-5, latents and the reconstructed
video within 2e-4, every recorded parameter gradient within 1e-3 of its scale, the normaliser state within 1e-4."""
import pytest
import torch

import tok_train_cases as TC
from dreamer4_amd import _lib
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
def narrow():
    return TC.fixture()


def run_case(tok, kw, g, name, check_state=True):
    """One recorded call: losses, latents, reconstruction, every recorded gradient; -> the number of gradients compared"""
    t = lambda k: torch.from_numpy(g[f'{name}_{k}'])
    video = t('video').cuda()
    frames = 1 if video.ndim == 4 else video.shape[2]
    if tok.use_loss_normalization and check_state:
        with torch.no_grad():
            tok.recon_loss_normalizer.exp_avg_sq.copy_(t('norm_before'))
    tok.zero_grad(set_to_none=True)
    total, (losses, recon_video) = tok(video, return_intermediates=True, draws=TC.case_draws(g, name))
    assert isinstance(losses, TokenizerLosses) and all(float(getattr(losses, f)) == 0. for f in losses._fields if f != 'recon')
    close(losses.recon, t('recon'), 'recon', TC.LOSS_TOL); close(total, t('total'), 'total', TC.LOSS_TOL)
    close(recon_video, t('recon_video'), 'recon_video', TC.VALUE_TOL)
    with torch.no_grad():
        close(tok(video, return_latents=True, patch_mask=t('patch_mask')), t('latents'), 'latents', TC.VALUE_TOL)
    if tok.use_loss_normalization:
        close(tok.recon_loss_normalizer.exp_avg_sq, t('norm_after'), 'normaliser state', TC.STATE_TOL)
    total.backward()
    grads, own = TC.case_grads(g, name), dict(tok.named_parameters())
    assert set(grads) == {k for k in own if TC.has_gradient(k, kw, frames)}, 'the fixture holds the complete set'
    for k, ref in grads.items():
        assert own[k].grad is not None, k
        close(own[k].grad, ref, 'd ' + k, TC.GRAD_TOL)
    gmax = max(v.abs().max().item() for v in grads.values())
    for k, p in own.items():
        if k not in grads and p.grad is not None:                      # unread parameters; on one frame, the cancelled time-attention blocks
            assert p.grad.abs().max().item() <= TC.NOISE_FLOOR * gmax, k
    return len(grads)


@pytest.mark.parametrize('name,extra,count', [('train', {}, 132), ('train2', {}, 132), ('nonorm', dict(use_loss_normalization=False), 132),
                                              ('xspace', dict(decoder_v_space_loss=False), 132), ('image', {}, 114)])
def test_training_forward_vs_reference_fixture(narrow, name, extra, count):
    kw, W, g = narrow
    assert run_case(mirror(kw, W, **extra), kw, g, name) == count


def test_second_call_carries_the_normaliser_state(narrow):
    kw, W, g = narrow
    tok = mirror(kw, W)
    for name in ('train', 'train2'):                                   # the state is NOT reset in between
        t = lambda k: torch.from_numpy(g[f'{name}_{k}'])
        close(tok.recon_loss_normalizer.exp_avg_sq, t('norm_before'), 'state before ' + name, TC.STATE_TOL)
        total = tok(t('video').cuda(), draws=TC.case_draws(g, name))
        close(total, t('total'), 'total of ' + name, TC.LOSS_TOL)
        close(tok.recon_loss_normalizer.exp_avg_sq, t('norm_after'), 'state after ' + name, TC.STATE_TOL)
    before = tok.recon_loss_normalizer.exp_avg_sq.clone()
    tok(torch.from_numpy(g['train_video']).cuda(), draws=TC.case_draws(g, 'train'), update_loss_ema=False)
    assert torch.equal(tok.recon_loss_normalizer.exp_avg_sq, before), 'update_loss_ema=False leaves the state alone'
    tok.eval()
    tok(torch.from_numpy(g['train_video']).cuda(), draws=TC.case_draws(g, 'train'))
    assert torch.equal(tok.recon_loss_normalizer.exp_avg_sq, before), 'update_loss_ema defaults to self.training'


def test_return_latents_under_a_given_patch_mask_has_gradient(narrow):
    kw, W, g = narrow
    tok = mirror(kw, W)
    lat = tok(torch.from_numpy(g['latents_video']).cuda(), return_latents=True, patch_mask=torch.from_numpy(g['latents_patch_mask']))
    close(lat, g['latents_latents'], 'latents', TC.VALUE_TOL)
    lat.square().sum().backward()
    assert tok.mask_token.grad.abs().max().item() > 0 and tok.patch_to_tokens._modules['1'].weight.grad.abs().max().item() > 0
    assert tok.time_embed.weight.grad is None, 'the decoder is not run'
    tok.eval()                                                         # eval: no masking by default = tokenize
    video = torch.from_numpy(g['latents_video']).cuda()
    with torch.no_grad():
        close(tok(video, return_latents=True), tok.tokenize(video), 'eval latents against the encoder engine', TC.VALUE_TOL)


def test_wide_fixture_needs_train_wide_frames_and_matches_with_it():
    kw, W, g = TC.fixture(wide=True)
    video = torch.from_numpy(g['train_video']).cuda()
    with pytest.raises(_lib.D4Error):
        mirror(kw, W)(video, draws=TC.case_draws(g, 'train'))
    assert run_case(mirror(kw, W, train_wide_frames=True), kw, g, 'train') == 132


def test_decode_and_tokenize_are_untouched_by_a_training_forward(narrow):
    kw, W, g = narrow
    tok = mirror(kw, W).eval()
    video = torch.from_numpy(g['train_video']).cuda()
    noise = torch.from_numpy(g['train_noise']).cuda()
    lat0 = tok.tokenize(video)
    dec0 = tok.decode(lat0, noise=noise)
    tok.train()
    tok(video, draws=TC.case_draws(g, 'train')).backward()
    tok.eval()
    assert torch.equal(tok.tokenize(video), lat0) and torch.equal(tok.decode(lat0, noise=noise), dec0)


def test_ten_adamw_steps_lower_the_reconstruction_loss(narrow):
    """A short optimisation on one fixed clip, fresh draws every step; judged on FIXED draws before and after (a step's loss depends on its own mask,
    time and noise).  The backward is usable, not just correct."""
    kw, W, g = narrow
    tok = mirror(kw, W, use_loss_normalization=False)
    video = torch.from_numpy(g['train_video']).cuda()
    fixed = TC.case_draws(g, 'train')
    probe = lambda: tok(video, draws=fixed).item()
    with torch.no_grad():
        first = probe()
    opt = torch.optim.AdamW([p for k, p in tok.named_parameters() if TC.has_gradient(k)], lr=3e-3, weight_decay=0.)
    gen = torch.Generator(device='cuda').manual_seed(3)
    for step in range(10):
        opt.zero_grad(set_to_none=True)
        tok(video, generator=gen).backward()
        opt.step()
        tok.invalidate_prepared()
    with torch.no_grad():
        last = probe()
    assert last < first, (first, last)


def test_dispatcher_route_gives_the_same_results(narrow, monkeypatch):
    """D4_TRUNK_DISPATCHER=1: the pixel-side operators (and the blocks) through their torch.ops.d4hip registrations instead of plain autograd.Functions:
    the same C entry points."""
    kw, W, g = narrow
    video = torch.from_numpy(g['train_video']).cuda()
    got = []
    for route in ('0', '1'):
        monkeypatch.setenv('D4_TRUNK_DISPATCHER', route)
        tok = mirror(kw, W)
        total = tok(video, draws=TC.case_draws(g, 'train'))
        total.backward()
        got.append((total, tok.mask_token.grad, tok.patch_to_tokens._modules['2'].weight.grad, tok.noised_patch_to_tokens._modules['1'].weight.grad))
    for a, b in zip(*got):
        close(b, a, 'dispatcher route against the default route', 1e-6)


def test_default_constructed_tokenizer_trains_on_every_parameter_it_reads():
    torch.manual_seed(0)
    tok = VideoTokenizer(dim=64, dim_latent=8, patch_size=4, image_size=16, num_latent_tokens=8, encoder_depth=4, decoder_depth=4, attn_heads=2,
                         lpips_loss_weight=0.).cuda().train()
    video = torch.rand(2, 3, 4, 16, 16, generator=torch.Generator().manual_seed(1)).cuda()
    loss = tok(video, generator=torch.Generator(device='cuda').manual_seed(2))
    assert loss.shape == () and torch.isfinite(loss)
    loss.backward()
    for k, p in tok.named_parameters():
        assert (p.grad is not None and p.grad.abs().max().item() > 0) == TC.has_gradient(k), k
