"""GPU: MuonAdamAtan2 (dreamer4_amd/optim.py) as a user holds it: three steps on the fixture's small DynamicsWorldModel against the
float64 restatement (tests/muon_ref.py) stepping a float64 copy, what is in neither list stays put, a save / load mid-run continues bit for bit,
and ten steps lower the loss of each whole-model training forward."""
import pytest
import torch

import muon_cases as MC
from dreamer4_amd import MuonAdamAtan2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def problem():
    """the CPU model (initial weights), its synthetic gradients, and the float64 trajectories, computed once"""
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    m = MC.small_dynamics()
    return dict(model=m, init={k: p.detach().clone() for k, p in m.named_parameters()}, grads=MC.trajectory_gradients(m),
                ref={case: MC.trajectory_reference(m, case, torch.float64) for case in MC.TRAJECTORY})


def device_model(problem):
    m = MC.small_dynamics()
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(problem['init'][k])
    return m.cuda()


def optimiser(m, case, **extra):
    listed = [p for k, p in m.named_parameters() if k not in MC.UNLISTED]
    return MuonAdamAtan2(m.muon_parameters(), listed, **MC.TRAJECTORY[case], **extra)


def set_grads(m, grads):
    for k, p in m.named_parameters():
        p.grad = None if grads[k] is None else grads[k].cuda()


@pytest.mark.parametrize('case', sorted(MC.TRAJECTORY))
def test_three_steps_follow_the_float64_restatement(problem, case):
    m = device_model(problem)
    opt = optimiser(m, case)
    for step in problem['grads']:
        set_grads(m, step)
        opt.step()
        for k, p in m.named_parameters():                      # the clip scales what the kernels read, never .grad
            assert p.grad is None or torch.equal(p.grad.cpu(), step[k]), k
    assert opt.last_launches == (2 if 'max_grad_norm' in MC.TRAJECTORY[case] else 0) + (2 + 3 * 5) + 1
    ref, bound = problem['ref'][case], MC.FACTOR * MC.E32_TRAJECTORY[case]
    worst = (0., '')
    for k, p in m.named_parameters():
        if k in MC.UNLISTED or k == MC.SKIPPED or p.numel() == 0:
            assert torch.equal(p.detach().cpu(), problem['init'][k]), f'{k} moved'
            continue
        assert not torch.equal(p.detach().cpu(), problem['init'][k]), f'{k} did not move'
        err = MC.rel_err(p.detach().cpu(), ref[k])
        worst = max(worst, (err, k))
        assert err <= bound, f'{k}: error {err:.3e} above the bound {bound:.3e}'
    print(f'{case}: worst error {worst[0]:.3e} ({worst[1]}), bound {bound:.3e}')


def test_save_and_load_mid_run_continues_bit_for_bit(problem):
    case = 'nesterov_spectral_clip'
    straight = device_model(problem)
    opt = optimiser(straight, case)
    for step in problem['grads']:
        set_grads(straight, step)
        opt.step()
    resumed = device_model(problem)
    opt_a = optimiser(resumed, case)
    for step in problem['grads'][:2]:
        set_grads(resumed, step)
        opt_a.step()
    state = opt_a.state_dict()
    opt_b = optimiser(resumed, case, workspace_bytes=8 << 20)          # another pass partition on top
    opt_b.load_state_dict(state)
    set_grads(resumed, problem['grads'][2])
    opt_b.step()
    for (k, a), (_, b) in zip(straight.named_parameters(), resumed.named_parameters()):
        assert torch.equal(a, b), k


def test_ten_steps_lower_the_tokenizer_s_reconstruction_loss():
    import tok_train_cases as TC
    from test_gpu_tok_train import mirror
    kw, W, g = TC.fixture()
    tok = mirror(kw, W, use_loss_normalization=False)
    video = torch.from_numpy(g['train_video']).cuda()
    fixed = TC.case_draws(g, 'train')
    probe = lambda: tok(video, draws=fixed).item()
    with torch.no_grad():
        first = probe()
    opt = MuonAdamAtan2(tok.muon_parameters(), tok.parameters(), lr=3e-3, muon_lr=2e-2, max_grad_norm=1.)
    gen = torch.Generator(device='cuda').manual_seed(3)
    for step in range(10):
        opt.zero_grad(set_to_none=True)
        tok(video, generator=gen).backward()
        opt.step()
        tok.invalidate_prepared()
    with torch.no_grad():
        last = probe()
    print(f'tokenizer: {first:.5f} -> {last:.5f}')
    assert last < first, (first, last)


def test_ten_steps_lower_the_dynamics_flow_loss():
    from util import golden_model, load_golden, t
    g = load_golden('train.npz')
    m = golden_model('weights_train.npz').cuda()
    lat = t(g['latents']).cuda()
    B_, T_ = lat.shape[:2]
    fixed = dict(shortcut_train=False, step_sizes_log2=torch.zeros(B_, dtype=torch.long),
                 signal_levels=torch.randint(0, m.max_steps, (B_, T_), generator=torch.Generator().manual_seed(5)),
                 noise=torch.randn(lat.shape, generator=torch.Generator().manual_seed(6)))
    probe = lambda: m(latents=lat, discrete_actions=t(g['actions']), draws=fixed, add_autoregressive_action_loss=False).item()
    with torch.no_grad():
        first = probe()
    opt = MuonAdamAtan2(m.muon_parameters(), m.parameters(), lr=3e-3, muon_lr=2e-2, max_grad_norm=1.)
    gen = torch.Generator(device='cuda').manual_seed(3)
    for step in range(10):
        opt.zero_grad(set_to_none=True)
        m(latents=lat, discrete_actions=t(g['actions']), generator=gen, add_autoregressive_action_loss=False).backward()
        opt.step()
        m.invalidate_prepared()
    with torch.no_grad():
        last = probe()
    print(f'dynamics: {first:.5f} -> {last:.5f}')
    assert last < first, (first, last)
