"""GPU: MuonAdamAtan2(muon_products='bf16') (dreamer4_amd/optim.py) as a user holds it: three steps on the fixture's small
DynamicsWorldModel with the injected gradients of tests/muon_cases.py.  The Muon-group parameters follow the float64 trajectory within
FACTOR (2) x E16_TRAJECTORY (tests/muon_bf16_cases.py: the emulated contract's own distance from float64); everything the iteration does not touch
(the Adam-atan2 group and its state, every momentum, the skipped and unlisted parameters) holds the bits of a 'fp32' optimiser on the same gradients.
A save / load mid-run continues bit for bit, the state loads across modes, and ten steps lower the loss of each whole-model training forward."""
import copy

import pytest
import torch

import muon_bf16_cases as BC
import muon_cases as MC
from dreamer4_amd import MuonAdamAtan2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def problem():
    """the CPU model (initial weights), its synthetic gradients, and the float64 trajectories, computed once"""
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    m = MC.small_dynamics()
    return dict(model=m, init={k: p.detach().clone() for k, p in m.named_parameters()}, grads=MC.trajectory_gradients(m), muon=BC.muon_names(m),
                ref={case: MC.trajectory_reference(m, case, torch.float64) for case in MC.TRAJECTORY})


def device_model(problem):
    m = MC.small_dynamics()
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(problem['init'][k])
    return m.cuda()


def optimiser(m, case, products='bf16', **extra):
    listed = [p for k, p in m.named_parameters() if k not in MC.UNLISTED]
    return MuonAdamAtan2(m.muon_parameters(), listed, **MC.TRAJECTORY[case], muon_products=products, **extra)


def set_grads(m, grads):
    for k, p in m.named_parameters():
        p.grad = None if grads[k] is None else grads[k].cuda()


def run(problem, case, products, steps=None):
    m = device_model(problem)
    opt = optimiser(m, case, products)
    for step in problem['grads'][:steps]:
        set_grads(m, step)
        opt.step()
    return m, opt


@pytest.mark.parametrize('case', sorted(MC.TRAJECTORY))
def test_three_steps_follow_the_float64_restatement(problem, case):
    m, opt = run(problem, case, 'bf16')
    hi, opt_hi = run(problem, case, 'fp32')
    clip = 2 if 'max_grad_norm' in MC.TRAJECTORY[case] else 0
    assert opt.last_launches == clip + (3 + 3 * 5) + 1 and opt_hi.last_launches == clip + (2 + 3 * 5) + 1       # bf16: + normalise
    assert opt.muon_workspace_bytes() <= opt_hi.muon_workspace_bytes()
    ref, bound = problem['ref'][case], BC.FACTOR * BC.E16_TRAJECTORY[case]
    worst, moved = (0., ''), 0
    for (k, p), (_, q) in zip(m.named_parameters(), hi.named_parameters()):
        if k in MC.UNLISTED or k == MC.SKIPPED or p.numel() == 0:
            assert torch.equal(p.detach().cpu(), problem['init'][k]), f'{k} moved'
            continue
        st, st_hi = opt.state[p], opt_hi.state[q]
        assert st['step'] == st_hi['step'] and torch.equal(st['exp_avg'], st_hi['exp_avg']), f'{k}: exp_avg depends on the product form'
        if k in problem['muon']:
            assert st.keys() == st_hi.keys() == {'step', 'exp_avg'}
            moved += not torch.equal(p, q)
            err = MC.rel_err(p.detach().cpu(), ref[k])
            worst = max(worst, (err, k))
            assert err <= bound, f'{k}: error {err:.3e} above the bound {bound:.3e}'
        else:
            assert torch.equal(p, q) and torch.equal(st['exp_avg_sq'], st_hi['exp_avg_sq']), f'{k}: the Adam-atan2 group depends on the product form'
    assert moved > 0, 'no Muon parameter differs from the fp32 form\'s: the bf16 products did not run'
    print(f'{case}: worst error {worst[0]:.3e} ({worst[1]}), bound {bound:.3e}, ratio {worst[0] / bound:.2f}')


def test_save_and_load_mid_run_continues_bit_for_bit_and_loads_across_modes(problem):
    case = 'nesterov_spectral_clip'
    straight, _ = run(problem, case, 'bf16')
    resumed, opt_a = run(problem, case, 'bf16', steps=2)
    state = copy.deepcopy(opt_a.state_dict())            # as a file would hold it: load_state_dict may share tensors with what it is given
    opt_b = optimiser(resumed, case, 'bf16', workspace_bytes=2 << 20)          # another pass partition on top
    opt_b.load_state_dict(copy.deepcopy(state))
    set_grads(resumed, problem['grads'][2])
    opt_b.step()
    passes = (opt_b.last_launches - 2 - 1) // (3 + 3 * 5)
    assert passes >= 3 and opt_a.last_launches == 2 + (3 + 3 * 5) + 1, (passes, opt_a.last_launches)
    for (k, a), (_, b) in zip(straight.named_parameters(), resumed.named_parameters()):
        assert torch.equal(a, b), k
    # the same state under 'fp32': the third step is then the fp32 form's on the bf16 run's weights and momentum
    other, _ = run(problem, case, 'bf16', steps=2)
    opt_d = optimiser(other, case, 'fp32')
    opt_d.load_state_dict(state)
    set_grads(other, problem['grads'][2])
    opt_d.step()
    assert opt_d.last_launches == 2 + (2 + 3 * 5) + 1
    resumed_named = dict(resumed.named_parameters())
    differs = 0
    for (k, a), (_, b) in zip(straight.named_parameters(), other.named_parameters()):
        assert torch.isfinite(b).all(), k
        if k in problem['muon'] and k != MC.SKIPPED:
            assert torch.equal(opt_d.state[b]['exp_avg'], opt_b.state[resumed_named[k]]['exp_avg']), k
            differs += not torch.equal(a, b)
        else:
            assert torch.equal(a, b), k
    assert differs > 0, 'the fp32 optimiser stepped with the bf16 products'


def ten_steps(make, probe, forward, products):
    model = make()
    with torch.no_grad():
        first = probe(model)
    opt = MuonAdamAtan2(model.muon_parameters(), model.parameters(), lr=3e-3, muon_lr=2e-2, max_grad_norm=1., muon_products=products)
    gen = torch.Generator(device='cuda').manual_seed(3)
    for step in range(10):
        opt.zero_grad(set_to_none=True)
        forward(model, gen).backward()
        opt.step()
        model.invalidate_prepared()
    with torch.no_grad():
        return first, probe(model)


def test_ten_steps_lower_the_tokenizer_s_reconstruction_loss():
    import tok_train_cases as TC
    from test_gpu_tok_train import mirror
    kw, W, g = TC.fixture()
    video = torch.from_numpy(g['train_video']).cuda()
    fixed = TC.case_draws(g, 'train')
    got = {p: ten_steps(lambda: mirror(kw, W, use_loss_normalization=False), lambda tok: tok(video, draws=fixed).item(),
                        lambda tok, gen: tok(video, generator=gen), p) for p in ('bf16', 'fp32')}
    print(f"tokenizer: bf16 {got['bf16'][0]:.5f} -> {got['bf16'][1]:.5f} | fp32 {got['fp32'][0]:.5f} -> {got['fp32'][1]:.5f}")
    assert got['bf16'][1] < got['bf16'][0], got


def test_ten_steps_lower_the_dynamics_flow_loss():
    from util import golden_model, load_golden, t
    g = load_golden('train.npz')
    lat = t(g['latents']).cuda()
    B_, T_ = lat.shape[:2]
    make = lambda: golden_model('weights_train.npz').cuda()
    fixed = dict(shortcut_train=False, step_sizes_log2=torch.zeros(B_, dtype=torch.long),
                 signal_levels=torch.randint(0, make().max_steps, (B_, T_), generator=torch.Generator().manual_seed(5)),
                 noise=torch.randn(lat.shape, generator=torch.Generator().manual_seed(6)))
    got = {p: ten_steps(make, lambda m: m(latents=lat, discrete_actions=t(g['actions']), draws=fixed, add_autoregressive_action_loss=False).item(),
                        lambda m, gen: m(latents=lat, discrete_actions=t(g['actions']), generator=gen, add_autoregressive_action_loss=False), p)
           for p in ('bf16', 'fp32')}
    print(f"dynamics: bf16 {got['bf16'][0]:.5f} -> {got['bf16'][1]:.5f} | fp32 {got['fp32'][0]:.5f} -> {got['fp32'][1]:.5f}")
    assert got['bf16'][1] < got['bf16'][0], got
