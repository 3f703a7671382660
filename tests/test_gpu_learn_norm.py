"""GPU: learn_from_experience with keep_reward_ema_stats and clip_values against tests/golden/learn_norm.npz, the reference
implementation's own two consecutive calls (tools/gen_golden_learn_norm.py): losses, head gradients and both EMA buffers after each call, at the
tolerances tests/test_gpu_learn.py uses for learn.npz; the whole-model path; both options off are the bits of a model built without them; the
trainer passes the model's options through."""
import pytest
import torch

from dreamer4_amd import Actions, DreamTrainer, Experience
from test_gpu_learn import close
from util import golden_model, load_golden, t

pytestmark = pytest.mark.gpu
HEADS = ('policy_head', 'value_head', 'action_embedder.discrete_action_unembed')


@pytest.fixture(scope='module')
def G():
    return load_golden('learn_norm.npz')


def experience(g, name):
    f = lambda k: t(g[f'{name}_exp_{k}'])
    return Experience(latents=f('latents'), agent_embed=f('agent_embed'), rewards=f('rewards'), values=f('values'), log_probs=Actions(f('log_probs'), None),
                      actions=Actions(f('actions'), None), lens=f('lens'), terminals=f('terminals'), is_truncated=~f('terminals'),
                      old_action_unembeds=Actions(f('unembeds'), None), step_size=int(g[f'{name}_step_size']))


def model(g, name, **over):
    kw = dict(keep_reward_ema_stats=True, clip_values=True, value_clip=float(g[f'{name}_value_clip']), reward_ema_decay=float(g[f'{name}_decay']))
    kw.update(over)
    return golden_model(str(g[f'{name}_weights']), **kw).cuda()


def ema_of(m):
    return torch.stack([m.ema_returns_mean.detach(), m.ema_returns_var.detach()]).cpu()


@pytest.mark.parametrize('name,obj', [(n, o) for n in ('hl', 'symexp') for o in ('ppo', 'pmpo')])
def test_two_consecutive_calls_vs_reference_fixture(G, name, obj):
    m = model(G, name)
    exp = experience(G, name)
    P = dict(m.named_parameters())
    assert ema_of(m).tolist() == [0., 1.]
    for call in (1, 2):
        tag = f'{name}_{obj}_call{call}'
        m.zero_grad()
        pl, vl = m.learn_from_experience(exp, objective=obj)
        close(pl, G[f'{tag}_policy_loss'], atol=1e-5); close(vl, G[f'{tag}_value_loss'], atol=1e-5)
        close(ema_of(m), G[f'{tag}_ema'], atol=1e-5)
        pl.backward(retain_graph=True); vl.backward()
        n = 0
        for k, v in G.items():
            kind, _, key = k.partition('/')
            if kind == f'{tag}_grad':
                close(P[key].grad, v, atol=2e-6, rtol=1e-3); n += 1
            elif kind == f'{tag}_gnorm':
                close(P[key].grad.norm(), v, atol=1e-6, rtol=1e-3); n += 1
            elif kind == f'{tag}_gsample':
                close(P[key].grad.flatten()[::97], v, atol=2e-6, rtol=1e-3)
        assert n >= 8, n
        assert all(p.grad is None for k, p in P.items() if not k.startswith(HEADS)), 'only the two heads learn'
    assert m.ema_returns_mean.device.type == 'cuda' and 'ema_returns_mean' in m.state_dict()


def test_learning_the_whole_world_model_vs_reference_fixture(G):
    """only_learn_policy_value_heads=False with both options on: the gradients reach the trunk, match the reference's norms, and differ from those
    of the run with the options off."""
    exp = experience(G, 'hl')
    norms = {}
    for on in (True, False):
        m = model(G, 'hl') if on else model(G, 'hl', keep_reward_ema_stats=False, clip_values=False)
        P = dict(m.named_parameters())
        for call in ((1, 2) if on else (1,)):
            tag = f'hl_ppo_full_call{call}'
            m.zero_grad()
            pl, vl = m.learn_from_experience(exp, objective='ppo', only_learn_policy_value_heads=False)
            if on:
                close(pl, G[f'{tag}_policy_loss'], atol=1e-5); close(vl, G[f'{tag}_value_loss'], atol=1e-5)
                close(ema_of(m), G[f'{tag}_ema'], atol=1e-5)
            vl.backward(retain_graph=True)
            got = {k: p.grad.norm().cpu() for k, p in P.items() if p.grad is not None}
            if not on:
                trunk = [k for k in got if not k.startswith(HEADS) and f'hl_ppo_full_call1_vgnorm/{k}' in G]
                # (value clipping changes the rows where the clipped loss wins: every trunk gradient of the value loss moves, most of them by per cents)
                moved = [k for k in trunk if not torch.allclose(got[k], norms[k], rtol=1e-2, atol=0.)]
                assert len(trunk) >= 50 and not any(torch.equal(got[k], norms[k]) for k in trunk) and 2 * len(moved) >= len(trunk), 'the options change the trunk gradients'
                break
            n = 0
            for k, v in G.items():
                if k.startswith(f'{tag}_vgnorm/'):
                    close(got[k.split('/', 1)[1]], v, atol=3e-6, rtol=2e-3); n += 1
            assert n >= 90, n
            norms = got
            m.zero_grad()
            pl.backward()
            n = 0
            for k, v in G.items():
                if k.startswith(f'{tag}_pgnorm/'):
                    close(P[k.split('/', 1)[1]].grad.norm(), v, atol=3e-6, rtol=2e-3); n += 1
            assert n >= 90, n


@pytest.mark.parametrize('name', ('hl', 'symexp'))
def test_options_off_are_the_bits_of_a_model_built_without_them(G, name):
    exp = experience(G, name)
    out = []
    for kw in (None, dict(keep_reward_ema_stats=False, clip_values=False, value_clip=0.1, reward_ema_decay=0.9, reward_quantile_filter=(0.2, 0.8))):
        m = golden_model(str(G[f'{name}_weights'])).cuda() if kw is None else golden_model(str(G[f'{name}_weights']), **kw).cuda()
        for obj in ('ppo', 'pmpo'):
            m.zero_grad()
            pl, vl = m.learn_from_experience(exp, objective=obj)
            pl.backward(retain_graph=True); vl.backward()
            out.append([pl.detach().clone(), vl.detach().clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None])
        assert ema_of(m).tolist() == [0., 1.], 'the buffers are not touched with the option off'
    for a, b in zip(out[:2], out[2:]):
        assert len(a) == len(b) > 8 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_each_option_alone_changes_what_it_should(G):
    """keep_reward_ema_stats alone leaves the value loss's bits and moves the pmpo policy loss; clip_values alone leaves the policy loss's bits."""
    exp = experience(G, 'hl')
    base = golden_model(str(G['hl_weights'])).cuda().learn_from_experience(exp, objective='pmpo')
    ema = model(G, 'hl', clip_values=False).learn_from_experience(exp, objective='pmpo')
    clip = model(G, 'hl', keep_reward_ema_stats=False).learn_from_experience(exp, objective='pmpo')
    assert torch.equal(ema[1], base[1]) and not torch.equal(ema[0], base[0])
    assert torch.equal(clip[0], base[0]) and clip[1] > base[1]


def test_trainer_passes_the_options_through(G):
    m = model(G, 'hl')
    tr = DreamTrainer(m, batch_size=3, generate_timesteps=4, seed=3)
    tr.learn(experience(G, 'hl'))
    close(ema_of(m), G['hl_ppo_call1_ema'], atol=1e-5)
