"""Host: the learner's two actor-critic options, keep_reward_ema_stats and clip_values, without a GPU.

  * The float64 references of tests/learn_norm_ref.py, put behind the heads of oracle/restate.py, reproduce tests/golden/learn_norm.npz: the
    reference implementation's losses, head gradients and EMA buffers after the first and the second of two consecutive calls, for ppo and pmpo,
    for the HL-Gauss and the two-hot value head; in the fixture both branches of the maximum and both sides of the clamp occur.
  * The tables of tests/learn_norm_cases.py hold what they name; every row of the clipped-value cases keeps its margins (an input condition, so no
    row is ever left out of a comparison), and the five situations each make up at least 10 % of the rows of at least one case.
  * Every mutation of the references moves an output of at least one case by 10 x the GPU bound, on the very inputs the GPU test uses; the float32
    evaluation of each reference stays within the recorded E32, which is at most twice the measured one.
  * The new constructor arguments are recorded in the config and survive a checkpoint; run_learner refuses a process group of several ranks."""
import math

import pytest
import torch

import learn_cases as LC
import learn_norm_cases as NC
import learn_norm_ref as N
from oracle import restate
from util import golden_oracle, load_golden, t

ROOM = 10
SEEN = {'stats': set(N.STATS_MUTATIONS), 'clip_hl': set(N.CLIP_MUTATIONS), 'clip_twohot': set(N.CLIP_MUTATIONS)}
HEADS = ('policy_head', 'value_head', 'action_embedder.discrete_action_unembed')


# ------------------------------------------------------------------------------------------------------------------- the fixture
def fixture_exp(g, name, dtype=torch.float64):
    f = lambda k: t(g[f'{name}_exp_{k}'])
    term = f('terminals')
    return dict(latents=f('latents').to(dtype), agent_embed=f('agent_embed').to(dtype), rewards=f('rewards').to(dtype), values=f('values').to(dtype),
                log_probs=f('log_probs').to(dtype), actions=f('actions'), old_action_unembeds=f('unembeds').to(dtype), lens=f('lens'), terminals=term,
                is_truncated=~term, step_size=int(g[f'{name}_step_size']))


def reference_step(cfg, W, exp, obj, ema, decay, value_clip, monkeypatch):
    """One learn_from_experience call with both options on, in float64: restate's heads and policy loss, this suite's references for the return
    statistics and the clipped value loss.  -> policy loss, value loss, the EMA pair after the call, returns, per-row terms."""
    plain = restate.returns_and_advantage
    state = {}

    def with_stats(cfg_, exp_, normalize=True, eps=1e-6):
        returns, old, _, mask = plain(cfg_, exp_, normalize=False)
        f32 = lambda v: torch.tensor(v, dtype=torch.float32).item()
        s = N.return_stats_ref(dict(returns=returns.reshape(-1), old_values=old.reshape(-1), mask=mask.reshape(-1).double(), ema=ema, decay=decay,
                                    q=(f32(0.05), f32(0.95))))
        adv = s['adv'].reshape(returns.shape)
        if normalize:
            mean = restate.masked_mean(adv, mask)
            adv = (adv - mean) / restate.masked_mean((adv - mean).pow(2), mask).clamp(min=eps).sqrt()
        state.update(ema=s['ema'], returns=returns, old=old, mask=mask)
        return returns, old, adv, mask

    with monkeypatch.context() as mp:
        mp.setattr(restate, 'returns_and_advantage', with_stats)
        # (restate's own, unclipped value loss is not used; its two-hot encoder is float32 only)
        mp.setattr(restate, 'symexp_two_hot', lambda values, vrange, bins: torch.zeros(*values.shape, bins, dtype=values.dtype))
        pl, _ = restate.learn_losses(cfg, W, exp, obj)
    vbins = restate.value_head_bins(cfg, W, exp['agent_embed'])
    bins = cfg.value_num_bins
    two_hot = cfg.reward_encoder_type == 'symexp_two_hot'
    sup = W['value_encoder.bin_values'].float() if two_hot else torch.linspace(cfg.value_range[0], cfg.value_range[1], bins + 1)
    p = dict(returns=state['returns'].reshape(-1), old_values=state['old'].reshape(-1), support=sup, vmin=cfg.value_range[0], vmax=cfg.value_range[1],
             sigma=cfg.hl_gauss_sigma_to_bin_ratio * (cfg.value_range[1] - cfg.value_range[0]) / bins, eps=cfg.hl_gauss_eps, two_hot=two_hot, value_clip=value_clip)
    terms = N.value_clip_terms(p, vbins.reshape(-1, bins))
    vl = terms['row'][state['mask'].reshape(-1)].mean()
    return pl, vl, state['ema'], state, terms


def close(got, want, atol, rtol, what):
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    assert got.shape == want.shape and torch.allclose(got, want, atol=atol, rtol=rtol), f'{what}: max abs diff {(got - want).abs().max().item():.3e} (scale {want.abs().max().item():.3e})'


@pytest.mark.parametrize('name,obj', [(n, o) for n in ('hl', 'symexp') for o in ('ppo', 'pmpo')])
def test_references_reproduce_the_reference_fixture(name, obj, monkeypatch):
    g = load_golden('learn_norm.npz')
    cfg, W = golden_oracle(str(g[f'{name}_weights']))
    W = {k: (v.double().requires_grad_(k.startswith(HEADS)) if v.is_floating_point() else v) for k, v in W.items()}
    exp = fixture_exp(g, name)
    ema = (0., 1.)
    heads = {k: v for k, v in W.items() if k.startswith(HEADS) and v.numel() > 0}
    for call in (1, 2):
        pl, vl, ema_t, state, terms = reference_step(cfg, W, exp, obj, ema, float(g[f'{name}_decay']), float(g[f'{name}_value_clip']), monkeypatch)
        tag = f'{name}_{obj}_call{call}'
        close(pl.detach(), g[f'{tag}_policy_loss'], 1e-5, 1e-5, tag + ' policy loss')
        close(vl.detach(), g[f'{tag}_value_loss'], 1e-5, 1e-5, tag + ' value loss')
        close(ema_t, g[f'{tag}_ema'], 1e-6, 1e-5, tag + ' ema')
        grads = dict(zip(heads, torch.autograd.grad(pl + vl, list(heads.values()), allow_unused=True)))
        n = 0
        for k, v in g.items():
            kind, _, key = k.partition('/')
            if not kind.startswith(tag + '_g'):
                continue
            gr = grads[key]
            got = {'grad': gr, 'gnorm': gr.norm(), 'gsample': gr.flatten()[::97]}[kind[len(tag) + 1:]]
            close(got, v, 2e-6, 1e-3, k); n += 1
        assert n >= 8, n
        ema = tuple(torch.tensor(g[f'{tag}_ema']).tolist())              # the buffers are float32: carry what the reference carried
        if call == 1:
            close(state['returns'], g[f'{name}_returns'], 1e-5, 1e-5, 'returns')
            mask = state['mask'].reshape(-1)
            assert torch.equal(mask, t(g[f'{name}_mask']).reshape(-1))
            branch, side = (terms['loss2'] > terms['loss1'])[mask], torch.sign(terms['diff']) * (terms['diff'].abs() > float(g[f'{name}_value_clip']))
            assert torch.equal(branch, t(g[f'{name}_branch']).reshape(-1)[mask]) and torch.equal(side[mask].detach(), t(g[f'{name}_side']).reshape(-1)[mask].double())
            assert branch.any() and not branch.all(), 'both branches of the maximum'
            assert {-1., 1.} <= set(side[mask].tolist()), 'both sides of the clamp'
    first, second = g[f'{name}_{obj}_call1_ema'], g[f'{name}_{obj}_call2_ema']
    assert abs(first[0] - second[0]) > 1e-3 and abs(first[1] - second[1]) > 1e-3, 'the second call starts from the first call\'s buffers'


# ------------------------------------------------------------------------------------------------------------------- the case tables
def test_case_tables_cover_what_they_name():
    cases = [c for tb in NC.ALL_TABLES.values() for c in tb]
    seeds, names = [c['seed'] for c in cases], [c['name'] for c in cases]
    assert len(set(seeds)) == len(seeds) and len(set(names)) == len(names) and min(seeds) >= 32000
    assert set(seeds).isdisjoint(c['seed'] for tb in LC.ALL_TABLES.values() for c in tb)
    assert NC.BOUND == {f: 8 * e for f, e in NC.E32.items()} and set(NC.E32) == set(NC.FAMILIES) == set(SEEN)
    st = NC.STATS
    assert {c['kept'] for c in st} == set(NC.KEPT) | {0} and {c['mask'] for c in st} == {'ones', 'rand', 'one', 'none'}
    assert {(c['kept'], c['mask']) for c in st} >= {(k, m) for k in NC.KEPT for m in ('ones', 'rand')}
    assert {c['data'] for c in st} == set(NC.DATA) and {c['q'] for c in st} == set(NC.QS) and {c['ema'] for c in st} == set(NC.EMA)
    for c in st:
        d = NC.stats_inputs(c)
        kept = d['returns'].numel() if d['mask'] is None else int(d['mask'].sum())
        assert kept == c['kept'] and d['returns'].dtype == torch.float32
        ref = NC.stats_expect(c, d)
        if c['ema'] == 'tiny':
            assert ref['ema'][1] < N.STD_EPS, 'the carried-in variance must stay below the clamp'
        if c['data'] in ('ties', 'signs'):
            z = d['returns'][d['returns'] == 0]
            assert z.numel() == 0 or c['kept'] < 8 or (torch.signbit(z).any() and not torch.signbit(z).all()), 'both zeros'
        if c['data'] == 'range' and c['kept'] >= 64:
            a = d['returns'].abs()
            assert a.max() / a.min() > 1e5
        if c['kept'] == 21 and c['q'] == (0.05, 0.95):                     # both positions on integer ranks, 1 and 19, to the rounding of float32(q)
            assert all(abs(q * 20 - r) < 1e-6 for q, r in zip(d['q'], (1, 19)))
    cl = NC.CLIP_ALL
    assert {(c['two_hot'], c['bins']) for c in cl} == {(th, b) for th in (0, 1) for b in (20, 63, 64, 65, 255)} and {c['rows'] for c in cl} == {1, 4, 5, 130}
    assert {(c['two_hot'], c['ldpad']) for c in cl} == {(th, p) for th in (0, 1) for p in ('r4', 'p5')}
    assert {(c['two_hot'], c['mask']) for c in cl} == {(th, m) for th in (0, 1) for m in ('rand', 'null', 'zero')}
    best = {}
    for c in cl:
        d = NC.clip_inputs(c)
        assert (NC.clip_margins(d) >= NC.clip_margin(c)).all(), c['name']
        for k, v in NC.clip_situations(c, d).items():
            best[(c['two_hot'], k)] = max(best.get((c['two_hot'], k), 0.), v if c['rows'] >= 128 else 0.)
        if c['rows'] == 130:
            lo, hi = NC.clip_range(c)
            tv = N.value_clip_terms(d, d['logits'].double())
            clipped = d['old_values'].double() + tv['diff'].clamp(-d['value_clip'], d['value_clip'])
            assert (d['returns'] > hi).any() and (d['returns'] < lo).any() and (clipped > hi).any() and (clipped < lo).any(), 'returns and clipped values beyond the range'
    assert all(v >= 0.1 for v in best.values()) and len(best) == 10, best            # each situation, for each encoder, in a case of 130 rows


@pytest.mark.parametrize('family', sorted(NC.FAMILIES))
def test_inputs_see_every_mutation_and_float32_stays_within_e32(family):
    table, inputs, expect, mutations = NC.FAMILIES[family]
    e32, bound = NC.E32[family], NC.BOUND[family]
    rows = []
    for c in table:
        d = inputs(c)
        ref = expect(c, d)
        assert all(torch.isfinite(x).all() for x in ref.values()), c['name']
        rows.append((c['name'], N.err_all(expect(c, d, torch.float32), ref), {m: N.err_all(expect(c, d, mut=(m,)), ref) for m in mutations}))
    best = {m: max((mv[m], n) for n, _, mv in rows) for m in mutations}
    seen = {m for m, (v, _) in best.items() if v >= ROOM * bound}
    worst = max(rows, key=lambda r: r[1])
    print(f'{family}: E32 measured {worst[1]:.3e} ({worst[0]}), recorded {e32:.3e}, GPU bound {bound:.3e}; largest movement per mutation: '
          + ', '.join(f'{m} {v:.2e} ({n})' for m, (v, n) in sorted(best.items())))
    bad = [f'{n}: float32 evaluation {e:.3e} above the recorded E32 {e32:.3e}' for n, e, _ in rows if not e <= e32]
    assert not bad, '\n'.join(bad)
    assert worst[1] >= e32 / 2, 'the recorded E32 is more than twice what this table measures'
    assert seen == SEEN[family], (sorted(seen - SEEN[family]), sorted(SEEN[family] - seen))


def test_quantile_bound_holds_for_a_float32_interpolation():
    """The bound of the GPU test on lo and hi, tried on the CPU: one float32 interpolation between the float32 neighbours against float64."""
    for c in NC.STATS:
        if c['kept'] == 0:
            continue
        d = NC.stats_inputs(c)
        ref = NC.stats_expect(c, d)['stats'][:2]
        for q, want, (x0, x1) in zip(d['q'], ref.tolist(), N.order_statistics(d)):
            pos = float(torch.tensor(q, dtype=torch.float32).double()) * (c['kept'] - 1)
            got = torch.lerp(torch.tensor(x0, dtype=torch.float32), torch.tensor(x1, dtype=torch.float32), torch.tensor(pos - math.floor(pos), dtype=torch.float32)).item()
            assert abs(got - want) <= NC.QUANTILE_ULPS * 2. ** -24 * max(abs(x0), abs(x1)), c['name']


# ------------------------------------------------------------------------------------------------------------------- the Python surface
KW = dict(dim=16, dim_latent=4, num_latent_tokens=3, depth=1, time_block_every=1, attn_heads=1, attn_dim_head=16, num_discrete_actions=(3,),
          reward_encoder_kwargs=dict(num_bins=15), multi_token_pred_len=1)


def test_constructor_config_and_checkpoint_round_trip(tmp_path):
    from dreamer4_amd import DynamicsWorldModel
    m = DynamicsWorldModel(**KW)
    assert (m.keep_reward_ema_stats, m.reward_ema_decay, m.reward_quantile_filter, m.clip_values, m.value_clip) == (False, 0.998, (0.05, 0.95), False, 0.4)
    m = DynamicsWorldModel(**KW, keep_reward_ema_stats=True, reward_ema_decay=0.99, reward_quantile_filter=(0.1, 0.9), clip_values=True, value_clip=0.25)
    assert (m.keep_reward_ema_stats, m.reward_ema_decay, m.reward_quantile_filter, m.clip_values, m.value_clip) == (True, 0.99, (0.1, 0.9), True, 0.25)
    kw = m._config[1]
    assert kw['keep_reward_ema_stats'] is True and kw['clip_values'] is True and kw['value_clip'] == 0.25 and kw['reward_ema_decay'] == 0.99
    with torch.no_grad():
        m.ema_returns_mean.fill_(0.7); m.ema_returns_var.fill_(3.5)
    path = tmp_path / 'wm.pt'
    m.save(str(path))
    r = DynamicsWorldModel.init_and_load(str(path))
    assert (r.keep_reward_ema_stats, r.reward_ema_decay, r.reward_quantile_filter, r.clip_values, r.value_clip) == (True, 0.99, (0.1, 0.9), True, 0.25)
    assert r.ema_returns_mean.item() == pytest.approx(0.7) and r.ema_returns_var.item() == 3.5
    for bad in (dict(reward_quantile_filter=(0.9, 0.1)), dict(reward_quantile_filter=(0.1,)), dict(reward_ema_decay=0.3), dict(value_clip=-1.)):
        with pytest.raises(ValueError):
            DynamicsWorldModel(**KW, **bad)


def test_run_learner_refuses_several_ranks_with_the_return_statistics(monkeypatch):
    from dreamer4_amd import Actions, DynamicsWorldModel, Experience, learner, parallel
    m = DynamicsWorldModel(**KW, keep_reward_ema_stats=True)
    B, T = 2, 3
    exp = Experience(latents=torch.zeros(B, T, 3, 4), agent_embed=torch.zeros(B, T, 16), rewards=torch.zeros(B, T), values=torch.zeros(B, T),
                     log_probs=Actions(torch.zeros(B, T, 1), None), actions=Actions(torch.zeros(B, T, 1, dtype=torch.long), None), step_size=4)
    monkeypatch.setattr(parallel, 'world_size', lambda group=None: 2)
    with pytest.raises(NotImplementedError, match='single-process'):
        learner.run_learner(m, exp)
