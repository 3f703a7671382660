"""Host: the inputs and the bounds of tests/test_gpu_learn_ops.py (the learner's loss kernels called alone) can see the errors those tests are for.

  * The tables of tests/learn_cases.py hold the shapes they claim, their seeds are their own, and every non-degenerate policy case is off-policy
    as measured on the float64 reference: at least 20 % of the unmasked rows outside the clip band and 20 % inside, both advantage signs on either
    side, a mean KL of at least 1e-2 per action type where there is a KL term.
  * For every case the float64 reference (tests/learn_ref.py) is evaluated once as it is and once per mutation: every mutation must move an
    output of at least one case by 10 x the GPU bound, on the very inputs the GPU test uses.  SEEN records which mutations each family sees.
  * The float32 evaluation of each reference stays within the recorded E32 of its float64 evaluation, and the recorded E32 is at most twice the
    measured one.
  * The references agree with oracle/restate.py (written independently) in float32 on every case both can express."""
import glob
import importlib
import os

import pytest
import torch

import learn_cases as LC
import learn_ref as L
from oracle import restate

ROOM = 10
SEEN = {
    'gae': {'no_trunc', 'past_len', 'no_lam', 'gamma_wrong', 'defaults_inv', 'last_traj'},
    'policy': set(L.POLICY_MUTATIONS) - {'pmpo_sign0'},
    'policy_wide': {'kl_swap', 'kl_no_grad', 'clip_pass', 'tie_rule', 'spo_no_quad', 'gate_grad', 'gate_sign', 'var_unmasked', 'no_alpha', 'ent_sign', 'beta_log1mx',
                    'link_swap', 'last_row', 'last_type', 'last_cont', 'mask_ignored'},
    'value': set(L.VALUE_MUTATIONS),
}


def other_seeds():
    """the seeds of every other case table of the suite"""
    seeds = []
    for f in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), '*_cases.py'))):
        name = os.path.basename(f)[:-3]
        if name == 'learn_cases':
            continue
        mod = importlib.import_module(name)
        for v in vars(mod).values():
            tables = v.values() if isinstance(v, dict) else [v]
            for t in tables:
                if isinstance(t, (list, tuple)) and t and all(isinstance(c, dict) and 'seed' in c for c in t):
                    seeds += [c['seed'] for c in t]
    return seeds


def test_case_tables_cover_what_they_name():
    cases = [c for t in LC.ALL_TABLES.values() for c in t]
    seeds, names = [c['seed'] for c in cases], [c['name'] for c in cases]
    assert len(set(seeds)) == len(seeds) and len(set(names)) == len(names) and min(seeds) >= 30000
    other = other_seeds()
    assert set(seeds).isdisjoint(other) and len(other) > 300
    assert LC.BOUND == {f: 8 * e for f, e in LC.E32.items()} and set(LC.E32) == set(LC.FAMILIES) == set(SEEN)
    ga = LC.GAE
    assert {c['B'] for c in ga} == {1, 5, 130} and {c['T'] for c in ga} == {1, 2, 7, 33}
    assert {c[k] for c in ga for k in ('lens', 'trunc', 'term')} == {'null', 'mixed'} and any(c['lens'] == c['trunc'] == c['term'] == 'null' for c in ga)
    for c in ga:
        d = LC.gae_inputs(c)
        if d['lens'] is not None:
            assert d['lens'].min() >= 1 and d['lens'].max() <= c['T'] and (c['B'] == 1 or {1, c['T']} <= set(d['lens'].tolist()))
            assert d['rewards'].isnan().sum() == d['values'].isnan().sum() == (c['T'] - d['lens']).sum()          # NaN exactly past `len`
            assert c['T'] < 7 or c['B'] == 1 or ((d['lens'] > 1) & (d['lens'] < c['T'])).any()
        for k in ('trunc', 'term'):
            assert d[k] is None or c['B'] == 1 or (d[k].any() and not d[k].all())
        assert all(torch.isfinite(x).all() for x in LC.gae_expect(c, d).values())
    po = LC.POLICY
    assert {c['rows'] for c in po} == {1, 128, 129, 130, 300} and {c['sizes'] for c in po} == set(LC.SIZES) and {c['ldpad'] for c in po} == {'apad', 'p3'}
    assert {(c['nc'], c['link']) for c in po} >= {(1, 'softplus'), (1, 'exp'), (3, 'softplus'), (3, 'exp')} and any(c['nc'] == 0 for c in po)
    assert {(c['obj'], c['gate'], c['norm']) for c in po if not c['special'] and c['mask'] == 'rand' and c['rows'] >= 128} >= \
        {(o, g, n) for o in ('ppo', 'spo', 'pmpo') for g in (0., 1., 2.5) for n in (0, 1)}
    assert {c['mask'] for c in po} == {'rand', 'null', 'zero'} and {c['special'] for c in po} == {None, 'equal_adv', 'shift90', 'zero_adv'}
    assert {(c['kl'], bool(c['sizes']), c['nc'] > 0) for c in po if c['obj'] == 'pmpo' and c['rows'] >= 128} >= \
        {(k, a, b) for k in ('fwd', 'rev') for a, b in ((True, False), (False, True), (True, True))} | {('off', True, True)}
    assert all(c['special'] == 'wide' and c['nc'] > 0 for c in LC.POLICY_WIDE) and {c['obj'] for c in LC.POLICY_WIDE} == {'ppo', 'spo', 'pmpo'}
    assert {c['link'] for c in LC.POLICY_WIDE} == {'softplus', 'exp'}
    for c in po + LC.POLICY_WIDE:
        d = LC.policy_inputs(c)
        ld, ldc = LC.policy_pads(c)
        assert ld >= sum(c['sizes']) and ldc >= 2 * c['nc'] and (c['kl'] == 'off') == (d['old_logits'] is None and d['old_cparams'] is None)
        if d['logits'] is not None:
            assert 2. < d['logits'].std() < 4. or c['special'] == 'shift90'
            assert (c['special'] == 'shift90') == bool(d['logits'].max() > 80.)
        if d['cparams'] is not None:
            a, b = L.beta_ab(d['cparams'].reshape(c['rows'], c['nc'], 2).double(), c['link'])
            if c['special'] == 'wide':
                assert a.min() >= 10. and b.min() >= 10. and max(a.max(), b.max()) >= 150.
            else:
                assert d['cparams'].abs().max() <= 3.
            assert d['actions_cont'].min() > 0. and d['actions_cont'].max() < 1.
        t = L.policy_terms(d, None if d['logits'] is None else d['logits'].double(), None if d['cparams'] is None else d['cparams'].double())
        m = t['mask'] > 0
        if c['special'] == 'equal_adv':                      # the masked variance is 0: max(var, eps) clamps
            adv = d['adv'][m]
            assert c['norm'] and (adv == adv[0]).all() and not (d['adv'] == adv[0]).all() and (t['adv'][m] == 0).all()
        if c['special'] == 'zero_adv':
            assert (d['adv'][m] == 0).sum() > 20
        if c['mask'] == 'zero':
            assert m.sum() == 0
        if c['degenerate']:
            continue
        r, adv = t['ratio'][m], t['adv'][m]
        out = (r < 1. - c['clip']) | (r > 1. + c['clip'])
        assert out.float().mean() >= 0.2 and (~out).float().mean() >= 0.2, (c['name'], out.float().mean().item())
        for side in (out, ~out):
            assert (adv[side] > 0).any() and (adv[side] < 0).any(), c['name']
        if c['kl'] != 'off':
            sizes = [n for n in c['sizes']] + [2] * c['nc']
            assert len(t['kls']) == len(sizes)
            for n, kl in zip(sizes, t['kls']):               # (a type with one option has one distribution: its KL is 0)
                assert n == 1 or kl[m].mean() >= 1e-2, (c['name'], n, kl[m].mean().item())
    va = LC.VALUE
    assert {(c['two_hot'], c['bins']) for c in va} == {(t, b) for t in (0, 1) for b in (20, 63, 64, 65, 255)} and {c['rows'] for c in va} == {1, 4, 5, 130}
    assert {(c['two_hot'], c['ldpad']) for c in va} == {(t, p) for t in (0, 1) for p in ('r4', 'p5')} and {(c['two_hot'], c['mask']) for c in va} == \
        {(t, m) for t in (0, 1) for m in ('rand', 'null', 'zero')}
    assert any(c['eps'] > 1 for c in va)
    for c in va:
        d = LC.value_inputs(c)
        assert LC.value_ld(c) >= c['bins'] and d['support'].numel() == c['bins'] + (0 if c['two_hot'] else 1) and d['support'].dtype == torch.float32
        assert d['mask'] is None or c['mask'] == 'zero' or d['mask'][:d['n_special']].all()
        if c['rows'] == 130:
            ret, sup = d['returns'], d['support']
            lo, hi = sup[0], sup[-1]
            assert (ret == lo).any() and (ret == hi).any() and (ret < lo).any() and (ret > hi).any() and ((ret > lo) & (ret < hi)).sum() > 100
            assert all((ret == s).any() for s in (sup[1], sup[-2], sup[c['bins'] // 2]))


@pytest.mark.parametrize('family', sorted(LC.FAMILIES))
def test_inputs_see_every_mutation_and_float32_stays_within_e32(family):
    table, inputs, expect, mutations = LC.FAMILIES[family]
    e32, bound = LC.E32[family], LC.BOUND[family]
    rows = []
    for c in table:
        d = inputs(c)
        ref = expect(c, d)
        assert all(torch.isfinite(x).all() for x in ref.values() if x is not None), c['name']
        rows.append((c['name'], L.err_all(expect(c, d, torch.float32), ref), {m: L.err_all(expect(c, d, mut=(m,)), ref) for m in mutations}))
    best = {m: max((mv[m], n) for n, _, mv in rows) for m in mutations}
    seen = {m for m, (v, _) in best.items() if v >= ROOM * bound}
    worst = max(rows, key=lambda r: r[1])
    print(f'{family}: E32 measured {worst[1]:.3e} ({worst[0]}), recorded {e32:.3e}, GPU bound {bound:.3e}; largest movement per mutation: '
          + ', '.join(f'{m} {v:.2e} ({n})' for m, (v, n) in sorted(best.items())))
    bad = [f'{n}: float32 evaluation {e:.3e} above the recorded E32 {e32:.3e}' for n, e, _ in rows if not e <= e32]
    assert not bad, '\n'.join(bad)
    assert worst[1] >= e32 / 2, 'the recorded E32 is more than twice what this table measures'
    assert seen == SEEN[family], (sorted(seen - SEEN[family]), sorted(SEEN[family] - seen))
    if family == 'policy_wide':                              # what the concentrated family cannot see, the main family does
        assert SEEN['policy_wide'] <= SEEN['policy']


def test_pmpo_sign_of_a_zero_advantage_is_inert():
    """`adv >= 0` against `adv > 0` cannot matter: PMPO weighs the row by |tanh(adv)|, which is 0 there.  Shown on the case with exact zeros, so
    that the one mutation of the list no input can see is known to be harmless rather than forgotten."""
    c = next(c for c in LC.POLICY if c['special'] == 'zero_adv')
    d = LC.policy_inputs(c)
    ref, got = LC.policy_expect(c, d), LC.policy_expect(c, d, mut=('pmpo_sign0',))
    assert c['obj'] == 'pmpo' and all(torch.equal(got[k], ref[k]) for k in ref if ref[k] is not None)


# ------------------------------------------------------------------------------------------------------------------- against oracle/restate.py
def _f32(x):
    return None if x is None else (x.float() if x.is_floating_point() else x)


@pytest.mark.parametrize('c', LC.GAE, ids=lambda c: c['name'])
def test_gae_reference_agrees_with_restate(c):
    d = LC.gae_inputs(c)
    B, T = c['B'], c['T']
    exp = dict(rewards=d['rewards'], values=d['values'], lens=torch.full((B,), T) if d['lens'] is None else d['lens'],
               is_truncated=torch.ones(B, dtype=torch.bool) if d['trunc'] is None else d['trunc'], terminals=torch.zeros(B, dtype=torch.bool) if d['term'] is None else d['term'])
    cfg = restate.Config(dim=8, dim_latent=4, num_latent_tokens=2, gae_discount_factor=c['gamma'], gae_lambda=c['lam'])
    ret, val, adv, mask = restate.returns_and_advantage(cfg, exp, normalize=False)
    ref = LC.gae_expect(c, d)
    assert L.err_all(dict(returns=ret, adv=adv, mask=mask.float()), ref) <= LC.BOUND['gae']


@pytest.mark.parametrize('c', LC.VALUE, ids=lambda c: c['name'])
def test_value_reference_agrees_with_restate(c):
    """restate builds the supports itself from the range and the bin count; the loss and its gradient follow from its target probabilities."""
    d = LC.value_inputs(c)
    cfg = restate.Config(dim=8, dim_latent=4, num_latent_tokens=2, hl_gauss_sigma_to_bin_ratio=0.75, hl_gauss_eps=c['eps'])
    vr = (c['vmin'], c['vmax'])
    tgt = restate.symexp_two_hot(d['returns'], vr, c['bins']) if c['two_hot'] else restate.hl_gauss_to_probs(cfg, d['returns'], vr, c['bins'])
    v = d['logits'].clone().requires_grad_()
    mask = torch.ones(c['rows']) if d['mask'] is None else d['mask']
    loss = (-(tgt * v.log_softmax(-1)).sum(-1) * mask).sum() / mask.sum().clamp(min=1.)
    loss.backward()
    assert L.err_all(dict(loss=loss.detach().reshape(1), dv=v.grad), LC.value_expect(c, d)) <= LC.BOUND['value']


@pytest.mark.parametrize('c', LC.POLICY + LC.POLICY_WIDE, ids=lambda c: c['name'])
def test_policy_reference_agrees_with_restate(c, monkeypatch):
    """restate.learn_losses in float32 with its heads replaced by this case's logits / raw parameters: B = rows trajectories of one step, values 0 and
    rewards = the advantages (so its GAE returns them), masked rows truncated.  restate defines the mean over an empty mask differently for the value
    branch only; the policy loss and its gradients are compared on every case."""
    d = LC.policy_inputs(c)
    R = c['rows']
    fam = 'policy_wide' if c['special'] == 'wide' else 'policy'
    mask = torch.ones(R) if d['mask'] is None else d['mask']
    logits = None if d['logits'] is None else d['logits'].clone().requires_grad_()
    cparams = None if d['cparams'] is None else d['cparams'].clone().requires_grad_()
    cfg = restate.Config(dim=8, dim_latent=4, num_latent_tokens=2, num_discrete_actions=c['sizes'], num_continuous_actions=c['nc'], ppo_eps_clip=c['clip'],
                         policy_entropy_weight=c['ent_w'], pmpo_pos_to_neg_weight=c['pmpo_alpha'], pmpo_reverse_kl=c['kl'] == 'rev', pmpo_kl_div_loss_weight=c['kl_w'],
                         value_num_bins=4, continuous_beta_param=c['link'] + '_p1')
    assert cfg.num_discrete_actions == tuple(n for n in c['sizes'])
    monkeypatch.setattr(restate, 'policy_head', lambda cfg, W, ae: ae)
    monkeypatch.setattr(restate, 'policy_logits', lambda cfg, W, pe: logits[:, None])
    monkeypatch.setattr(restate, 'policy_cont_params', lambda cfg, W, pe: cparams.reshape(R, 1, c['nc'], 2))
    monkeypatch.setattr(restate, 'value_head_bins', lambda cfg, W, ae: torch.zeros(R, 1, 4))
    un = lambda x: None if x is None else x[:, None]
    exp = dict(rewards=d['adv'][:, None], values=torch.zeros(R, 1), lens=torch.ones(R, dtype=torch.long), is_truncated=mask == 0, terminals=torch.zeros(R, dtype=torch.bool),
               agent_embed=torch.zeros(R, 1, 8), actions=un(d['actions']), log_probs=un(d['old_lp']), old_action_unembeds=un(d['old_logits']),
               actions_cont=un(d['actions_cont']), log_probs_cont=un(d['old_lp_cont']), old_cont_params=un(d['old_cparams']))
    pl, _ = restate.learn_losses(cfg, {}, exp, c['obj'], use_delight_gating=c['gate'] > 0, delight_temperature=c['gate'] or 1., normalize_advantages=bool(c['norm']),
                                 eps=c['eps'])
    leaves = [x for x in (logits, cparams) if x is not None]
    grads = list(torch.autograd.grad(pl, leaves)) if pl.requires_grad else [torch.zeros_like(x) for x in leaves]
    ref = LC.policy_expect(c, d)
    got = dict(loss=pl.detach().reshape(1), dlogits=grads.pop(0) if logits is not None else None, dcparams=grads.pop(0) if cparams is not None else None)
    assert L.err_all(got, {k: ref[k] for k in got}) <= LC.BOUND[fam]
