"""GPU: the learner's loss kernels of csrc/learn.hip (gae_kernel; policy_loss_kernel with the three reduce1_kernel modes and
finalize_losses_kernel; value_loss_kernel), one operator call per case through the C-ABI entry points d4_gae_adv / d4_policy_loss /
d4_hl_gauss_ce, each against the plain float64 reference of tests/learn_ref.py.  Every policy case is off-policy: the behaviour
log-probs, old logits and old Beta parameters differ from the current ones (tests/learn_cases.py; the host test asserts by how much).

A case asserts
  * the values: max |out - float64| <= BOUND[family] x max |float64| for the loss, dlogits, dcparams, the three per-row terms, returns / adv /
    mask and dv (an output whose reference is zero everywhere — an all-zero mask, the KL term without a KL — must be zero exactly);
  * untouched memory: every operand and output lies between NaN guards with NaN in the gaps of its padded rows; nothing outside [rows][ld] is
    written, the pad columns total .. ld and 2 nc .. ldc are exactly 0, and a read past a row (or, for the GAE, past `len`: NaN there) poisons
    the output.
Further tests: d4_policy_loss on the learner's own buffers gives d4_learn's dlogits bit for bit; every refusal returns its error and launches
nothing (the outputs stay NaN); the last test prints each family's worst error as a fraction of its bound.

Tolerance (learn_cases.py): E32 = float32 against float64 evaluation of the same reference on the CPU, worst case of the family, recorded with
25 % headroom; the GPU bound is 8 x E32, relative to the output's max-abs:
    family        measured E32   recorded E32   bound (8 x)
    gae           2.1e-7         2.6e-7         2.1e-6
    policy        9.5e-6         1.2e-5         9.6e-5
    policy_wide   6.6e-4         8.3e-4         6.6e-3       (alpha, beta in the tens to hundreds: lgamma(a + b) - lgamma(a) - lgamma(b) cancels)
    value         3.4e-7         4.3e-7         3.4e-6"""
import ctypes as C

import pytest
import torch

import learn_cases as LC
import learn_ref as L
from dreamer4_amd import _lib
from test_gpu_attn_cores import DEV, GUARD, Buf, bits, stream
from test_gpu_glue import flat_in, out_buf, rows_in

pytestmark = pytest.mark.gpu

WORST = {}                       # family -> (error / bound, what)


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def note(family, name, what, err):
    bound = LC.BOUND[family]
    print(f'{family} {name} {what}: err {err:.3e} (bound {bound:.3e})')
    if family not in WORST or err / bound > WORST[family][0]:
        WORST[family] = (err / bound, f'{name} {what}: {err:.3e} of {bound:.3e}')


def check(family, name, what, buf, ref, ld=None):
    """buf holds ref [rows, cols] at leading dimension ld (flat: ld None): within the family's bound of it, the pad columns exactly 0, everything
    else of the buffer still NaN."""
    ref = ref.reshape(1, -1) if ld is None else ref
    rows, cols = ref.shape
    ld = cols if ld is None else ld
    got = buf.dev.cpu()
    inside = torch.zeros(got.numel(), dtype=torch.bool)
    inside.as_strided((rows, ld), (ld, 1), GUARD + buf.off).fill_(True)
    assert got[~inside].isnan().all(), f'{what}: {int((~got[~inside].isnan()).sum())} elements written outside [rows][ld]'
    g = got.as_strided((rows, ld), (ld, 1), GUARD + buf.off)
    assert not g.isnan().any(), f'{what}: NaN in the output (an operand gap or an element past `len` was read, or an element was not written)'
    assert (g[:, cols:] == 0).all(), f'{what}: the pad columns are not zero'
    err = L.err(g[:, :cols], ref)
    note(family, name, what, err)
    assert err <= LC.BOUND[family], f'{name} {what}: error {err:.3e} above the bound {LC.BOUND[family]:.3e}'


def untouched(*bufs):
    for b in bufs:
        assert b.dev.isnan().all(), 'a refused call wrote to an output'


def dev(x, dtype=None):
    return None if x is None else (x if dtype is None else x.to(dtype)).contiguous().to(DEV)


def ptr(x):
    return None if x is None else (x.ptr if isinstance(x, Buf) else C.c_void_p(x.data_ptr()))


# ------------------------------------------------------------------------------------------------------------------- GAE
def gae_call(lib, c, d, **over):
    B, T = c['B'], c['T']
    a = dict(rewards=flat_in(d['rewards']), values=flat_in(d['values']), lens=dev(d['lens'], torch.int64), trunc=dev(d['trunc'], torch.uint8),
             term=dev(d['term'], torch.uint8), B=B, T=T, returns=out_buf(B * T), adv=out_buf(B * T), mask=out_buf(B * T))
    a.update(over)
    rc = lib.d4_gae_adv(ptr(a['rewards']), ptr(a['values']), ptr(a['lens']), ptr(a['trunc']), ptr(a['term']), c['gamma'], c['lam'], a['B'], a['T'], ptr(a['returns']),
                        ptr(a['adv']), ptr(a['mask']), stream())
    torch.cuda.synchronize()
    return rc, a


@pytest.mark.parametrize('c', LC.GAE, ids=[c['name'] for c in LC.GAE])
def test_gae_adv(lib, c):
    d = LC.gae_inputs(c)
    rc, a = gae_call(lib, c, d)
    _lib.check(rc)
    ref = LC.gae_expect(c, d)
    for k in ('returns', 'adv', 'mask'):
        check('gae', c['name'], k, a[k], ref[k].reshape(1, -1))
    assert torch.equal(a['mask'].dev.cpu()[GUARD:-GUARD].double(), ref['mask'].reshape(-1))             # the mask is 0 / 1, exactly


def test_gae_returns_are_those_of_d4_gae(lib):
    c = LC.GAE[-2]
    d = LC.gae_inputs(c)
    rc, a = gae_call(lib, c, d)
    _lib.check(rc)
    ret = out_buf(c['B'] * c['T'])
    _lib.check(lib.d4_gae(ptr(a['rewards']), ptr(a['values']), ptr(a['lens']), ptr(a['trunc']), ptr(a['term']), c['gamma'], c['lam'], c['B'], c['T'], ret.ptr, stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(ret.dev.cpu()), bits(a['returns'].dev.cpu()))


def test_gae_adv_refusals(lib):
    c = LC.GAE[4]
    d = LC.gae_inputs(c)
    for over in (dict(rewards=None), dict(values=None), dict(returns=None), dict(adv=None), dict(mask=None), dict(B=0), dict(T=0)):
        rc, a = gae_call(lib, c, d, **over)
        assert rc != 0 and 'd4_gae_adv' in lib.d4_last_error().decode(), over
        untouched(*[a[k] for k in ('returns', 'adv', 'mask') if a[k] is not None])


# ------------------------------------------------------------------------------------------------------------------- policy loss
def policy_call(lib, c, d, **over):
    R, sizes, nc = c['rows'], c['sizes'], c['nc']
    A, na = sum(sizes), len(sizes)
    ld, ldc = LC.policy_pads(c)
    ldo = A + 1
    nan_rows = lambda n, w: out_buf(n * w)               # an operand of a part that is not in use: never read, NaN throughout
    a = dict(logits=rows_in(d['logits'], ld) if na else nan_rows(R, ld), ld=ld, actions=dev(d['actions']), old_lp=flat_in(d['old_lp']) if na else None,
             old_logits=rows_in(d['old_logits'], ldo) if d['old_logits'] is not None else None, ldo=ldo, adv=flat_in(d['adv']),
             mask=flat_in(d['mask']) if d['mask'] is not None else None, sizes=dev(torch.tensor(sizes, dtype=torch.int32)) if na else None, rows=R, na=na, total=A,
             cparams=rows_in(d['cparams'], ldc) if nc else nan_rows(R, ldc), ldc=ldc, actions_cont=flat_in(d['actions_cont']) if nc else None,
             old_lp_cont=flat_in(d['old_lp_cont']) if nc else None, old_cparams=flat_in(d['old_cparams']) if d['old_cparams'] is not None else None, nc=nc,
             beta_param=int(c['link'] == 'exp'), objective=d['objective'], normalize=d['normalize'], use_gate=d['use_gate'], reverse_kl=d['reverse_kl'], eps=d['eps'],
             clip=d['clip'], ent_w=d['ent_w'], gate_temp=d['gate_temp'], pmpo_alpha=d['pmpo_alpha'], kl_w=d['kl_w'],
             loss=out_buf(1), dlogits=out_buf(R * ld), dcparams=out_buf(R * ldc), row_pl=out_buf(R), row_ent=out_buf(R), row_aux=out_buf(R), scratch=out_buf(R + 64))
    a.update(over)
    desc = _lib.PolicyLossDesc()
    for k, v in a.items():
        k = {'old_lp': 'old_log_probs', 'old_lp_cont': 'old_log_probs_cont', 'adv': 'advantages', 'sizes': 'action_sizes'}.get(k, k)
        setattr(desc, k, v if isinstance(v, (int, float)) else ptr(v))
    rc = lib.d4_policy_loss(C.byref(desc), stream())
    torch.cuda.synchronize()
    return rc, a


OUTPUTS = ('loss', 'dlogits', 'dcparams', 'row_pl', 'row_ent', 'row_aux')


def policy_case(lib, c, family):
    d = LC.policy_inputs(c)
    rc, a = policy_call(lib, c, d)
    _lib.check(rc)
    ref = LC.policy_expect(c, d)
    R, A, nc = c['rows'], sum(c['sizes']), c['nc']
    check(family, c['name'], 'loss', a['loss'], ref['loss'])
    check(family, c['name'], 'dlogits', a['dlogits'], ref['dlogits'] if A else torch.zeros(R, 0, dtype=torch.float64), a['ld'])
    check(family, c['name'], 'dcparams', a['dcparams'], ref['dcparams'] if nc else torch.zeros(R, 0, dtype=torch.float64), a['ldc'])
    for k in ('row_pl', 'row_ent', 'row_aux'):
        check(family, c['name'], k, a[k], ref[k])
    g = a['scratch'].dev.cpu()
    assert g[:GUARD].isnan().all() and g[-GUARD:].isnan().all(), 'written outside the scratch'


@pytest.mark.parametrize('c', LC.POLICY, ids=[c['name'] for c in LC.POLICY])
def test_policy_loss(lib, c):
    policy_case(lib, c, 'policy')


@pytest.mark.parametrize('c', LC.POLICY_WIDE, ids=[c['name'] for c in LC.POLICY_WIDE])
def test_policy_loss_concentrated_beta(lib, c):
    policy_case(lib, c, 'policy_wide')


def test_policy_loss_refusals(lib):
    """Each returns its error and launches nothing: the outputs are still NaN."""
    c = next(c for c in LC.POLICY if c['kl'] == 'fwd' and len(c['sizes']) == 3 and c['nc'] == 3 and c['rows'] == 300)
    d = LC.policy_inputs(c)
    A = sum(c['sizes'])
    overs = [dict(ld=A - 1), dict(ldc=2 * c['nc'] - 1), dict(old_logits=None), dict(old_cparams=None), dict(ldo=A - 1), dict(objective=3), dict(objective=-1),
             dict(rows=0), dict(beta_param=2), dict(use_gate=1, gate_temp=0.)]
    overs += [{k: None} for k in ('logits', 'actions', 'old_lp', 'sizes', 'adv', 'cparams', 'actions_cont', 'old_lp_cont', 'loss', 'dlogits', 'dcparams', 'row_pl', 'row_ent',
                                  'row_aux', 'scratch')]
    for over in overs:
        rc, a = policy_call(lib, c, d, **over)
        assert rc != 0 and 'd4_policy_loss' in lib.d4_last_error().decode(), over
        untouched(*[a[k] for k in OUTPUTS + ('scratch',) if a[k] is not None])
    assert lib.d4_policy_loss(None, stream()) != 0
    rc, a = policy_call(lib, c, d, kl_w=0., old_logits=None, old_cparams=None)          # without a KL weight the old parameters may be null
    _lib.check(rc)
    rc, a = policy_call(lib, c, d, objective=0, old_logits=None, old_cparams=None)      # ... and kl_w is read under pmpo only
    _lib.check(rc)
    assert (a['row_aux'].dev.cpu()[GUARD:-GUARD] == 0).all()


def test_stateless_policy_loss_is_d4_learn_bit_for_bit(lib):
    """d4_policy_loss on the learner's own logits, advantages and mask (d4_debug_buffer) writes the dlogits d4_learn wrote, bit for bit, and the same
    policy loss: both run one sequence (policy_loss_run of csrc/learn.hip)."""
    from dreamer4_amd.learner import run_learner
    from util import make_noise, oracle_config, small_model
    m = small_model(num_discrete_actions=(3, 2)).cuda()
    B, T = 5, 6
    e = m.generate(T, batch_size=B, return_for_policy_optimization=True, noise=make_noise(oracle_config(m), T, B, 77))
    with torch.no_grad():          # off-policy: the heads move after the rollout
        for k, p in m.named_parameters():
            if k.startswith(('policy_head', 'action_embedder.discrete_action_unembed')) and p.numel():
                p.add_(0.02 * p.abs().mean() * torch.randn_like(p))
    R, A, na, Apad = B * T, 5, 2, 8
    for objective in ('ppo', 'spo', 'pmpo'):
        losses, _ = run_learner(m, e, objective=objective)
        torch.cuda.synchronize()

        ptrs = {}
        for n in ('l_logits', 'l_dlogits', 'l_adv', 'l_mask'):
            ptrs[n] = C.c_void_p()
            _lib.check(lib.d4_debug_buffer(m._engine, n.encode(), C.byref(ptrs[n])))
        want = torch.empty(R * Apad, device=DEV)                # the learner's dlogits, copied out before the stateless call
        _lib.check(lib.d4_copy_rows(ptrs['l_dlogits'], Apad, C.c_void_p(want.data_ptr()), Apad, R, Apad, stream()))
        exp = e.to(DEV)
        lenT = exp.agent_embed.shape[1]
        a = dict(actions=exp.actions.discrete[:, -lenT:].reshape(R, na).long().contiguous(), old_lp=exp.log_probs.discrete[:, -lenT:].reshape(R, na).float().contiguous(),
                 old_logits=exp.old_action_unembeds.discrete[:, -lenT:].reshape(R, A).float().contiguous(), sizes=torch.tensor([3, 2], dtype=torch.int32, device=DEV))
        out = dict(loss=out_buf(1), dlogits=out_buf(R * Apad), row_pl=out_buf(R), row_ent=out_buf(R), row_aux=out_buf(R), scratch=out_buf(R + 64))
        desc = _lib.PolicyLossDesc()
        desc.logits, desc.ld, desc.actions, desc.old_log_probs, desc.old_logits, desc.ldo = ptrs['l_logits'], Apad, ptr(a['actions']), ptr(a['old_lp']), ptr(a['old_logits']), A
        desc.advantages, desc.mask, desc.action_sizes, desc.rows, desc.na, desc.total = ptrs['l_adv'], ptrs['l_mask'], ptr(a['sizes']), R, na, A
        desc.objective, desc.normalize, desc.use_gate, desc.reverse_kl = {'ppo': 0, 'spo': 1, 'pmpo': 2}[objective], int(objective != 'pmpo'), int(m.use_delight_gating), int(m.pmpo_reverse_kl)
        desc.eps, desc.clip, desc.ent_w, desc.gate_temp, desc.pmpo_alpha, desc.kl_w = 1e-6, m.ppo_eps_clip, m.policy_entropy_weight, m.delight_temperature, m.pmpo_pos_to_neg_weight, m.pmpo_kl_div_loss_weight
        for k, v in out.items():
            setattr(desc, k, v.ptr)
        _lib.check(lib.d4_policy_loss(C.byref(desc), stream()))
        torch.cuda.synchronize()
        got = out['dlogits'].dev[GUARD:-GUARD]
        assert want.abs().max() > 0 and torch.equal(bits(got.cpu()), bits(want.cpu())), objective
        assert torch.equal(bits(out['loss'].dev[GUARD:GUARD + 1].cpu()), bits(losses[:1].cpu())), objective


# ------------------------------------------------------------------------------------------------------------------- value loss
def value_call(lib, c, d, **over):
    R, bins, ld = c['rows'], c['bins'], LC.value_ld(c)
    a = dict(logits=rows_in(d['logits'], ld), ld=ld, returns=flat_in(d['returns']), mask=flat_in(d['mask']) if d['mask'] is not None else None, support=flat_in(d['support']),
             rows=R, bins=bins, loss=out_buf(1), dv=out_buf(R * ld), scratch=out_buf(2 * R + 64))
    a.update(over)
    rc = lib.d4_hl_gauss_ce(ptr(a['logits']), a['ld'], ptr(a['returns']), ptr(a['mask']), ptr(a['support']), a['rows'], a['bins'], c['vmin'], c['vmax'], c['sigma'], c['eps'],
                            c['two_hot'], ptr(a['loss']), ptr(a['dv']), ptr(a['scratch']), stream())
    torch.cuda.synchronize()
    return rc, a


@pytest.mark.parametrize('c', LC.VALUE, ids=[c['name'] for c in LC.VALUE])
def test_value_loss(lib, c):
    d = LC.value_inputs(c)
    rc, a = value_call(lib, c, d)
    _lib.check(rc)
    ref = LC.value_expect(c, d)
    check('value', c['name'], 'loss', a['loss'], ref['loss'])
    check('value', c['name'], 'dv', a['dv'], ref['dv'], a['ld'])
    g = a['scratch'].dev.cpu()
    assert g[:GUARD].isnan().all() and g[-GUARD:].isnan().all(), 'written outside the scratch'


def test_value_loss_refusals(lib):
    c = LC.VALUE[1]
    d = LC.value_inputs(c)
    for over in (dict(ld=c['bins'] - 1), dict(rows=0), dict(bins=0), dict(logits=None), dict(returns=None), dict(support=None), dict(loss=None), dict(dv=None), dict(scratch=None)):
        rc, a = value_call(lib, c, d, **over)
        assert rc != 0 and 'd4_hl_gauss_ce' in lib.d4_last_error().decode(), over
        untouched(*[a[k] for k in ('loss', 'dv', 'scratch') if a[k] is not None])


def test_worst_errors_as_fractions_of_their_bounds():
    assert set(WORST) == set(LC.FAMILIES), 'a family ran no case'
    for f in sorted(WORST):
        print(f'{f}: worst error {WORST[f][0]:.3f} of its bound ({WORST[f][1]})')
    assert all(v[0] <= 1. for v in WORST.values())
