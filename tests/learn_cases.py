"""Case tables of tests/test_gpu_learn_ops.py (the learner's loss kernels of csrc/learn.hip called alone through d4_gae_adv, d4_policy_loss and
d4_hl_gauss_ce) and of tests/test_learn_ops_host.py, which shows on the CPU that these inputs and bounds can see the errors the GPU tests are
for.  Seeds are this table's own (30000 ..), disjoint from every other table's.

Every policy case is OFF-policy: the behaviour log-probs, old logits and old Beta parameters come from logits / raw parameters perturbed by
noise (`noise`, `noise_c`), the stored actions are drawn from that behaviour policy.  The host test asserts from the float64 reference that
each non-degenerate case has at least 20 % of its unmasked rows outside the clip band and 20 % inside, both advantage signs on either side, and,
with a KL term, a mean KL of at least 1e-2 per action type.

Tolerance, by the rule of glue_cases.py: E32 = float32 against float64 evaluation of the reference on the CPU, worst case of the family, recorded
with 25 % headroom; the GPU bound is FACTOR (8) x E32 relative to each output's max-abs.
    family        measured E32   recorded E32   bound (8 x)
    gae           2.1e-7         2.6e-7         2.1e-6
    policy        9.5e-6         1.2e-5         9.6e-5
    policy_wide   6.6e-4         8.3e-4         6.6e-3       (alpha, beta in the tens to hundreds: lgamma(a + b) - lgamma(a) - lgamma(b) cancels)
    value         3.4e-7         4.3e-7         3.4e-6"""
import itertools
import math

import torch

import learn_ref as L

FACTOR = 8
E32 = {'gae': 2.6e-7, 'policy': 1.2e-5, 'policy_wide': 8.3e-4, 'value': 4.3e-7}
BOUND = {f: FACTOR * e for f, e in E32.items()}
CLIP = 0.2


def _seed(table, base):
    for i, c in enumerate(table):
        c['seed'] = base + i
    return table


def _gen(c, k=0):
    return torch.Generator().manual_seed(c['seed'] * 16 + k)


# ------------------------------------------------------------------------------------------------------------------- GAE
def _g(B, T, lens, trunc, term):
    return dict(name=f'gae-B{B}-T{T}-lens_{lens}-trunc_{trunc}-term_{term}', B=B, T=T, lens=lens, trunc=trunc, term=term, gamma=0.97, lam=0.9)


GAE = _seed([_g(1, 1, 'null', 'null', 'null'), _g(1, 7, 'mixed', 'mixed', 'mixed'), _g(5, 1, 'mixed', 'mixed', 'null'), _g(5, 2, 'mixed', 'null', 'mixed'),
             _g(5, 7, 'null', 'mixed', 'mixed'), _g(5, 7, 'mixed', 'null', 'null'), _g(5, 33, 'mixed', 'mixed', 'mixed'), _g(130, 1, 'null', 'mixed', 'mixed'),
             _g(130, 2, 'mixed', 'mixed', 'null'), _g(130, 7, 'mixed', 'mixed', 'mixed'), _g(130, 33, 'mixed', 'mixed', 'mixed'), _g(130, 33, 'null', 'null', 'null')], 30000)


def gae_inputs(c):
    """rewards, values [B, T] with NaN past `len`; lens (1, T and values between) / is_truncated / terminals or None."""
    g = _gen(c)
    B, T = c['B'], c['T']
    r, v = torch.randn(B, T, generator=g), 2. * torch.randn(B, T, generator=g)
    lens = trunc = term = None
    if c['lens'] == 'mixed':
        lens = torch.randint(1, T + 1, (B,), generator=g)
        lens[0] = 1 if B > 1 or T == 1 else max(1, T // 2)
        if B > 1:
            lens[1] = T
        past = torch.arange(T) >= lens[:, None]
        r[past], v[past] = math.nan, math.nan
    if c['trunc'] == 'mixed':
        trunc = torch.rand(B, generator=g) < 0.5
        trunc[-1] = False
        if B > 1:
            trunc[0] = True
    if c['term'] == 'mixed':
        term = torch.rand(B, generator=g) < 0.5
        term[-1] = True
        if B > 1:
            term[0] = False
    return dict(rewards=r, values=v, lens=lens, trunc=trunc, term=term)


def gae_expect(c, d, dtype=torch.float64, mut=()):
    return L.gae_ref(d['rewards'], d['values'], d['lens'], d['trunc'], d['term'], c['gamma'], c['lam'], dtype, mut)


# ------------------------------------------------------------------------------------------------------------------- policy loss
SIZES = ((4,), (3, 5, 2), (1,), (17,), ())
OBJ = {'ppo': 0, 'spo': 1, 'pmpo': 2}


def _p(rows, sizes, nc, link, ldpad, obj, gate, norm, mask='rand', kl='off', special=None, noise=None, noise_c=None, degenerate=False):
    if nc == 0 and sizes in ((), (1,)):
        nc = 1
    n = len([s for s in sizes if s > 1]) + nc
    c = dict(rows=rows, sizes=tuple(sizes), nc=nc, link=link, ldpad=ldpad, obj=obj, gate=gate, norm=norm, mask=mask, kl=kl, special=special,
             noise=(0.5 if kl != 'off' else 0.55 / math.sqrt(n)) if noise is None else noise,
             noise_c=(0.5 if link == 'exp' else 1.0) * (1.3 if kl != 'off' else 1.) / math.sqrt(n) if noise_c is None else noise_c,
             degenerate=degenerate or rows < 128 or mask == 'zero' or special == 'equal_adv', clip=CLIP, ent_w=0.05, pmpo_alpha=1.5, kl_w=0.3 if kl != 'off' else 0.,
             eps=1e-6)
    c['name'] = (f"policy-{obj}-R{rows}-a{'_'.join(map(str, sizes)) or 'none'}-nc{nc}{link[0]}-{ldpad}-gate{gate:g}-norm{norm}-mask_{mask}-kl_{kl}"
                 + (f'-{special}' if special else ''))
    return c


def _cross():
    out = []
    for i, (obj, gate, norm) in enumerate(itertools.product(('ppo', 'spo', 'pmpo'), (0., 1., 2.5), (0, 1))):
        kl = ('fwd', 'rev', 'off')[(i // 2) % 3] if obj == 'pmpo' else 'off'
        out.append(_p((128, 129, 300)[i % 3], SIZES[i % 5], (0, 1, 3)[(i // 2 + i) % 3], ('softplus', 'exp')[(i // 3) % 2], ('apad', 'p3')[i % 2], obj, gate, norm, kl=kl))
    return out


POLICY = _seed(_cross() + [
    _p(1, (4,), 0, 'softplus', 'apad', 'ppo', 1., 0), _p(1, (3, 5, 2), 3, 'exp', 'p3', 'pmpo', 1., 1, kl='fwd'), _p(1, (), 1, 'softplus', 'apad', 'spo', 0., 0, mask='null'),
    _p(129, (3, 5, 2), 3, 'exp', 'p3', 'ppo', 1., 1, special='equal_adv'), _p(129, (3, 5, 2), 1, 'softplus', 'apad', 'pmpo', 1., 1, special='equal_adv', kl='rev'),
    _p(129, (4,), 1, 'softplus', 'apad', 'spo', 1., 1, mask='zero'), _p(130, (3, 5, 2), 3, 'softplus', 'p3', 'pmpo', 1., 0, mask='zero', kl='fwd'),
    _p(300, (3, 5, 2), 1, 'exp', 'apad', 'ppo', 2.5, 1, mask='null'),
    _p(300, (3, 5, 2), 3, 'softplus', 'apad', 'pmpo', 1., 0, kl='fwd'), _p(300, (3, 5, 2), 3, 'exp', 'p3', 'pmpo', 0., 1, kl='rev'),
    _p(300, (17,), 3, 'exp', 'apad', 'pmpo', 1., 0, kl='fwd'), _p(129, (4,), 3, 'softplus', 'p3', 'pmpo', 2.5, 0, kl='rev'),
    _p(129, (3, 5, 2), 1, 'softplus', 'p3', 'pmpo', 1., 0, kl='off'),
    _p(129, (3, 5, 2), 0, 'softplus', 'apad', 'ppo', 1., 1, special='shift90'), _p(129, (17,), 0, 'softplus', 'p3', 'pmpo', 0., 0, special='shift90', kl='fwd'),
    _p(300, (4,), 0, 'softplus', 'apad', 'pmpo', 0., 0, special='zero_adv'),
    _p(128, (3, 5, 2), 0, 'softplus', 'p3', 'pmpo', 1., 0, kl='rev'), _p(129, (), 3, 'exp', 'p3', 'pmpo', 1., 1, kl='fwd'),
], 30100)

# alpha, beta in the tens to hundreds: a family of its own, with its own bound
POLICY_WIDE = _seed([_p(300, (), 1, 'softplus', 'apad', 'ppo', 0., 0, special='wide'), _p(129, (4,), 3, 'exp', 'p3', 'spo', 1., 1, special='wide'),
                     _p(300, (3, 5, 2), 3, 'softplus', 'p3', 'pmpo', 1., 0, special='wide', kl='fwd'), _p(128, (), 3, 'exp', 'apad', 'pmpo', 0., 1, special='wide', kl='rev')], 30200)


def policy_pads(c):
    """(ld, ldc): the learner's Apad / Cpad, or total + 3 / 2 nc + 3"""
    A, C2 = sum(c['sizes']), 2 * c['nc']
    if c['ldpad'] == 'apad':
        return (A + 3) // 4 * 4 + (4 if A == 0 else 0), (C2 + 3) // 4 * 4 + (4 if C2 == 0 else 0)
    return A + 3, C2 + 3


def policy_inputs(c):
    """The arguments of one call as L.policy_ref reads them, every tensor float32 (indices int64)."""
    g = _gen(c)
    R, sizes, nc, wide = c['rows'], c['sizes'], c['nc'], c['special'] == 'wide'
    A = sum(sizes)
    f32 = lambda x: x.double().float()
    p = dict(rows=R, sizes=sizes, nc=nc, link=c['link'], objective=OBJ[c['obj']], normalize=c['norm'], eps=c['eps'], use_gate=int(c['gate'] > 0), gate_temp=c['gate'] or 1.,
             pmpo_alpha=c['pmpo_alpha'], kl_w=c['kl_w'], reverse_kl=int(c['kl'] == 'rev'), clip=c['clip'], ent_w=c['ent_w'],
             logits=None, actions=None, old_lp=None, old_logits=None, cparams=None, actions_cont=None, old_lp_cont=None, old_cparams=None)
    if A:
        logits = 3. * torch.randn(R, A, generator=g)
        if c['special'] == 'shift90':
            logits[R // 2] += 90.
        old = logits + c['noise'] * torch.randn(R, A, generator=g)
        acts, olp, o = [], [], 0
        for n in sizes:
            ls = torch.log_softmax(old[:, o:o + n].double(), -1)
            a = torch.multinomial(ls.exp(), 1, generator=g)
            acts.append(a); olp.append(ls.gather(1, a))
            o += n
        p.update(logits=logits, actions=torch.cat(acts, 1), old_lp=f32(torch.cat(olp, 1)), old_logits=old if c['kl'] != 'off' else None)
    if nc:
        if wide:            # alpha, beta = 13 .. 300
            raw = 20. + 280. * torch.rand(R, 2 * nc, generator=g) if c['link'] == 'softplus' else 2.5 + 3. * torch.rand(R, 2 * nc, generator=g)
            step = c['noise_c'] * torch.randn(R, 2 * nc, generator=g)
            old = raw * (1. + 0.06 * step) if c['link'] == 'softplus' else raw + 0.12 * step
        else:               # raw parameters in [-3, 3]
            raw = 6. * torch.rand(R, 2 * nc, generator=g) - 3.
            old = raw + c['noise_c'] * torch.randn(R, 2 * nc, generator=g)
        old = old.reshape(R, nc, 2)
        a, b = L.beta_ab(old.double(), c['link'])
        mean, std = a / (a + b), torch.sqrt(a * b / ((a + b) ** 2 * (a + b + 1.)))
        x = f32((mean + 0.8 * std * torch.randn(R, nc, generator=g).double()).clamp(0.02, 0.98))
        p.update(cparams=raw, actions_cont=x, old_lp_cont=f32(L.beta_log_prob(a, b, x.double())), old_cparams=old.contiguous() if c['kl'] != 'off' else None)
    adv = 0.3 + torch.randn(R, generator=g)
    if c['special'] == 'equal_adv':
        adv = torch.full((R,), 0.75)
    if c['special'] == 'zero_adv':
        adv[::3] = 0.
    mask = {'rand': (torch.rand(R, generator=g) < 0.7).float(), 'null': None, 'zero': torch.zeros(R)}[c['mask']]
    if c['mask'] == 'rand':
        mask[-1] = 1.
        if c['special'] == 'equal_adv':                   # the masked advantages are equal, the others are not: an unmasked variance would differ
            adv = torch.where(mask > 0, adv, torch.randn(R, generator=g))
    p.update(adv=adv, mask=mask)
    return p


def policy_expect(c, d, dtype=torch.float64, mut=()):
    return L.policy_ref(d, dtype, mut)


# ------------------------------------------------------------------------------------------------------------------- value loss
VMIN, VMAX = -3., 5.


def _v(two_hot, bins, rows, ldpad, mask='rand', eps=1e-10):
    return dict(name=f"value-{'twohot' if two_hot else 'hlgauss'}-bins{bins}-R{rows}-{ldpad}-mask_{mask}" + ('-eps1.5' if eps > 1 else ''), two_hot=two_hot, bins=bins,
                rows=rows, ldpad=ldpad, mask=mask, eps=eps, vmin=VMIN, vmax=VMAX, sigma=0.75 * (VMAX - VMIN) / bins)


VALUE = _seed([_v(th, b, r, lp, m) for (th, b), r, lp, m in zip(itertools.product((0, 1), (20, 63, 64, 65, 255)), (130, 5, 4, 1, 5, 5, 130, 4, 5, 1),
                                                               ('r4', 'p5') * 5, ('rand', 'null', 'rand', 'rand', 'zero', 'rand', 'rand', 'null', 'zero', 'rand'))]
              + [_v(0, 65, 130, 'p5', eps=1.5), _v(1, 255, 130, 'r4', 'null'), _v(0, 20, 5, 'r4', 'rand'), _v(1, 20, 4, 'r4', 'rand')], 30300)


def value_ld(c):
    return (c['bins'] + 3) // 4 * 4 if c['ldpad'] == 'r4' else c['bins'] + 5


def value_support(c):
    """float32: the [bins + 1] edges of HL-Gauss, or the [bins] symexp bin values of two-hot"""
    if c['two_hot']:
        v = torch.linspace(c['vmin'], c['vmax'], c['bins'])
        return v.sign() * (torch.exp(v.abs()) - 1.)
    return torch.linspace(c['vmin'], c['vmax'], c['bins'] + 1)


def value_inputs(c):
    """Returns: exactly on the ends of the range, beyond both, exactly on a bin edge / bin value (the first and the last included), the rest spread
    inside.  The special values come first (rotated by the seed where the rows are few) and are never masked."""
    g = _gen(c)
    R, bins = c['rows'], c['bins']
    sup = value_support(c)
    lo, hi = (sup[0].item(), sup[-1].item()) if c['two_hot'] else (c['vmin'], c['vmax'])
    special = [hi, lo, hi + 5., lo - 3., sup[bins // 2].item(), sup[1].item(), sup[-2].item(), sup[bins // 3].item()]
    k = c['seed'] % len(special)
    special = special[k:] + special[:k]
    ret = lo + (hi - lo) * torch.rand(R, generator=g)
    n = min(len(special), R if R < 4 else max(4, R - 1))
    ret[:n] = torch.tensor(special[:n])
    mask = {'rand': (torch.rand(R, generator=g) < 0.7).float(), 'null': None, 'zero': torch.zeros(R)}[c['mask']]
    if c['mask'] == 'rand':
        mask[:n] = 1.
        mask[-1] = 1.
    return dict(logits=2. * torch.randn(R, bins, generator=g), returns=ret, mask=mask, support=sup, vmin=c['vmin'], vmax=c['vmax'], sigma=c['sigma'], eps=c['eps'],
                two_hot=c['two_hot'], n_special=n)


def value_expect(c, d, dtype=torch.float64, mut=()):
    return L.value_ref(d, dtype, mut)


FAMILIES = {'gae': (GAE, gae_inputs, gae_expect, L.GAE_MUTATIONS), 'policy': (POLICY, policy_inputs, policy_expect, L.POLICY_MUTATIONS),
            'policy_wide': (POLICY_WIDE, policy_inputs, policy_expect, L.POLICY_MUTATIONS), 'value': (VALUE, value_inputs, value_expect, L.VALUE_MUTATIONS)}
ALL_TABLES = {f: t[0] for f, t in FAMILIES.items()}
