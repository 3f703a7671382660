"""Case tables of tests/test_gpu_learn_norm_ops.py (return_stats_kernel and value_loss_clip_kernel of csrc/learn.hip called alone through
d4_return_stats and d4_value_loss) and of tests/test_learn_norm_host.py, which shows on the CPU that these inputs and bounds can see
the errors the GPU tests are for.  Seeds are this table's own (32000 ..), disjoint from every other table's.

Tolerance, by the rule of learn_cases.py: E32 = float32 against float64 evaluation of the reference (tests/learn_norm_ref.py) on the CPU, worst
case of the family, recorded with 25 % headroom; the GPU bound is FACTOR (8) x E32 relative to each output's max-abs.
    family        measured E32   recorded E32   bound (8 x)
    stats         6.3e-7         7.9e-7         6.3e-6
    clip_hl       7.9e-6         9.8e-6         7.8e-5
    clip_twohot   8.0e-4         1.0e-3         8.0e-3       (bin values up to 147 next to bins 0.03 apart: a float32 value resolves a weight to ~3e-4)
The quantiles lo and hi have a bound of their own, because they are order statistics and not sums: against the float64 torch.quantile of the
float32 data they may differ by the float32 rounding of ONE interpolation a + w (b - a) between the two neighbouring order statistics a, b:
w, b - a, the product and the sum round once each, |b - a| <= 2 M and |result| <= M with M = max(|a|, |b|), so the error is at most
(2 + 2 + 2 + 1) 2^-24 M < QUANTILE_ULPS x 2^-24 x M with QUANTILE_ULPS = 8."""
import torch

import learn_cases as LC
import learn_norm_ref as N

FACTOR = 8
E32 = {'stats': 7.9e-7, 'clip_hl': 9.8e-6, 'clip_twohot': 1.0e-3}
BOUND = {f: FACTOR * e for f, e in E32.items()}
QUANTILE_ULPS = 8
DECAY = 0.998


def _gen(c, k=0):
    return torch.Generator().manual_seed(c['seed'] * 16 + k)


# ------------------------------------------------------------------------------------------------------------------- return statistics
KEPT = (1, 2, 3, 20, 21, 64, 65, 257, 1025, 4097, 70001)
QS = ((0.05, 0.95), (0., 1.), (0.5, 0.5), (0.25, 0.75))
DATA = ('normal', 'equal', 'ties', 'signs', 'range', 'small')


def _s(kept, mask, data, q, ema):
    return dict(name=f'stats-N{kept}-mask_{mask}-{data}-q{q[0]:g}_{q[1]:g}-ema_{ema}', kept=kept, mask=mask, data=data, q=q, ema=ema, decay=DECAY)


def _stats_table():
    out = []
    for i, kept in enumerate(KEPT):             # every kept count with all ones and with a random mask; data, q pair and EMA state rotate
        for j, mask in enumerate(('ones', 'rand')):
            data = DATA[(2 * i + j) % 5]
            out.append(_s(kept, mask, data, QS[(i + j) % 4], 'fresh' if (i + j) % 3 else 'carried'))
    out += [_s(21, 'ones', 'normal', (0.05, 0.95), 'fresh'), _s(21, 'rand', 'range', (0.25, 0.75), 'fresh'),      # both positions on integer ranks
            _s(1, 'one', 'normal', (0.05, 0.95), 'fresh'), _s(1, 'one', 'range', (0.25, 0.75), 'carried'),
            _s(0, 'none', 'normal', (0.05, 0.95), 'carried'), _s(0, 'none', 'ties', (0., 1.), 'fresh'),
            _s(4097, 'rand', 'small', (0.05, 0.95), 'tiny'), _s(65, 'ones', 'equal', (0.25, 0.75), 'tiny'), _s(257, 'rand', 'small', (0.5, 0.5), 'tiny'),
            _s(70001, 'rand', 'ties', (0.05, 0.95), 'fresh'), _s(70001, 'ones', 'range', (0.25, 0.75), 'carried'), _s(1025, 'ones', 'signs', (0.05, 0.95), 'fresh'),
            _s(4097, 'ones', 'normal', (0.05, 0.95), 'fresh'), _s(257, 'ones', 'equal', (0., 1.), 'fresh')]
    for i, c in enumerate(out):
        c['seed'] = 32000 + i
        c['name'] += f'-{i}'
    return out


STATS = _stats_table()
EMA = {'fresh': (0., 1.), 'carried': (0.37, 2.6), 'tiny': (0.3, 1e-7)}         # 'tiny': the variance stays below 1e-5 after the update (small data)


def stats_inputs(c):
    """returns, old_values [n] float32; mask [n] (None: all ones) with exactly c['kept'] ones ('one': a single survivor among 65, 'none': no survivor
    among 65); ema, decay, q as the kernel is given them."""
    g = _gen(c)
    kept, kind = c['kept'], c['mask']
    n = {'ones': kept, 'rand': kept + kept // 2 + 3, 'one': 65, 'none': 65}[kind]
    x = torch.randn(n, generator=g)
    data = c['data']
    if data == 'normal':
        ret = 0.5 + 2. * x
    elif data == 'equal':
        ret = torch.full((n,), 1.25)
    elif data == 'ties':
        ret = torch.randint(-2, 3, (n,), generator=g).float()
        ret[::7] = -0.
    elif data == 'signs':
        ret = x.clone()
        ret[::5], ret[1::5] = 0., -0.
    elif data == 'range':
        ret = x.sign() * 10. ** (6. * torch.rand(n, generator=g))
    else:
        ret = 0.3 + 0.01 * x
    mask = None
    if kind != 'ones':
        mask = torch.zeros(n)
        mask[torch.randperm(n, generator=g)[:kept]] = 1.
        if data != 'equal':              # what is masked out differs from what is kept: an unmasked quantile would move
            ret = torch.where(mask > 0, ret, ret * 3. + 1.)
    old = ret - ret.abs().mean().clamp(min=0.01) * (0.2 + torch.randn(n, generator=g))
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).item()
    return dict(returns=ret, old_values=old, mask=mask, ema=tuple(f32(v) for v in EMA[c['ema']]), decay=c['decay'], q=tuple(f32(v) for v in c['q']))


def stats_expect(c, d, dtype=torch.float64, mut=()):
    return N.return_stats_ref(d, dtype, mut)


# ------------------------------------------------------------------------------------------------------------------- clipped value loss
CLIP_ALL = [dict(c, name=c['name'].replace('value-', 'clip-'), seed=32200 + i)
        for i, c in enumerate([c for c in LC.VALUE if c['eps'] <= 1] + [LC._v(0, 65, 130, 'p5'), LC._v(0, 255, 130, 'r4', 'null'), LC._v(1, 20, 130, 'p5')])]
CLIP_HL, CLIP_TWOHOT = [c for c in CLIP_ALL if not c['two_hot']], [c for c in CLIP_ALL if c['two_hot']]


def clip_range(c):
    sup = LC.value_support(c)
    return (sup[0].item(), sup[-1].item()) if c['two_hot'] else (c['vmin'], c['vmax'])


def clip_margin(c):
    """1e-3 of the encoder's value range: the least distance of every row from both branch points"""
    lo, hi = clip_range(c)
    return 1e-3 * (hi - lo)


def clip_value_clip(c):
    lo, hi = clip_range(c)
    return 0.05 * (hi - lo)


def _draw(c, g, R):
    """One draw of R candidate rows.  The logits carry a bump of random height around a random point, so that the prediction `values` and the plain
    cross entropy both spread; the situation fixes old_values relative to values; the returns lie near the clipped value (within 1.2 sigma /
    a bin and a half), where float32 still resolves the clipped encoding, and some beyond the range."""
    bins, two_hot = c['bins'], c['two_hot']
    sup = LC.value_support(c).double()
    lo, hi = clip_range(c)
    ctr = N.centres(LC.value_support(c), two_hot).double()
    m = lo + (hi - lo) * torch.rand(R, generator=g).double()
    h = torch.tensor([0., 6., 12.])[torch.randint(0, 3, (R,), generator=g)].double()
    width = (hi - lo) / bins * (1. + 3. * torch.rand(R, generator=g).double())
    logits = (2. * torch.randn(R, bins, generator=g).double() + h[:, None] * torch.exp(-0.5 * ((ctr[None] - m[:, None]) / width[:, None]) ** 2)).float()
    if not two_hot:        # 40 % of the HL-Gauss rows predict well: a near-Gaussian softmax a little wider than the target's, away from the ends of the range
        peaked = torch.rand(R, generator=g) < 0.4
        m = torch.where(peaked, lo + (hi - lo) * (0.15 + 0.7 * (m - lo) / (hi - lo)), m)
        w = float(c['sigma']) * (1.2 + 0.8 * torch.rand(R, generator=g).double())
        sharp_logits = (-0.5 * ((ctr[None] - m[:, None]) / w[:, None]) ** 2 + 0.3 * torch.randn(R, bins, generator=g).double()).float()
        logits = torch.where(peaked[:, None], sharp_logits, logits)
    values = (logits.double().softmax(-1) * ctr).sum(-1)
    cv, mg = clip_value_clip(c), clip_margin(c)
    sit = torch.randint(0, 20, (R,), generator=g)
    sit = torch.where(sit < 6, 0, torch.where(sit < 12, 1, torch.where(sit < 18, 2, sit - 15)))          # 30 / 30 / 30 / 5 / 5 %
    # the local scale around the prediction: sigma (HL-Gauss) or the bin spacing there (two-hot)
    idx = torch.searchsorted(sup[:bins], values).clamp(1, bins - 1)
    scale = (sup[idx] - sup[idx - 1]) if two_hot else torch.full((R,), float(c['sigma'])).double()
    # HL-Gauss rows whose softmax is peaked at m (the prediction within half a sigma of it): the return goes there, the clipped value within 1.5 sigma of it
    sharp = ((values - m).abs() < 0.5 * scale) & (not two_hot)
    gap = torch.maximum((0.3 + torch.where(sharp, 1.2, 2.2) * torch.rand(R, generator=g).double()) * scale, torch.tensor(2. * mg).double())
    u = 2. * torch.rand(R, generator=g).double() - 1.
    T = torch.where(sit == 0, values - gap, torch.where(sit == 1, values + gap, values))
    T = torch.where(sit == 3, torch.tensor(hi + 1.).double(), torch.where(sit == 4, torch.tensor(lo - 1.).double(), T))
    old = torch.where((sit == 0) | (sit == 4), T - cv, torch.where((sit == 1) | (sit == 3), T + cv, values + u * (cv - 2. * mg)))
    ret = T + scale * (1.2 if not two_hot else 1.5) * (2. * torch.rand(R, generator=g).double() - 1.)
    ret = torch.where(sharp & (sit < 3), m + 0.3 * scale * u, ret)
    return logits, ret.float(), old.float()


def clip_inputs(c):
    """value_inputs' arguments with old_values and value_clip.  Rows are drawn by rejection: a row is kept when, in float64, |loss1 - loss2| and
    ||values - old| - value_clip| are both at least clip_margin(c)."""
    g = _gen(c)
    R, bins = c['rows'], c['bins']
    sup = LC.value_support(c)
    base = dict(support=sup, vmin=c['vmin'], vmax=c['vmax'], sigma=c['sigma'], eps=c['eps'], two_hot=c['two_hot'], value_clip=clip_value_clip(c), mask=None)
    logits, ret, old = torch.empty(R, bins), torch.empty(R), torch.empty(R)
    need = torch.ones(R, dtype=torch.bool)
    for _ in range(40):
        l, r, o = _draw(c, g, R)
        ok = clip_margins(dict(base, logits=l, returns=r, old_values=o)).min(0).values >= clip_margin(c)
        take = need & ok
        logits[take], ret[take], old[take] = l[take], r[take], o[take]
        need &= ~take
        if not need.any():
            break
    assert not need.any(), c['name']
    mask = {'rand': (torch.rand(R, generator=g) < 0.7).float(), 'null': None, 'zero': torch.zeros(R)}[c['mask']]
    if c['mask'] == 'rand':
        mask[-1] = 1.
    return dict(base, logits=logits, returns=ret, old_values=old, mask=mask)


def clip_margins(d):
    """[2, R] in float64: |loss1 - loss2| and ||values - old| - value_clip|"""
    t = N.value_clip_terms(d, d['logits'].double())
    return torch.stack([(t['loss1'] - t['loss2']).abs(), (t['diff'].abs() - d['value_clip']).abs()])


def clip_situations(c, d):
    """Fractions of the rows: clipped above, clipped below, inside the band, clipped loss larger, plain loss larger (float64 reference)."""
    t = N.value_clip_terms(d, d['logits'].double())
    cv = d['value_clip']
    f = lambda b: b.double().mean().item()
    return dict(above=f(t['diff'] > cv), below=f(t['diff'] < -cv), inside=f(t['diff'].abs() < cv), clipped_larger=f(t['loss2'] > t['loss1']),
                plain_larger=f(t['loss1'] > t['loss2']))


def clip_expect(c, d, dtype=torch.float64, mut=()):
    return N.value_clip_ref(d, dtype, mut)


def clip_ld(c):
    return LC.value_ld(c)


FAMILIES = {'stats': (STATS, stats_inputs, stats_expect, N.STATS_MUTATIONS), 'clip_hl': (CLIP_HL, clip_inputs, clip_expect, N.CLIP_MUTATIONS),
            'clip_twohot': (CLIP_TWOHOT, clip_inputs, clip_expect, N.CLIP_MUTATIONS)}
ALL_TABLES = {f: t[0] for f, t in FAMILIES.items()}
