"""GPU: the kernels of the learner's two actor-critic options (csrc/learn.hip: return_stats_kernel of keep_reward_ema_stats, value_loss_clip_kernel of
clip_values), one operator call per case through d4_return_stats / d4_value_loss, each against the plain float64 reference of
tests/learn_norm_ref.py on the inputs of tests/learn_norm_cases.py (whose host test shows what these inputs and bounds can see).

A case asserts
  * the values: max |out - float64| <= BOUND[family] x max |float64| for the advantage, the updated EMA pair, mean / var, the loss, the row losses
    and dlogits (an output whose reference is zero everywhere must be zero exactly);
  * the quantiles lo, hi against the float64 torch.quantile of the float32 data to the float32 rounding of one interpolation
    (learn_norm_cases.QUANTILE_ULPS x 2^-24 x the larger neighbouring order statistic): they are order statistics, not sums;
  * untouched memory: every operand and output lies between NaN guards; nothing outside [rows][ld] is written and the pad columns are exactly 0;
  * no kept return: the EMA pair keeps its bits.
d4_value_loss with clip_values = 0 gives d4_hl_gauss_ce's bits.  Bounds: learn_norm_cases.py (E32 measured on the CPU, x 8)."""
import ctypes as C

import pytest
import torch

import learn_cases as LC
import learn_norm_cases as NC
import learn_norm_ref as N
from dreamer4_amd import _lib
from test_gpu_attn_cores import DEV, GUARD, bits, stream
from test_gpu_glue import flat_in, out_buf, rows_in

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def ptr(x):
    return None if x is None else x.ptr


def inner(buf, n):
    """the n elements of a flat buffer, after the guards were seen intact"""
    g = buf.dev.cpu()
    assert g[:GUARD + buf.off].isnan().all() and g[GUARD + buf.off + n:].isnan().all(), 'written outside the buffer'
    out = g[GUARD + buf.off:GUARD + buf.off + n]
    assert not out.isnan().any(), 'NaN in the output (a gap was read or an element was not written)'
    return out


def close(family, name, what, got, ref):
    err = N.err(got, ref)
    print(f'{family} {name} {what}: err {err:.3e} (bound {NC.BOUND[family]:.3e})')
    assert err <= NC.BOUND[family], f'{name} {what}: error {err:.3e} above the bound {NC.BOUND[family]:.3e}'


# ------------------------------------------------------------------------------------------------------------------- return statistics
@pytest.mark.parametrize('c', NC.STATS, ids=[c['name'] for c in NC.STATS])
def test_return_stats(lib, c):
    d = NC.stats_inputs(c)
    n = d['returns'].numel()
    a = dict(returns=flat_in(d['returns']), old=flat_in(d['old_values']), mask=None if d['mask'] is None else flat_in(d['mask']),
             ema=flat_in(torch.tensor(d['ema'], dtype=torch.float32)), adv=out_buf(n), stats=out_buf(4))
    before = bits(inner(a['ema'], 2))
    _lib.check(lib.d4_return_stats(ptr(a['returns']), ptr(a['old']), ptr(a['mask']), n, ptr(a['ema']), d['decay'], d['q'][0], d['q'][1], ptr(a['adv']), ptr(a['stats']), stream()))
    torch.cuda.synchronize()
    ref = NC.stats_expect(c, d)
    ema, stats, adv = inner(a['ema'], 2), inner(a['stats'], 4), inner(a['adv'], n)
    for k in ('returns', 'old', 'mask'):
        assert a[k] is None or torch.equal(bits(a[k].dev.cpu()), bits(a[k].host)), f'{k} was written'
    if c['kept'] == 0:
        assert torch.equal(bits(ema), before), 'the EMA pair changed although no return was kept'
        assert (stats == 0).all()
    else:
        for got, want, (x0, x1) in zip(stats[:2].double().tolist(), ref['stats'][:2].tolist(), N.order_statistics(d)):
            bound = NC.QUANTILE_ULPS * 2. ** -24 * max(abs(x0), abs(x1))
            print(f"stats {c['name']} quantile: err {abs(got - want):.3e} (bound {bound:.3e})")
            assert abs(got - want) <= bound, f"{c['name']}: quantile {got!r} against {want!r}, bound {bound:.3e}"
        close('stats', c['name'], 'mean / var', stats[2:], ref['stats'][2:])
    close('stats', c['name'], 'ema', ema, ref['ema'])
    close('stats', c['name'], 'adv', adv, ref['adv'])


def test_return_stats_refusals(lib):
    d = NC.stats_inputs(NC.STATS[6])
    n = d['returns'].numel()
    base = dict(returns=flat_in(d['returns']), old=flat_in(d['old_values']), ema=flat_in(torch.tensor(d['ema'])), n=n, decay=d['decay'], q_lo=d['q'][0], q_hi=d['q'][1])
    for over in (dict(returns=None), dict(old=None), dict(ema=None), dict(n=0), dict(q_lo=0.9, q_hi=0.1), dict(q_hi=1.5), dict(decay=0.3), dict(adv=None), dict(stats=None)):
        a = dict(base, adv=out_buf(n), stats=out_buf(4))
        a.update(over)
        rc = lib.d4_return_stats(ptr(a['returns']), ptr(a['old']), None, a['n'], ptr(a['ema']), a['decay'], a['q_lo'], a['q_hi'], ptr(a['adv']), ptr(a['stats']), stream())
        torch.cuda.synchronize()
        assert rc != 0 and 'd4_return_stats' in lib.d4_last_error().decode(), over
        assert all(a[k] is None or a[k].dev.isnan().all() for k in ('adv', 'stats')), 'a refused call wrote to an output'


# ------------------------------------------------------------------------------------------------------------------- clipped value loss
def value_call(lib, c, d, clip, **over):
    R, bins, ld = c['rows'], c['bins'], NC.clip_ld(c)
    a = dict(logits=rows_in(d['logits'], ld), ld=ld, returns=flat_in(d['returns']), old_values=flat_in(d['old_values']) if d.get('old_values') is not None else None,
             mask=flat_in(d['mask']) if d['mask'] is not None else None, support=flat_in(d['support']), rows=R, bins=bins, loss=out_buf(1), row_loss=out_buf(R),
             dlogits=out_buf(R * ld), scratch=out_buf(R + 64), value_clip=d.get('value_clip', 0.))
    a.update(over)
    desc = _lib.ValueLossDesc()
    for k in ('logits', 'returns', 'old_values', 'mask', 'support', 'loss', 'row_loss', 'dlogits', 'scratch'):
        setattr(desc, k, ptr(a[k]))
    desc.ld, desc.rows, desc.bins, desc.vmin, desc.vmax, desc.sigma, desc.eps = a['ld'], a['rows'], a['bins'], c['vmin'], c['vmax'], c['sigma'], c['eps']
    desc.two_hot, desc.clip_values, desc.value_clip = c['two_hot'], clip, a['value_clip']
    rc = lib.d4_value_loss(C.byref(desc), stream())
    torch.cuda.synchronize()
    return rc, a


def rows_of(buf, rows, cols, ld):
    got = buf.dev.cpu()
    inside = torch.zeros(got.numel(), dtype=torch.bool)
    inside.as_strided((rows, ld), (ld, 1), GUARD + buf.off).fill_(True)
    assert got[~inside].isnan().all(), 'written outside [rows][ld]'
    g = got.as_strided((rows, ld), (ld, 1), GUARD + buf.off)
    assert not g.isnan().any(), 'NaN in the output (a gap was read or an element was not written)'
    assert (g[:, cols:] == 0).all(), 'the pad columns are not zero'
    return g[:, :cols]


@pytest.mark.parametrize('c', NC.CLIP_ALL, ids=[c['name'] for c in NC.CLIP_ALL])
def test_value_loss_clipped(lib, c):
    d = NC.clip_inputs(c)
    rc, a = value_call(lib, c, d, 1)
    _lib.check(rc)
    ref = NC.clip_expect(c, d)
    fam = 'clip_twohot' if c['two_hot'] else 'clip_hl'
    close(fam, c['name'], 'loss', inner(a['loss'], 1), ref['loss'])
    close(fam, c['name'], 'row_loss', inner(a['row_loss'], c['rows']), ref['row_loss'])
    close(fam, c['name'], 'dlogits', rows_of(a['dlogits'], c['rows'], c['bins'], a['ld']), ref['dv'])
    g = a['scratch'].dev.cpu()
    assert g[:GUARD].isnan().all() and g[-GUARD:].isnan().all(), 'written outside the scratch'


@pytest.mark.parametrize('c', LC.VALUE, ids=[c['name'] for c in LC.VALUE])
def test_value_loss_unclipped_gives_hl_gauss_ce_bits(lib, c):
    d = LC.value_inputs(c)
    rc, a = value_call(lib, c, d, 0)
    _lib.check(rc)
    R, bins, ld = c['rows'], c['bins'], a['ld']
    loss, dv, scratch = out_buf(1), out_buf(R * ld), out_buf(2 * R + 64)
    _lib.check(lib.d4_hl_gauss_ce(ptr(a['logits']), ld, ptr(a['returns']), ptr(a['mask']), ptr(a['support']), R, bins, c['vmin'], c['vmax'], c['sigma'], c['eps'], c['two_hot'],
                                  ptr(loss), ptr(dv), ptr(scratch), stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(a['loss'].dev.cpu()), bits(loss.dev.cpu())) and torch.equal(bits(a['dlogits'].dev.cpu()), bits(dv.dev.cpu()))
    ref = LC.value_expect(c, d)                 # and the row losses, which d4_hl_gauss_ce keeps to itself, sum to the loss
    count = max(1., float(c['rows'] if d['mask'] is None else d['mask'].sum()))
    assert N.err(inner(a['row_loss'], R).double().sum().reshape(1) / count, ref['loss']) <= LC.BOUND['value']


def test_value_loss_refusals(lib):
    c = NC.CLIP_ALL[1]
    d = NC.clip_inputs(c)
    for over in (dict(ld=c['bins'] - 1), dict(rows=0), dict(bins=0), dict(logits=None), dict(returns=None), dict(old_values=None), dict(support=None), dict(loss=None),
                 dict(row_loss=None), dict(dlogits=None), dict(scratch=None), dict(value_clip=-0.1)):
        rc, a = value_call(lib, c, d, 1, **over)
        assert rc != 0 and 'd4_value_loss' in lib.d4_last_error().decode(), over
        assert all(a[k] is None or a[k].dev.isnan().all() for k in ('loss', 'row_loss', 'dlogits', 'scratch')), 'a refused call wrote to an output'
