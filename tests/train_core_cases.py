"""Case tables, inputs and tolerances shared by tests/test_gpu_train_cores.py (the attention cores of the training path against float64,
through d4_train_attn_core / d4_train_xattn_core) and tests/test_train_cores_host.py (the same inputs on the CPU: can the bound see a wrong
mask row, a skipped belief projection, a geometry ignored, ...?).

A case is a dict.  `core` 0 is the whole-problem-in-LDS kernel, 1 the tiled core; `form` the name d4_debug_last_form must give; `key` names the
inputs, which the core-0 and the core-1 case of one shape share (and with them the float64 reference).  Inputs are seeded normals as flat
[rows][ld] buffers: q columns x 3, gamma x 0.3, logits of unit scale, leading dimensions above the minimum in a third of the cases.  A normal
row is never zero, so the gradient of the normalisations is defined everywhere.

The tolerance.  E32[family] is the largest error of the float32 evaluation of train_core_ref against its float64 evaluation over the family's
cases, measured on the CPU and recorded here with a quarter of headroom (test_train_cores_host.py asserts it still holds).  The kernels differ
from the float32 reference only in summation order and the device's tanhf / expf / sincosf, so the GPU bound is FACTOR x E32.  An error is the
max-abs difference of a (group, head) problem relative to that problem's reference max-abs, floored at 1e-3 of the tensor's max-abs
(train_core_ref.problem_err); the per-tensor error is never larger.  With one key the softmax is constant and dq, dk and dgamma_part are
identically zero in exact arithmetic, while a kernel that forms dS = P (dP - delta) from two differently ordered sums leaves rounding noise;
there the error is taken relative to max |dv|, the gradient of the same problem that does not vanish (dq and dk are sums of dS q / dS k with
|q|, |k| scaled > 1, so this is the stricter choice)."""
import functools

import torch

import train_core_ref as R

FACTOR = 8
# families: the self shapes the LDS kernels take (<= 64 items; both cores run them), the self shapes of the tiled core alone, cross (both cores).
# measured (test_train_cores_host.py prints them): self_lds 4.44e-6 (dk of the two-frame time case), self_long 5.25e-6 (dq at 256 frames, dh 16),
# cross 1.00e-5 (the gate logit's gradient of a one-query problem over 1024 keys: a single scalar d_o3 . o per problem)
E32 = {'self_lds': 5.6e-6, 'self_long': 6.6e-6, 'cross': 1.26e-5}
BOUND = {f: FACTOR * e for f, e in E32.items()}
GUARD = 16                      # floats after every buffer


def _n(g, n, scale=1.0):
    return torch.randn(n, generator=g, dtype=torch.float32) * scale


# ------------------------------------------------------------------------------------------------------------------- self attention
LDS_SHAPES = [(64, n) for n in (1, 2, 16, 17, 32, 33, 64)] + [(32, n) for n in (5, 16, 32, 33, 64)] + [(16, n) for n in (12, 32, 33, 64)]
LONG_ITEMS = (65, 100, 128, 130, 256)


def lds_form(dh, items):
    cap = 16 if items <= 16 else 32 if items <= 32 else 64
    if dh != 64:
        cap = max(cap, 32)
    return f'attn_bwd_kernel<{dh},{cap}>'


def _self_shape(i, geo, dh, items, heads=None, groups=None, cols=None, batch=2, ns=None):
    """the i-th shape of its table: heads, groups, residual, belief, clamp, specials and the leading dimension rotate with i"""
    if items == 2:
        # one (group, head) problem: a two-key softmax of queries x 3 is often saturated, the gradients through it then sink toward the floor of
        # the per-problem measure, and there float32 (the reference's as much as a kernel's) has no relative accuracy left to measure against
        heads, groups, cols, batch = 1, 1, 1, 1
    heads = (1, 2, 3, 5)[i % 4] if heads is None else heads
    c = dict(geo=geo, dh=dh, items=items, heads=heads, vres=i % 2, belief=int(items > 1 and (i // 2) % 2 == 0), clamp=(50., 3., 0.)[i % 3],
             pad=5 if (i % 3 == 0 or items == 1) else 0, ns=0)
    if geo == 'frame':
        c['groups'] = (1 + i % 5 if items > 1 else 2 + i % 4) if groups is None else groups
        c['ns'] = (0, 1, items // 2, items - 1, items)[i % 5] if ns is None else ns
        c.update(g_inner=1, outer=items, item=1)
    else:
        cols = (1, 3)[(i // 2) % 2] if cols is None else cols
        c.update(groups=batch * cols, g_inner=cols, outer=items * cols, item=cols, cols=cols)
    c['key'] = f"{geo}-dh{dh}-n{items}"
    return c


def _self_cases():
    shapes, long = [], []
    for gi, geo in enumerate(('frame', 'time')):
        for i, (dh, items) in enumerate(LDS_SHAPES):
            shapes.append(_self_shape(i + gi, geo, dh, items))
        for i, (items, dh) in enumerate((n, dh) for n in LONG_ITEMS for dh in (64, 32, 16)):
            ns = (0, 1, 4, items // 2, items - 1, items)[i % 6]
            long.append(_self_shape(i + gi, geo, dh, items, heads=(1, 2, 3)[i % 3], groups=1 + i % 3, ns=ns))
        long.append(_self_shape(gi, geo, 16, 1024, heads=1, groups=1, cols=1, batch=1, ns=512))
    cs = [dict(c, core=0, family='self_lds', form=lds_form(c['dh'], c['items'])) for c in shapes]
    cs += [dict(c, core=1, family='self_lds', form=f"tiled<{c['geo']},{c['dh']}>") for c in shapes]
    cs += [dict(c, core=1, family='self_long', form=f"tiled<{c['geo']},{c['dh']}>") for c in long]
    for k, c in enumerate(shapes + long):
        c['seed'] = 5000 + k
    out = []
    for c in cs:
        seed = next(s['seed'] for s in shapes + long if s['key'] == c['key'])
        out.append(dict(c, seed=seed, name=f"{c['key']}-core{c['core']}"))
    return out


SELF = _self_cases()


def self_rows_total(c):
    return c['groups'] * c['items']


def self_ldp(c):
    hd = c['heads'] * c['dh']
    return 3 * hd + R.hp4_of(c['heads']) + c['heads'] + c['pad']


def self_inputs(c):
    g = torch.Generator().manual_seed(c['seed'])
    rows, hd, dh, ldp = self_rows_total(c), c['heads'] * c['dh'], c['dh'], self_ldp(c)
    proj = _n(g, rows * ldp).view(rows, ldp)
    proj[:, :hd] *= 3
    inv = 1.0 / (10000. ** (torch.arange(0, dh, 2).float() / dh)) if c['geo'] == 'time' else None
    return dict(proj=proj.reshape(-1), rv=_n(g, rows * hd) if c['vres'] else None, gamma=_n(g, hd, 0.3), d_o3=_n(g, rows * hd), inv_freq=inv)


def self_expect(c, d, dtype=torch.float64, mut=(), backward=True):
    return R.self_core(d['proj'], self_ldp(c), d['rv'], d['gamma'], d['d_o3'] if backward else None, groups=c['groups'], items=c['items'],
                       heads=c['heads'], dh=c['dh'], softclamp=c['clamp'], num_special=c['ns'], belief=c['belief'], g_inner=c['g_inner'],
                       g_outer_stride=c['outer'], item_stride=c['item'], causal=int(c['geo'] == 'time'), inv_freq=d['inv_freq'], dtype=dtype, mut=mut)


def self_mutations(c):
    m = ['no_gate', 'v_from_k']
    n = c['items']
    if c['pad'] and self_rows_total(c) > 1:
        m.append('ld_min')
    if c['vres']:
        m.append('no_vres')
    if c['belief']:
        m.append('no_belief')
    if n >= 2:
        m.append('gamma_only')
        if c['clamp'] > 0:
            m.append('no_clamp')
        if c['dh'] != 64:
            m.append('scale64')
        if c['geo'] == 'time':
            m += ['causal_strict', 'k_unrotated']
    if c['geo'] == 'frame' and 0 < c['ns'] < n:
        m.append('mask_row')
    if c['geo'] == 'time' and c['g_inner'] > 1:
        m.append('g_inner_ignored')
    return m


# ------------------------------------------------------------------------------------------------------------------- cross attention
CROSS_LDS_PAIRS = [(1, 1), (1, 7), (3, 20), (4, 64), (17, 33), (64, 5), (64, 64)]
CROSS_LONG_PAIRS = [(1, 74), (4, 256), (130, 5), (65, 65), (1, 1024)]


def _cross_shape(i, nq, nk, dh):
    one = nk == 1 or i % 3 == 0                  # (a one-key problem is only seen through the gate, the value columns and the leading dimensions)
    c = dict(nq=nq, nk=nk, dh=dh, heads=1 if nk >= 1024 else (2, 1, 3)[i % 3], groups=2 if nk >= 1024 else 2 + i % 3, item_major=(i // 2) % 2,
             clamp=(5., 0.)[i % 2], padq=3 if one else 0, padk=5 if one else 0)
    c['key'] = f'cross-{nq}x{nk}-dh{dh}'
    return c


def _cross_cases():
    shapes = [_cross_shape(i, nq, nk, dh) for i, (nq, nk, dh) in enumerate((q, k, dh) for q, k in CROSS_LDS_PAIRS for dh in (64, 32, 16))]
    long = [_cross_shape(i + 1, nq, nk, dh) for i, (nq, nk, dh) in enumerate((q, k, dh) for q, k in CROSS_LONG_PAIRS for dh in (64, 32, 16))]
    for k, c in enumerate(shapes + long):
        c['seed'] = 7000 + k
    cs = [dict(c, core=0, form=f"xattn_bwd_kernel<{c['dh']}>") for c in shapes]
    cs += [dict(c, core=1, form=f"tiled<cross,{c['dh']}>") for c in shapes + long]
    return [dict(c, family='cross', name=f"{c['key']}-core{c['core']}") for c in cs]


CROSS = _cross_cases()


def cross_lds(c):
    hd = c['heads'] * c['dh']
    return hd + c['heads'] + c['padq'], 2 * hd + c['padk']


def cross_inputs(c):
    g = torch.Generator().manual_seed(c['seed'])
    G, nq, nk, hd = c['groups'], c['nq'], c['nk'], c['heads'] * c['dh']
    ldq, ldk = cross_lds(c)
    projq = _n(g, G * nq * ldq).view(G * nq, ldq)
    projq[:, :hd] *= 3
    return dict(projq=projq.reshape(-1), projk=_n(g, G * nk * ldk), gamma=_n(g, hd, 0.3), d_o3=_n(g, G * nq * hd))


def cross_expect(c, d, dtype=torch.float64, mut=(), backward=True):
    ldq, ldk = cross_lds(c)
    return R.cross_core(d['projq'], ldq, d['projk'], ldk, d['gamma'], d['d_o3'] if backward else None, groups=c['groups'], nq=c['nq'], nk=c['nk'],
                        heads=c['heads'], dh=c['dh'], item_major=c['item_major'], softclamp=c['clamp'], dtype=dtype, mut=mut)


def cross_mutations(c):
    m = ['no_gate', 'v_from_k']
    if c['padq']:
        m.append('ld_min')
    if c['nk'] >= 2:
        m += ['gamma_only', 'item_major_swapped']
        if c['clamp'] > 0:
            m.append('no_clamp')
        if c['dh'] != 64:
            m.append('scale64')
    return m


# ------------------------------------------------------------------------------------------------------------------- shared evaluation
def inputs(c):
    return _inputs(c['key'])


def expect(c):
    """the float64 reference of the case's inputs (computed once per shape: the core-0 and the core-1 case share it)"""
    return _expect(c['key'])


def _first(key):
    return next(c for c in SELF + CROSS if c['key'] == key)


@functools.lru_cache(maxsize=None)
def _inputs(key):
    c = _first(key)
    return cross_inputs(c) if c['family'] == 'cross' else self_inputs(c)


@functools.lru_cache(maxsize=None)
def _expect(key):
    c = _first(key)
    return evaluate(c)


def evaluate(c, dtype=torch.float64, mut=(), backward=True):
    d = inputs(c)
    return (cross_expect if c['family'] == 'cross' else self_expect)(c, d, dtype, mut, backward)


def mutations(c):
    return cross_mutations(c) if c['family'] == 'cross' else self_mutations(c)


def worst(errs):
    """the largest per-problem error over the tensors of train_core_ref.errors"""
    return max(e for e, _ in errs.values())
