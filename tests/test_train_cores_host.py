"""Host: the inputs and the bound of tests/test_gpu_train_cores.py can see the errors those tests are for.

For every case of the shared tables (tests/train_core_cases.py) the float64 reference (tests/train_core_ref.py) is evaluated once as it is
and once per applicable mutation of train_core_ref.MUTATIONS: every mutation must move some output by at least 10 x the GPU bound of the
case's family, on the very inputs the GPU test uses, measured as the GPU test measures (per (group, head) problem).  And the float32
evaluation of the reference stays within the recorded E32 of its float64 evaluation: the measurement the bound is derived from.  The
core-0 and the core-1 case of one shape share their inputs, so they are evaluated once and counted twice."""
import collections
import functools

import torch

import train_core_cases as K
import train_core_ref as R

ROOM = 10
CASES = K.SELF + K.CROSS


@functools.lru_cache(maxsize=None)
def _measure(key, family):
    c = next(c for c in CASES if c['key'] == key and c['family'] == family)
    ref = K.expect(c)
    e32 = R.errors(K.evaluate(c, torch.float32), ref)
    moved = {m: K.worst(R.errors(K.evaluate(c, mut=(m,)), ref)) for m in K.mutations(c)}
    return e32, moved


def test_tables_are_what_the_issue_lists():
    names = [c['name'] for c in CASES]
    assert len(set(names)) == len(names)
    assert K.BOUND == {f: 8 * e for f, e in K.E32.items()}
    lds = {(c['geo'], c['dh'], c['items']) for c in K.SELF if c['core'] == 0}
    assert lds == {(g, dh, n) for g in ('frame', 'time') for dh, n in K.LDS_SHAPES} and all(n <= 64 for _, _, n in lds)
    tiled = {(c['geo'], c['dh'], c['items']) for c in K.SELF if c['core'] == 1}
    assert lds <= tiled                                                     # every LDS case again on the tiled core: the same inputs
    assert {(g, dh, n) for g in ('frame', 'time') for dh in (64, 32, 16) for n in K.LONG_ITEMS} | {('frame', 16, 1024), ('time', 16, 1024)} == tiled - lds
    assert {c['form'] for c in K.SELF if c['core'] == 0} == {f'attn_bwd_kernel<{a}>' for a in ('64,16', '64,32', '64,64', '32,32', '32,64', '16,32', '16,64')}
    for c in K.SELF:
        assert c['belief'] == 0 or c['items'] > 1                          # (one item with belief: the output is identically zero)
        assert 0 <= c['ns'] <= c['items'] and (c['geo'] == 'frame' or c['ns'] == 0)
    frame = [c for c in K.SELF if c['geo'] == 'frame' and c['core'] == 0]
    assert {('0' if c['ns'] == 0 else '1' if c['ns'] == 1 else 'all' if c['ns'] == c['items'] else 'all-1' if c['ns'] == c['items'] - 1 else 'half')
            for c in frame} >= {'0', '1', 'half', 'all-1', 'all'}
    time = [c for c in K.SELF if c['geo'] == 'time' and c['core'] == 0]
    assert {c['cols'] for c in time} == {1, 3} and {c['heads'] for c in frame + time} == {1, 2, 3, 5} and {c['groups'] for c in frame} >= {1, 2, 3, 4, 5}
    assert {c['clamp'] for c in K.SELF} == {50., 3., 0.} and {c['vres'] for c in K.SELF} == {0, 1}
    x0 = {(c['nq'], c['nk'], c['dh']) for c in K.CROSS if c['core'] == 0}
    x1 = {(c['nq'], c['nk'], c['dh']) for c in K.CROSS if c['core'] == 1}
    assert x0 == {(q, k, dh) for q, k in K.CROSS_LDS_PAIRS for dh in (64, 32, 16)}
    assert x1 - x0 == {(q, k, dh) for q, k in K.CROSS_LONG_PAIRS for dh in (64, 32, 16)} and x0 <= x1
    assert {(c['item_major'], c['clamp']) for c in K.CROSS if c['core'] == 0} == {(0, 0.), (0, 5.), (1, 0.), (1, 5.)}
    padded = sum(1 for c in CASES if c.get('pad') or c.get('padq'))
    assert 3 * padded >= len(CASES)                                         # leading dimensions above the minimum in a third of the cases


def test_no_input_row_is_zero():
    for key in sorted({c['key'] for c in CASES}):
        d = K.inputs(next(c for c in CASES if c['key'] == key))
        for n in ('proj', 'projk'):
            if n in d:
                assert (d[n] != 0).all(), key


def test_float32_evaluation_stays_within_e32():
    worst = collections.defaultdict(lambda: (0., ''))
    bad = []
    for c in CASES:
        e32, _ = _measure(c['key'], c['family'])
        for n, (e, _t) in e32.items():
            if e > worst[c['family']][0]:
                worst[c['family']] = (e, f"{n} of {c['key']}")
            if not e <= K.E32[c['family']]:
                bad.append(f"{c['name']}: float32 evaluation of {n} {e:.3e} above the recorded E32 {K.E32[c['family']]:.3e}")
    for f in K.E32:
        print(f'{f}: E32 measured {worst[f][0]:.3e} ({worst[f][1]}), recorded {K.E32[f]:.3e}, GPU bound {K.BOUND[f]:.3e}')
    assert set(worst) == set(K.E32) and not bad, '\n'.join(bad)


def test_every_mutation_moves_every_case_it_applies_to():
    applied = collections.Counter()
    weakest = (float('inf'), '')
    bad = []
    for c in CASES:
        _, moved = _measure(c['key'], c['family'])
        assert set(moved) == set(K.mutations(c)) and set(moved) <= set(R.MUTATIONS)
        if len(moved) < 3:
            bad.append(f"{c['name']}: only {sorted(moved)} apply")
        for m, v in moved.items():
            applied[m] += 1
            margin = v / K.BOUND[c['family']]
            if margin < weakest[0]:
                weakest = (margin, f"{m} at {c['name']} moves {v:.3e}")
            if not v >= ROOM * K.BOUND[c['family']]:
                bad.append(f"{c['name']}: {m} moves the outputs by {v:.3e} only (< {ROOM} x bound {K.BOUND[c['family']]:.3e})")
    print(f'weakest mutation: {weakest[1]} = {weakest[0]:.1f} x the bound; applications: {dict(applied)}')
    bad += [f'{m} applies to {applied[m]} cases only' for m in R.MUTATIONS if applied[m] < 5]
    assert not bad, '\n'.join(bad)
