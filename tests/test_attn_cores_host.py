"""Host: the inputs and the bound of tests/test_gpu_attn_cores.py can see the errors those tests are for.

For every case of the shared tables (tests/attn_core_cases.py) the float64 reference is evaluated once as it is and once per applicable
mutation of attn_core_ref.MUTATIONS (a key dropped or admitted, the mask a row off, belief / value residual / the hiddens' rms skipped, the
rotary position off by one, a wrong key scale or gamma, the gate of another row): every mutation must move a checked output by at least
10 x the GPU bound, on the very inputs the GPU test uses.  And the float32 evaluation of each reference stays within the recorded E32 of
its float64 evaluation — the measurement the bound is derived from."""
import torch

import attn_core_cases as K
import attn_core_ref as R

ROOM = 10


def _check(family, rows):
    """rows: (case name, float32-vs-float64 error, {mutation: movement}) per case"""
    bad = [f'{n}: float32 evaluation {e:.3e} above the recorded E32 {K.E32[family]:.3e}' for n, e, _ in rows if not e <= K.E32[family]]
    bad += [f'{n}: {m} moves the output by {v:.3e} only (< {ROOM} x bound {K.BOUND[family]:.3e})' for n, _, mv in rows for m, v in mv.items()
            if not v >= ROOM * K.BOUND[family]]
    seen = {m for _, _, mv in rows for m in mv}
    print(f'{family}: E32 measured {max(e for _, e, _ in rows):.3e} (recorded {K.E32[family]:.3e}); smallest movement per mutation: '
          + ', '.join(f'{m} {min(mv[m] for _, _, mv in rows if m in mv):.2e}' for m in sorted(seen)))
    assert not bad, '\n'.join(bad)
    return seen


def test_case_names_are_unique_and_bounds_follow_e32():
    for table in (K.SMALL_ATTN, K.POOL_MIX, K.TIME):
        names = [c['name'] for c in table]
        assert len(set(names)) == len(names)
    assert K.BOUND == {f: 8 * e for f, e in K.E32.items()}


def test_small_attn_inputs_see_every_mutation():
    rows = []
    for c in K.SMALL_ATTN:
        d = K.small_attn_inputs(c)
        ref = K.small_attn_expect(c, d)
        mv = {m: R.rel_err(K.small_attn_expect(c, d, mut=(m,)), ref) for m in K.small_attn_mutations(c)}
        rows.append((c['name'], R.rel_err(K.small_attn_expect(c, d, torch.float32), ref), mv))
    assert _check('small_attn', rows) == {'drop_newest', 'drop_oldest', 'extra_key', 'mask_row', 'no_belief', 'no_vres', 'scale64', 'gamma_only'}


def test_pool_mix_inputs_see_every_mutation():
    rows = []
    for c in K.POOL_MIX:
        d = K.pool_inputs(c)
        ref = K.pool_expect(c, d)
        mv = {m: R.rel_err(K.pool_expect(c, d, mut=(m,)), ref) for m in K.pool_mutations(c)}
        rows.append((c['name'], R.rel_err(K.pool_expect(c, d, torch.float32), ref), mv))
    assert _check('pool_mix', rows) == {'drop_newest', 'drop_oldest', 'gamma_only', 'no_rms', 'gate_row'}


def test_time_decode_inputs_see_every_mutation():
    rows = []
    for c in K.TIME:
        d = K.time_inputs(c)
        cache, out = K.time_expect(c, d)
        written = ~cache.isnan()
        scale = K.time_scale(c, cache, out)
        append = c['kind'] == 'append'

        def moved(cache_m, out_m):
            e = R.rel_err(cache_m[written], cache[written])
            return e if append else max(e, ((out_m.double() - out).abs().max() / scale).item())

        fill = torch.randn(cache.shape, generator=torch.Generator().manual_seed(c['seed']), dtype=torch.float64)     # ('extra_key' reads a never-written row)
        mv = {m: moved(*K.time_expect(c, d, mut=(m,), fill=fill)) for m in K.time_mutations(c)}
        rows.append((c['name'], moved(*K.time_expect(c, d, torch.float32)), mv))
    assert _check('time', rows) == {'drop_newest', 'drop_oldest', 'extra_key', 'no_belief', 'no_vres', 'rot_off', 'rot_off_k', 'scale64', 'gamma_only'}
