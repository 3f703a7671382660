"""Host: the inputs and the bounds of tests/test_gpu_deep_pool.py can see the errors those tests are for.

For every case of tests/deep_pool_cases.py the float32 evaluation of attn_core_ref.pool_mix_ref stays within the table's recorded E32 of its
float64 evaluation (the family's own value: a softmax over up to 1024 hiddens sums more terms than the pool_mix family's 64), and every
applicable mutation moves the output by at least 10 x the GPU bound, on the very inputs the GPU test uses.  The oracle the engine tests
compare against (restate.generate), evaluated in float32, stays within a tenth of those tests' tolerance of its float64 evaluation at every
engine configuration.  And the wide_frames option builds a depth-40 model's mirror and engine configuration on the CPU."""
import pytest
import torch

import attn_core_cases as K
import attn_core_ref as R
import deep_pool_cases as P
from oracle import restate
from util import make_noise, oracle_config, oracle_weights, small_model

ROOM = 10


def test_case_table_covers_what_it_names():
    names = [c['name'] for c in P.DEEP]
    assert len(set(names)) == len(names)
    assert P.BOUND == 8 * P.E32 and P.E32 != K.E32['pool_mix']
    assert {c['form'] for c in P.DEEP} == P.FORMS and len(P.FORMS) == 10
    assert all(1 <= c['L'] <= 1024 and c['D'] % 4 == 0 and c['D'] <= 1024 for c in P.DEEP)
    assert {c['L'] for c in P.DEEP} == {3, 65, 66, 127, 128, 129, 191, 193, 257, 1023, 1024}
    assert {c['D'] for c in P.DEEP} == {64, 96, 256, 260, 320, 512, 768, 1024}
    rows = [c for c in P.DEEP if 'rows' in c['form']]
    assert {c['L'] % 4 for c in rows if c['L'] > 64} == {0, 1, 2, 3} and any(c['L'] < 4 for c in rows)      # (L = 3: a wave without a hidden)
    assert {c['M'] for c in P.DEEP} == {1, 2, 5, 2048, 2049} and {(c['D'], c['M']) for c in P.DEEP if c['L'] >= 1023} == {(64, 1), (512, 2), (1024, 1)}
    assert {(c['M'], 'rows' in c['form']) for c in P.DEEP if c['M'] >= 2048} == {(2048, True), (2049, False)}
    assert all(c['L'] == 65 for c in P.DEEP if c['M'] >= 2048)
    for key in ('kb', 'qb', 'hb', 'ub', 'x_last'):
        assert {c[key] for c in P.DEEP} == {0, 1}, key
    assert any(c['hb'] and 'rows' not in c['form'] for c in P.DEEP)                  # the hiddens' bf16 image is read by the wave-per-row form
    assert all(c['kb'] or not (c['qb'] or c['hb']) for c in P.DEEP)
    assert len({c['seed'] for c in P.DEEP}) == len(P.DEEP) and min(c['seed'] for c in P.DEEP) >= 12000
    assert {c['seed'] for c in P.DEEP}.isdisjoint({c['seed'] for c in K.POOL_MIX})


def test_deep_pool_inputs_see_every_mutation():
    rows = []
    for c in P.DEEP:
        d = K.pool_inputs(c)
        ref = P.deep_expect(c, d)
        mv = {m: R.rel_err(P.deep_expect(c, d, mut=(m,)), ref) for m in K.pool_mutations(c)}
        rows.append((c['name'], R.rel_err(P.deep_expect(c, d, dtype=torch.float32), ref), mv))
    for n, e, mv in rows:
        print(f'{n}: E32 {e:.3e}; ' + ', '.join(f'{m} {v:.2e}' for m, v in mv.items()))
    worst = max(rows, key=lambda r: r[1])
    least = min(((v, m, n) for n, _, mv in rows for m, v in mv.items()))
    print(f'worst E32 {worst[1]:.3e} ({worst[0]}); recorded {P.E32:.3e}; smallest movement {least[0]:.3e} ({least[1]} at {least[2]}) = {least[0] / P.BOUND:.0f} x bound')
    bad = [f'{n}: float32 evaluation {e:.3e} above the recorded E32 {P.E32:.3e}' for n, e, _ in rows if not e <= P.E32]
    bad += [f'{n}: {m} moves the output by {v:.3e} only (< {ROOM} x bound {P.BOUND:.3e})' for n, _, mv in rows for m, v in mv.items() if not v >= ROOM * P.BOUND]
    assert not bad, '\n'.join(bad)
    assert worst[1] >= P.E32 / 2, 'the recorded E32 is more than twice what this table measures'
    assert {m for _, _, mv in rows for m in mv} == {'drop_newest', 'drop_oldest', 'gamma_only', 'no_rms', 'gate_row'}


def _generate(cfg, W, nz, dtype, T, B):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)                           # (the oracle creates its empty histories in the default dtype)
    try:
        return restate.generate(cfg, {k: v.to(dtype) if v.is_floating_point() else v for k, v in W.items()}, T, batch_size=B,
                                noise={k: v.to(dtype) for k, v in nz.items()})
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize('name', sorted(P.ENGINE))
def test_fp32_oracle_is_within_a_tenth_of_the_engine_tolerance(name):
    """tolerance of the engine tests: |a - b| <= 2e-4 + 1e-4 |b|"""
    m = small_model(**P.ENGINE[name], wide_frames=True)
    cfg, W = oracle_config(m), oracle_weights(m)
    B, T = 3, 3
    nz = make_noise(cfg, T, B, 77)
    f32, f64 = _generate(cfg, W, nz, torch.float32, T, B), _generate(cfg, W, nz, torch.float64, T, B)
    assert torch.equal(f32['actions'], f64['actions']) and torch.equal(f32['lens'], f64['lens'])
    for k in ('latents', 'agent_embed', 'rewards', 'values', 'log_probs'):
        a, b = f32[k].double(), f64[k]
        gap = ((a - b).abs() / (2e-4 + 1e-4 * b.abs())).max().item()
        print(f'{name} {k}: max |f32 - f64| {(a - b).abs().max().item():.2e} at scale {b.abs().max().item():.2g}, {gap:.3f} of the tolerance')
        assert gap <= 0.1, (k, gap)


def test_option_builds_a_deep_model_on_the_cpu():
    from dreamer4_amd import _lib
    m = small_model(depth=40, time_block_every=4, wide_frames=True)
    assert m.wide_frames is True and m.depth == 40
    c = m._make_config((1, 4, 1, 0))
    assert (c.depth, c.wide_frames) == (40, 1)
    assert _lib.Config._fields_[-1] == ('wide_frames', _lib.C.c_int32)
    assert 'd4_pool_mix_deep' in _lib.SYMBOLS and _lib.SYMBOLS['d4_pool_mix_deep'] == _lib.SYMBOLS['d4_pool_mix']
