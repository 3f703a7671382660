"""Host: the inputs and the bound of tests/test_gpu_fused_launches.py (the per-frame fused tails) can see the errors those tests are for.

For every case of the shared tables (tests/fused_cases.py) the float64 reference is evaluated once as it is and once per applicable
mutation (fused_ref.MUTATIONS and those of attn_core_ref that apply: the residual dropped, two weight tiles or two k groups exchanged, a row
or a compact rank off by one, c2_last ignored, two pool heads' value blocks exchanged, a key dropped or admitted, belief / value residual /
the hiddens' rms skipped): every mutation must move the output or the compact copy by at least 10 x the GPU bound, on the very inputs the
GPU test uses.  And the float32 evaluation of each reference stays within the recorded E32 of its float64 evaluation — the measurement the
bound is derived from.  The CPU side of the GEMM tests is checked too: the compact gather and the index permutation of tile16_weights."""
import torch

import fused_cases as FC
import fused_ref as F
from test_attn_cores_host import ROOM

ATTN_MUT = {'no_resid', 'k4_swap', 'tile_swap', 'row_shift', 'rank_off', 'last_missing', 'no_belief', 'drop_newest', 'no_vres', 'extra_key'}
POOL_MUT = {'no_resid', 'k4_swap', 'tile_swap', 'row_shift', 'rank_off', 'last_missing', 'head_swap', 'no_rms', 'drop_newest'}


def _check(family, rows):
    """rows: (case name, float32-vs-float64 error, {mutation: movement}) per case"""
    e32, bound = FC.E32[family], FC.BOUND[family]
    bad = [f'{n}: float32 evaluation {e:.3e} above the recorded E32 {e32:.3e}' for n, e, _ in rows if not e <= e32]
    bad += [f'{n}: {m} moves the output by {v:.3e} only (< {ROOM} x bound {bound:.3e})' for n, _, mv in rows for m, v in mv.items() if not v >= ROOM * bound]
    seen = {m for _, _, mv in rows for m in mv}
    print(f'{family}: E32 measured {max(e for _, e, _ in rows):.3e} (recorded {e32:.3e}); smallest movement per mutation: '
          + ', '.join(f'{m} {min(mv[m] for _, _, mv in rows if m in mv):.2e}' for m in sorted(seen)))
    assert not bad, '\n'.join(bad)
    return seen


def _rows(table, inputs, expect, mutations):
    rows = []
    for c in table:
        d = inputs(c)
        ref = expect(c, d)
        mv = {m: F.rel_err2(expect(c, d, mut=(m,)), ref) for m in mutations(c)}
        rows.append((c['name'], F.rel_err2(expect(c, d, torch.float32), ref), mv))
    return rows


def test_case_names_are_unique_and_bounds_follow_e32():
    for table in (FC.FRAME_ATTN_OUT, FC.ATTN_OUT_COLS, FC.FRAME_POOL):
        names = [c['name'] for c in table]
        assert len(set(names)) == len(names)
    assert FC.BOUND == {f: 8 * e for f, e in FC.E32.items()}


def test_case_tables_cover_the_listed_values():
    fa = FC.FRAME_ATTN_OUT
    assert {c['frames'] for c in fa} == {192, 193, 1024} and {c['S'] for c in fa} == {1, 2, 8, 11, 15, 16} and {c['D'] for c in fa} == {256, 288, 512, 544}
    assert all(c['S'] == 2 for c in fa if c['frames'] == 1024)
    for key, vals in (('vres', {0, 1}), ('ms', {0, 1}), ('clamp', {50., 3.}), ('c2', set(FC.C2S)), ('pad', {0, 4})):
        assert {c[key] for c in fa} == vals, key
    ac = FC.ATTN_OUT_COLS
    assert {c['frames'] for c in ac} == {1, 4} and {c['S'] for c in ac} == {1, 11, 16} and {c['D'] for c in ac} == {16, 272, 512} and {c['ldw'] for c in ac} == {512, 516}
    fp = FC.FRAME_POOL
    assert {c['S'] for c in fp if c['frames'] == 192} >= {1, 11, 16} and {c['L'] for c in fp} == {1, 5, 32, 33, 64} and {c['c2'] for c in fp} == set(FC.C2S)
    assert any(c['frames'] == 1024 and c['S'] == 2 and c['L'] == 1 for c in fp)
    assert all(c['L'] * c['M'] * c['D'] * 4 < 100e6 for c in fp), 'the hiddens of a case stay under 100 MB'


def test_frame_attn_out_inputs_see_every_mutation():
    assert _check('frame_attn_out', _rows(FC.FRAME_ATTN_OUT, FC.attn_inputs, FC.attn_expect, FC.attn_mutations)) == ATTN_MUT


def test_attn_out_cols_inputs_see_every_mutation():
    assert _check('attn_out_cols', _rows(FC.ATTN_OUT_COLS, FC.attn_inputs, FC.attn_expect, FC.attn_mutations)) == ATTN_MUT


def test_frame_pool_inputs_see_every_mutation():
    assert _check('frame_pool', _rows(FC.FRAME_POOL, FC.pool_inputs, FC.pool_expect, FC.pool_mutations)) == POOL_MUT


def test_compact_gather_and_tile_permutation():
    out = torch.arange(2 * 7 * 3, dtype=torch.float64).reshape(2, 7, 3)
    assert F.compact_rows(7, 1, 5, 1) == [1, 2, 3, 4, 6] and F.compact_rows(7, 1, 5, 0) == [1, 2, 3, 4] and F.compact_rows(7, 3, 3, 1) == [6]
    assert torch.equal(F.compact_gather(out, (1, 5, 1))[1, 4], out[1, 6]) and F.compact_gather(out, None) is None
    W = torch.arange(32 * 12, dtype=torch.float32).reshape(32, 12)
    t = F.tile16_ref(W, 32, 8)                                 # [2][2][16][4]
    assert t.shape == (2, 2, 16, 4) and t[1, 1, 5, 2] == W[16 + 5, 4 + 2] and t[0, 0, 15, 3] == W[15, 3]
