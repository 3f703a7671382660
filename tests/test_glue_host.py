"""Host: the inputs and the bounds of tests/test_gpu_glue.py (the glue launchers called alone) can see the errors those tests are for.

For every case of the numeric families of tests/glue_cases.py the float64 reference is evaluated once as it is and once per applicable mutation
(glue_ref.MUTATIONS): every mutation must move an output by at least 10 x the GPU bound, on the very inputs the GPU test uses.  The float32
evaluation of each reference stays within the recorded E32 of its float64 evaluation, and the recorded E32 is at most twice the measured one — the
measurement the bound is derived from.  For the families compared bit for bit (bf16 images, token assembly, index permutations, colsum_batch) every
mutation changes at least one bit of the expected output.  The float64 AdamW reference is checked against torch.optim.AdamW + clip_grad_norm_."""
import itertools

import pytest
import torch

import attn_core_cases as K
import deep_pool_cases as P
import fused_cases as FC
import glue_cases as GC
import glue_ref as G
import train_core_cases as TC
import wide_bf16_cases as W16
import wide_infer_cases as WI
from test_attn_cores_host import ROOM

SEEN = {
    'rmsnorm_rows': {'last_row', 'last_col', 'last_f4', 'no_eps', 'no_gamma'},
    'layernorm_rows': {'last_row', 'last_col', 'no_mean', 'no_eps', 'var_dm1', 'no_bias', 'no_silu'},
    'gather_space': {'last_row', 'last_col', 'last_f4', 'no_gamma', 'no_eps', 'no_second', 'first_zero'},
    'rmsnorm_bwd': {'last_row', 'no_eps', 'no_gamma', 'no_proj'},
    'colsum': {'last_row', 'last_col', 'skip64', 'last_chunk'},
    'adamw': {'no_bias_corr', 'l2_decay', 'clip_always', 'scale_not_in_norm', 'tail'},
    'adamw_wide': {'no_bias_corr', 'l2_decay', 'clip_always', 'scale_not_in_norm', 'tail'},
    'splitk_reduce': {'last_row', 'last_col', 'last_slice', 'no_bias', 'no_silu'},
    'mean_tokens': {'last_row', 'last_col', 'last_token', 'sum_not_mean'},
    'hl_gauss_scalar': {'last_row', 'last_col'},
    'euler_step': {'last_row', 'last_col', 'no_div'},
    'unary': {'last_col'},
    'build_latent_input': {'stride_as_tq', 'no_last'},
    'silu_bwd': {'last_col', 'sig_only'},
    'layernorm_silu_bwd': {'last_row', 'last_col', 'no_bias', 'no_silu', 'sig_only', 'no_mean_term', 'no_proj', 'no_eps'},
    'swiglu': {'last_row', 'last_col', 'halves_swapped', 'pad_unzeroed', 'sig_only'},
}


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def test_case_tables_cover_what_they_name():
    seeds = [c['seed'] for t in GC.ALL_TABLES.values() for c in t]
    names = [c['name'] for t in GC.ALL_TABLES.values() for c in t]
    assert len(set(seeds)) == len(seeds) and len(set(names)) == len(names) and min(seeds) >= 20000
    other = [c['seed'] for t in (K.SMALL_ATTN, K.POOL_MIX, K.TIME, FC.FRAME_ATTN_OUT, FC.ATTN_OUT_COLS, FC.FRAME_POOL, P.DEEP, TC.SELF, TC.CROSS, W16.WIDE16, WI.WIDE)
             for c in t]
    assert set(seeds).isdisjoint(other) and len(other) > 100
    assert GC.BOUND == {f: 8 * e for f, e in GC.E32.items()} and set(GC.E32) == set(GC.NUMERIC) == set(SEEN)
    for fam, forms in GC.FORMS.items():                      # every form of every family of the form record is named by a case
        assert {c['form'] for c in GC.ALL_TABLES[fam]} == forms, fam
    rn = GC.RMSNORM
    assert {c['D'] for c in rn if c['form'] == 'vec'} >= {4, 252, 4096} and {c['D'] for c in rn if c['form'] == 'scalar'} >= {1, 6, 65, 4100}
    assert {c['rows'] for c in rn} == {1, 4, 5} and {(c['form'], c['gamma']) for c in rn} >= {('vec', 'null'), ('scalar', 'null'), ('scalar', 'off')}
    assert any(c['D'] == 64 and c['pad'] == 3 for c in rn)                               # ldx = 67
    for c in rn:                                             # the form a case names is the one the launcher's rule picks
        vec = c['D'] % 4 == 0 and c['D'] <= 4096 and c['pad'] % 4 == 0 and c['gamma'] != 'off'
        assert c['form'] == ('vec' if vec else 'scalar'), c['name']
    ln = GC.LAYERNORM
    assert {c['D'] for c in ln} == {1, 63, 64, 65, 4095, 4096} and {c['rows'] for c in ln} == {1, 5}
    assert {c['bias'] for c in ln} == {0, 1} == {c['silu'] for c in ln} and any(c['pad'] for c in ln)
    gs = GC.GATHER_SPACE
    assert {(c['D'], c['off']) for c in gs if c['form'] == 'generic'} >= {(96, 0), (512, 1)}
    assert all(c['first'] > 0 and c['ns'] < c['S'] and c['first'] + c['ns'] <= c['S'] for c in gs) and any(c['frames'] * c['ns'] % 4 for c in gs)
    for c in gs:
        regs = {256: 'regs<1>', 512: 'regs<2>', 1024: 'regs<4>'}.get(c['D']) if c['off'] % 4 == 0 else None
        assert c['form'] == (regs or 'generic'), c['name']
    rb = GC.RMSNORM_BWD
    assert {c['D'] for c in rb} == {6, 64, 65, 1000} and {c['rows'] for c in rb} == {1, 7} and {c['dx'] for c in rb} == {0, 1}
    cs = GC.COLSUM
    assert {(c['rows'], c['cols']) for c in cs if c['form'] == 'plain' and not c['scratch']} == {(1, 1), (63, 17), (64, 16), (1025, 33), (8200, 20)}
    assert {(c['rows'], c['cols']) for c in cs if c['form'] == 'chunked'} == {(8192, 20), (8193, 35), (9000, 16)}
    assert all(c['pad'] > 0 for c in cs if c['form'] == 'chunked') and any(c['scratch'] == 16 * c['cols'] for c in cs if c['form'] == 'chunked')
    for c in cs:
        assert c['form'] == ('chunked' if c['scratch'] >= 16 * c['cols'] and c['rows'] >= 8192 else 'plain'), c['name']
    assert any(c['form'] == 'plain' and c['scratch'] == 16 * c['cols'] - 1 and c['rows'] >= 8192 for c in cs)
    assert [len(c['shapes']) for c in GC.COLSUM_BATCH] == [1, 4] and GC.COLSUM_BATCH[1]['shapes'] == [(5, 3), (1030, 16), (64, 33), (2, 100)]
    cv = GC.CVT_ROWS
    assert any(c['form'] == 'scalar' and c['cols'] == 37 for c in cv) and any(c['form'] == 'scalar' and c['lds'] == 101 for c in cv)
    assert any(c['form'] == 'scalar' and c['off'] == 1 for c in cv) and all(c['ldd'] > c['cols'] for c in cv)
    assert any(c['form'] == 'vec4' and c['rows'] * c['cols'] > 8192 * 256 * 4 for c in cv) and any(c['form'] == 'scalar' and c['rows'] * c['cols'] > 8192 * 256 for c in cv)
    for c in cv:
        v4 = c['cols'] % 4 == 0 and c['lds'] % 4 == 0 and c['ldd'] % 4 == 0 and c['off'] % 4 == 0
        assert c['form'] == ('vec4' if v4 else 'scalar'), c['name']
    assert [c['n'] for c in GC.CVT_FLAT] == [1, 255, 4096 * 256 + 257]
    aw = GC.ADAMW
    assert {c['n'] for c in aw} == {7, 1000, 4096 * 256 + 1000} and {c['clip'] for c in aw} == {'off', 'inactive', 'active'}
    assert len({(c['clip'], c['grad_scale'], c['wd']) for c in aw if c['n'] <= 1000}) == 12      # the full cross of the three options
    assert [(c['cols'], c['cols_pad']) for c in GC.CVT_PAD[:5]] == [(1, 8), (7, 8), (8, 8), (9, 16), (100, 104)] and all(c['lds'] % 4 for c in GC.CVT_PAD)
    assert GC.CVT_PAD[5]['rows'] * GC.CVT_PAD[5]['cols_pad'] // 8 > 8192 * 256 and all(c['ldd'] > c['cols_pad'] and c['ldd'] % 8 == 0 for c in GC.CVT_PAD)
    assert [(c['rows'], c['cols'], c['rows_pad']) for c in GC.CVT_TRANSPOSE] == [(1, 1, 8), (31, 33, 32), (32, 32, 32), (33, 31, 40), (100, 70, 104)]
    assert all(c['ldd'] > c['rows_pad'] for c in GC.CVT_TRANSPOSE)
    sk = GC.SPLITK
    assert {c['S'] for c in sk} == {1, 3, 8} and {c['bias'] for c in sk} == {0, 1} == {c['silu'] for c in sk} and all(c['pad'] for c in sk)
    assert {c['n'] for c in GC.MEAN_TOKENS} >= {1, 7, 8, 9, 17} and {c['bins'] for c in GC.HL_GAUSS} == {1, 63, 64, 65, 255} and all(c['out_stride'] == 3 for c in GC.HL_GAUSS)
    assert any(c['B'] == 3 and c['padx'] and c['padp'] for c in GC.EULER) and {c['op'] for c in GC.UNARY} == {'silu', 'tanh'}
    for table, size in ((sk, lambda c: c['M'] * c['N']), (GC.MEAN_TOKENS, lambda c: c['B'] * c['d']), (GC.EULER, lambda c: c['B'] * c['n_el']), (GC.UNARY, lambda c: c['n']),
                        (GC.SILU_BWD, lambda c: c['n'])):
        assert max(size(c) for c in table) > GC.GRID1D                # one case of every grid1d kernel takes a second trip of its stride loop
    assert {(c['D'], c['pad'] > 0) for c in GC.LN_SILU_BWD} >= {(5, True), (64, True), (130, True)} and {c['rows'] for c in GC.LN_SILU_BWD} == {1, 5}
    for w in ('fwd', 'bwd'):                                 # grid_for of backward.hip: 4096 x 256 threads
        sw = [c for c in GC.SWIGLU if c['which'] == w]
        assert {(c['inner'], c['inner_pad']) for c in sw} >= {(5, 16), (16, 16), (100, 112)} and max(c['rows'] * c['inner_pad'] for c in sw) >= 4096 * 256 + 777
        assert all(c['inner_pad'] == (c['inner'] + 15) // 16 * 16 for c in sw)


def test_assemble_cases_cover_every_pair_and_both_grids():
    cs = [c for c in GC.ASSEMBLE if c['B'] * c['Tq'] == 6]
    for a, b in itertools.combinations(GC.ASSEMBLE_FACTORS, 2):
        have = {(c[a], c[b]) for c in cs}
        want = set(itertools.product({c[a] for c in cs}, {c[b] for c in cs}))
        assert have == want, (a, b, sorted(want - have))
    assert {c['act'] for c in cs} == set(GC.ACTIONS) and {c['form'] for c in cs} == {'vec4', 'scalar'}
    for c in GC.ASSEMBLE:
        assert c['form'] == ('vec4' if c['D'] % 8 == 0 and not c['off'] else 'scalar') and c['D'] % 2 == 0
    assert {(c['D'], c['off']) for c in cs if c['form'] == 'scalar'} == {(36, 0), (40, 1)}
    big = {c['form']: c['B'] * c['Tq'] * c['S'] * c['D'] for c in GC.ASSEMBLE if c['B'] * c['Tq'] > 6}
    assert big['vec4'] // 4 > GC.GRID1D and big['scalar'] > GC.GRID1D          # a second trip of the grid-stride loop in either kernel
    d = GC.assemble_inputs(GC.ASSEMBLE[0])
    assert d['prev_actions'][2, 0] == -1 and (d['prev_actions'][[0, 1, 3, 4, 5], 0] >= 0).all()
    d = GC.assemble_inputs(GC.ASSEMBLE[1])
    assert d['prev_cont'][2, 0].isnan() and d['prev_cont'].isnan().sum() == 1


@pytest.mark.parametrize('family', sorted(GC.NUMERIC))
def test_numeric_inputs_see_every_mutation(family):
    table, inputs, expect, mutations = GC.NUMERIC[family]
    e32, bound = GC.E32[family], GC.BOUND[family]
    rows = []
    for c in table:
        d = inputs(c)
        ref = expect(c, d)
        mv = {m: G.rel_err_all(expect(c, d, mut=(m,)), ref) for m in mutations(c)}
        rows.append((c['name'], G.rel_err_all(expect(c, d, torch.float32), ref), mv))
    seen = {m for _, _, mv in rows for m in mv}
    worst = max(rows, key=lambda r: r[1])
    least = min((v, m, n) for n, _, mv in rows for m, v in mv.items())
    print(f'{family}: E32 measured {worst[1]:.3e} ({worst[0]}), recorded {e32:.3e}, GPU bound {bound:.3e}; smallest movement {least[0]:.3e} ({least[1]} at {least[2]}) '
          f'= {least[0] / bound:.0f} x bound; per mutation: ' + ', '.join(f'{m} {min(mv[m] for _, _, mv in rows if m in mv):.2e}' for m in sorted(seen)))
    bad = [f'{n}: float32 evaluation {e:.3e} above the recorded E32 {e32:.3e}' for n, e, _ in rows if not e <= e32]
    bad += [f'{n}: {m} moves the output by {v:.3e} only (< {ROOM} x bound {bound:.3e})' for n, _, mv in rows for m, v in mv.items() if not v >= ROOM * bound]
    assert not bad, '\n'.join(bad)
    assert worst[1] >= e32 / 2, 'the recorded E32 is more than twice what this table measures'
    assert seen == SEEN[family]


def test_bf16_inputs_hold_the_ties_and_see_truncation():
    for c in GC.CVT_ROWS + GC.CVT_FLAT:
        x = GC.cvt_rows_inputs(c)['x'] if 'rows' in c else GC.bf16_input(c['seed'], c['n'])
        b = bits(x.reshape(-1)).long() & 0xFFFFFFFF
        assert not x.isnan().any() and ((b >> 23) & 0xFF).min() >= 0 and not (((b >> 23) & 0xFF == 0) & (b & 0x7FFFFF != 0)).any()         # no NaN, no subnormal
        ref = G.bf16_ref(x)
        if x.numel() >= 255:
            tie = (b & 0xFFFF) == 0x8000
            up = tie & ((b >> 16) & 1 == 1)
            assert up.sum() > 10 and (tie & ~up).sum() > 10                                # ties that round up and ties that round down
            for v in (0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF):
                assert (b == v).any()
            assert ref.reshape(-1)[4].isinf()                                              # the largest finite float rounds to infinity
        muts = ['truncate'] if x.numel() > 1 else []
        muts += ['last_row', 'last_col'] if 'rows' in c else []
        for m in muts:
            assert not torch.equal(bits(G.bf16_ref(x, mut=(m,))), bits(ref)), (c['name'], m)
    t = torch.tensor([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001], dtype=torch.int32).view(torch.float32)
    assert (bits(G.bf16_ref(t)).long() & 0xFFFF).tolist() == [0x3F80, 0x3F82, 0x3F80, 0x3F81]
    assert (bits(G.bf16_ref(t, mut=('truncate',))).long() & 0xFFFF).tolist() == [0x3F80, 0x3F81, 0x3F80, 0x3F80]


def test_padded_bf16_images_see_their_mutations():
    for c in GC.CVT_PAD[:5] + GC.CVT_TRANSPOSE:
        x = GC.cvt_rows_inputs(c)['x']
        ref = (lambda m=(): G.cvt_pad_ref(x, c['cols_pad'], m)) if 'cols_pad' in c else (lambda m=(): G.cvt_transpose_ref(x, c['rows_pad'], m))
        want = ref()
        inner = (c['rows'], c['cols']) if 'cols_pad' in c else (c['cols'], c['rows'])
        assert want.shape == (inner[0], c.get('cols_pad', c.get('rows_pad'))) and (want[:, inner[1]:] == 0).all() and not want.isnan().any()
        if 'rows_pad' in c:
            assert torch.equal(bits(want[:, :c['rows']]), bits(x.t().to(torch.bfloat16)))
        for m in ['pad_unzeroed'] * (want.shape[1] > inner[1]) + ['truncate'] * (x.numel() >= 32):
            assert not torch.equal(bits(ref((m,))), bits(want)), (c['name'], m)


def _differs(a, b):
    return not torch.equal(bits(a), bits(b))


def test_permutation_references_see_exchanged_axes_and_wrong_extents():
    assert all(c['nh'] != c['nw'] and c['T'] != c['nh'] and c['B'] != c['C'] for c in GC.VIDEO[:1]) and GC.VIDEO[0]['ps'] == 2      # no exchanged pair of axes cancels
    c = GC.VIDEO[0]
    v = GC.rand(c, c['B'], c['C'], c['T'], c['nh'] * c['ps'], c['nw'] * c['ps'])
    p = G.video_to_patches_ref(v, c['ps'])
    assert p.shape == (c['B'] * c['T'] * c['nh'] * c['nw'], c['ps'] ** 2 * c['C']) and p[(1 * 5 + 2) * 12 + 1 * 4 + 3, (1 * 2 + 0) * 3 + 2] == v[1, 2, 2, 1 * 2 + 1, 3 * 2 + 0]
    assert torch.equal(G.patches_to_video_ref(p, c['B'], c['C'], c['T'], c['nh'], c['nw'], c['ps']), v)                  # the round trip
    for m in ('swap_hw', 'swap_p', 'swap_th'):
        assert _differs(G.video_to_patches_ref(v, c['ps'], (m,)), p), m
    for m in ('swap_hw', 'swap_p'):
        assert _differs(G.patches_to_video_ref(p, c['B'], c['C'], c['T'], c['nh'], c['nw'], c['ps'], (m,)), v), m
    for c in GC.CACHE:
        assert c['cache_batch'] > c['B'] and c['Tcap'] > c['frames'] and len({c['Lt'], c['cache_batch'], c['S'], c['H'], c['Tcap'], c['frames']}) == 6
        cache = GC.rand(c, c['Lt'], 2, c['cache_batch'] * c['S'], c['H'], c['Tcap'], c['dh'])
        ext = G.cache_to_ext_ref(cache, c['B'], c['S'], c['frames'])
        assert ext.shape == (c['Lt'], 2, c['B'] * c['S'], c['H'], c['frames'], c['dh']) and ext[1, 1, 4, 3, 6, 5] == cache[1, 1, 4, 3, 6, 5]
        empty = torch.full_like(cache, float('nan'))
        back = G.ext_to_cache_ref(ext, empty)
        assert back.isnan().sum() == cache.numel() - ext.numel() and torch.equal(back[:, :, :c['B'] * c['S'], :, :c['frames']], ext)
        for m in ('batch_as_b', 'tcap_as_frames', 'swap_bcol'):                           # either direction sees each
            assert _differs(G.cache_to_ext_ref(cache, c['B'], c['S'], c['frames'], (m,)), ext), m
            assert _differs(G.ext_to_cache_ref(ext, empty, (m,)), back), m
    assert {c['dh'] for c in GC.CACHE} == {16, 32, 64}
    assert max(c['Lt'] * 2 * c['B'] * c['S'] * c['H'] * c['frames'] * c['dh'] for c in GC.CACHE) >= GC.PAST_GRID    # a second trip of cache_transfer's stride loop
    c = GC.CUNEMBED[0]
    U = GC.rand(c, c['nc'], c['mtp'], c['d'], 2)
    w = G.cunembed_gather_ref(U)
    assert c['mtp'] > 1 and w.shape == (2 * c['nc'], c['d']) and w[2 * 1 + 1, 3] == U[1, 0, 3, 1] and _differs(G.cunembed_gather_ref(U, ('head1',)), w)
    dU = G.cunembed_scatter_ref(w, c['nc'], c['mtp'], c['d'])
    assert torch.equal(dU[:, 0], U[:, 0]) and (dU[:, 1:] == 0).all() and _differs(G.cunembed_scatter_ref(w, c['nc'], c['mtp'], c['d'], ('head1',)), dU)
    for c in GC.COORD:
        g = G.coord_grid_ref(c['nh'], c['nw'], c['ld'])
        assert (g[:, 2:] == 0).all() and not g.isnan().any()
        want = torch.stack(torch.meshgrid(torch.linspace(-1, 1, c['nh']) if c['nh'] > 1 else torch.tensor([-1.]),
                                          torch.linspace(-1, 1, c['nw']) if c['nw'] > 1 else torch.tensor([-1.]), indexing='ij'), -1).reshape(-1, 2)
        assert (g[:, :2] - want).abs().max() <= 1.2e-7                       # torch.linspace to the last bit or the one before (contraction)
        if c['nh'] in (1, 2, 3, 5, 9) and c['nw'] in (1, 2, 3, 5, 9):
            assert torch.equal(g[:, :2], want)                               # dyadic steps: nothing rounds
        if c['nh'] != c['nw']:
            assert _differs(G.coord_grid_ref(c['nh'], c['nw'], c['ld'], ('swap_hw',)), g)
        if c['ld'] > 2:
            assert _differs(G.coord_grid_ref(c['nh'], c['nw'], c['ld'], ('pad_unzeroed',)), g)
    assert any(c['nh'] == 1 for c in GC.COORD) and any(c['nw'] == 1 for c in GC.COORD)
    c = GC.PACK[0]
    assert c['n_total'] > c['n_lat']
    pos, img, lat = GC.rand(c, c['P'], c['D']), GC.rand(dict(seed=c['seed'] + 50), c['frames'], c['P'], c['D']), GC.rand(dict(seed=c['seed'] + 60), c['frames'], c['n_total'], c['D'])
    tok, comp = G.decoder_pack_ref(pos, img, lat, c['n_lat'])
    assert tok.shape == (3, 7, 7) and torch.equal(tok[2, 6], lat[2, 1]) and torch.equal(comp, tok[:, :5]) and _differs(G.decoder_pack_ref(pos, img, lat, c['n_lat'], ('all_latents',))[0], tok)
    assert _differs(G.pad_cols_ref(pos, 12, ('pad_unzeroed',)), G.pad_cols_ref(pos, 12)) and (G.pad_cols_ref(pos, 12)[:, 7:] == 0).all()
    for table, size in ((GC.COPY_ROWS, lambda c: c['rows'] * c['cols']), (GC.PAD_COLS, lambda c: c['rows'] * c['cols_pad']), (GC.CUNEMBED, lambda c: 2 * c['nc'] * c['d']),
                        (GC.CACHE, lambda c: c['Lt'] * 2 * c['B'] * c['S'] * c['H'] * c['frames'] * c['dh']),
                        (GC.VIDEO, lambda c: c['B'] * c['C'] * c['T'] * c['nh'] * c['nw'] * c['ps'] ** 2), (GC.PACK, lambda c: c['frames'] * (c['P'] + c['n_lat']) * c['D'])):
        assert max(size(c) for c in table) > GC.GRID1D                       # a second trip of the grid-stride loop


def test_weight_packing_and_latent_references():
    for c in GC.FOLD[:2]:
        W, gamma = GC.rand(c, c['rows'], c['K']), GC.rand(dict(seed=c['seed'] + 50), c['K']) if c['gamma'] else None
        ref = G.fold_rows_ref(W, gamma)
        assert _differs(G.fold_rows_ref(W, gamma, ('last_row',)), ref) and (gamma is None or _differs(G.fold_rows_ref(W, gamma, ('no_gamma',)), ref))
        assert gamma is not None or torch.equal(ref, W)
    assert [(c['inner'], c['inner_pad']) for c in GC.SWIGLU_PACK[:3]] == [(5, 32), (32, 32), (40, 64)] and {c['gamma'] for c in GC.FOLD} == {0, 1}
    for c in GC.SWIGLU_PACK[:3]:
        i, ip, k = c['inner'], c['inner_pad'], c['K']
        W, bias, gamma = GC.rand(c, 2 * i, k), GC.rand(dict(seed=c['seed'] + 50), 2 * i), GC.rand(dict(seed=c['seed'] + 60), k)
        Wp, bp = G.swiglu_pack_ref(W, bias, gamma, i, ip)
        assert Wp.shape == (2 * ip, k) and torch.equal(Wp[3], W[3] * gamma) and torch.equal(Wp[32 + 3], W[i + 3] * gamma) and bp[32 + 3] == bias[i + 3]
        if i == 40:
            assert torch.equal(Wp[64 + 7], W[39] * gamma) and torch.equal(Wp[96 + 7], W[79] * gamma) and (Wp[64 + 8:96] == 0).all() and (bp[96 + 8:] == 0).all()
        for m in ['no_gamma', 'gate_first'] + (['pad_unzeroed'] if ip > i else []):
            W2, b2 = G.swiglu_pack_ref(W, bias, gamma, i, ip, (m,))
            assert _differs(W2, Wp) or _differs(b2, bp), (c['name'], m)
    exact = [c for c in GC.BUILD_LATENT if c['w'] in (0., 1.)]
    assert {c['w'] for c in exact} == {0., 1.} and all(c['stride'] > c['Tq'] for c in GC.BUILD_LATENT) and any(not c['ctx'] for c in GC.BUILD_LATENT)
    for c in exact:                                          # at w = 0 and 1 the lerp is a copy: compared bit for bit
        d = GC.latent_inputs(c)
        ref = G.build_latent_ref(d['hist'], d['ctx'], d['x'], Tq=c['Tq'], w=c['w'], dtype=torch.float32)
        src = d['hist'] if c['w'] == 0. else d['ctx']
        assert torch.equal(ref[:, :2], src[:, :2]) and torch.equal(ref[:, 2], d['x'])
    assert max(c['B'] * c['Tq'] * c['n_el'] for c in GC.BUILD_LATENT) > GC.GRID1D and max(2 * c['inner_pad'] * c['K'] for c in GC.SWIGLU_PACK) > GC.GRID1D
    assert max(c['rows'] * c['K'] for c in GC.FOLD) > GC.GRID1D


def test_assemble_reference_sees_every_mutation():
    seen = set()
    for c in GC.ASSEMBLE[:9]:
        d = GC.assemble_inputs(c)
        tok, comp = G.assemble_ref(c, d)
        assert tok.shape == (c['B'] * c['Tq'], c['S'], c['D']) and (comp is None) == (not c['compact'])
        if c['na'] or c['nc']:
            a = 1 + c['ns'] + c['nr']
            assert (tok[2, a] == 0).all() and (tok[[0, 1, 3, 4, 5], a] != 0).any(-1).all()      # the frame with the sentinel has a zero action token
        for m in GC.assemble_mutations(c):
            t2, c2 = G.assemble_ref(c, d, mut=(m,))
            changed = not torch.equal(bits(t2), bits(tok)) or (comp is not None and not torch.equal(bits(c2), bits(comp)))
            assert changed, (c['name'], m)
            seen.add(m)
    assert seen == {'last_row', 'no_offset', 'no_sentinel', 'rank_off', 'no_task'}


def test_colsum_batch_reference_sees_a_shifted_first_block():
    c = GC.COLSUM_BATCH[1]
    mats = GC.colsum_batch_inputs(c)['mats']
    ref, off = G.colsum_batch_ref(mats), G.colsum_batch_ref(mats, mut=('first_off',))
    assert torch.equal(ref[0], off[0]) and all(not torch.equal(a, b) for a, b in zip(ref[1:], off[1:]))
    for x, r in zip(mats, ref):                              # the batch sums what colsum sums
        assert torch.equal(r, G.colsum_ref(x))


@pytest.mark.parametrize('c', [c for c in GC.ADAMW if c['n'] <= 1000], ids=lambda c: c['name'])
def test_adamw_reference_is_torch_adamw_with_clip_grad_norm(c):
    d = GC.adamw_inputs(c)
    p = torch.nn.Parameter(d['p'].double().clone())
    opt = torch.optim.AdamW([p], lr=c['lr'], betas=(c['b1'], c['b2']), eps=c['eps'], weight_decay=c['wd'])
    ref = G.adamw_ref(d['p'], d['grads'], lr=c['lr'], b1=c['b1'], b2=c['b2'], eps=c['eps'], wd=c['wd'], max_norm=d['max_norm'], grad_scale=c['grad_scale'])
    for t in range(GC.ADAMW_STEPS):
        p.grad = d['grads'][t].double() * c['grad_scale']
        norm = torch.nn.utils.clip_grad_norm_([p], d['max_norm']) if d['max_norm'] > 0 else p.grad.norm()
        opt.step()
        st = opt.state[p]
        for got, want in zip(ref[t], (p.detach(), st['exp_avg'], st['exp_avg_sq'], norm.reshape(1))):
            assert G.rel_err_all((got,), (want,)) <= 1e-12


def test_prep_eval_cases_and_reference():
    pe = GC.PREP_EVAL
    assert all(c['hist_stride'] > c['Tq'] for c in pe) and {c['frame_base'] > 0 for c in pe} == {False, True} and any(not c['hist'] for c in pe)
    assert {(c['na'] > 0, c['nc'] > 0) for c in pe} == {(True, False), (False, True), (True, True)} and max(c['B'] * c['Tq'] for c in pe) > 128
    seen = set()
    for c in pe:
        d = GC.prep_inputs(c)
        sig, pact, pcont = GC.prep_expect(c, d)
        B, Tq = c['B'], c['Tq']
        assert sig.dtype == torch.int32 and sig.reshape(B, Tq)[:, -1].eq(c['sig_val']).all() and (Tq == 1 or sig.reshape(B, Tq)[:, :-1].eq(c['ctx_sig']).all())
        first = c['frame_base'] == 0 or not c['hist']                  # the -1 / NaN sentinel: global frame 0, or no history at all
        if c['na']:
            pa = pact.reshape(B, Tq, c['na'])
            assert pa.dtype == torch.int64 and (pa[:, 0] == -1).all() == first and (not c['hist'] or (pa[:, 1:] >= 0).all())
            if c['hist']:
                assert torch.equal(pa[B - 1, Tq - 1], d['hist'][B - 1, c['frame_base'] + Tq - 2]) or (Tq == 1 and first)
        if c['nc']:
            pc = pcont.reshape(B, Tq, c['nc'])
            assert pc[:, 0].isnan().all() == first and (not c['hist'] or not pc[:, 1:].isnan().any())
        for m in GC.prep_mutations(c):
            got = GC.prep_expect(c, d, mut=(m,))
            assert any(_differs(a, b) for a, b in zip(got[1:], (pact, pcont)) if a.numel()), (c['name'], m)
            seen.add(m)
    assert seen == {'last_row', 'stride_as_tq', 'no_sentinel', 'no_base'}


def test_multi_copy_and_zero_pad_cases_and_references():
    ten, one = GC.MULTI_COPY[0], GC.MULTI_COPY[1]
    assert len(ten['segs']) == 10 and len(one['segs']) == 1 and {n for n, _, _ in ten['segs']} >= {1, 3, 4, 5} and max(n for n, _, _ in ten['segs']) > 512 * 256 * 4
    assert sum(s is None for _, _, s in ten['segs']) == 2 and {(d % 4 == 0, s is None or s % 4 == 0) for _, d, s in ten['segs']} >= {(True, True), (False, True), (True, False)}
    assert any(n > 512 * 256 and (d % 4 or (s or 0) % 4) for n, d, s in ten['segs'])       # the scalar loop takes a second trip too
    for c in GC.MULTI_COPY:
        segs, nd, ns = GC.multi_copy_layout(c)
        spans = sorted((d, d + n) for d, _, n in segs)
        assert all(a[1] + 4 <= b[0] + 3 and a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= nd      # no two segments overlap
        assert [(d % 4, None if s is None else s % 4) for d, s, _ in segs] == [(do, so) for _, do, so in c['segs']]
        src, dst0 = GC.rand(c, ns), torch.full((nd,), float('nan'))
        want = G.multi_copy_ref(segs, src, dst0)
        assert want.isnan().sum() == nd - sum(n for _, _, n in segs)
        for d, s, n in segs:
            assert torch.equal(want[d:d + n], torch.zeros(n) if s is None else src[s:s + n])
        for m in ['last_col', 'last_f4'] + (['no_zero'] if any(s is None for _, s, _ in segs) else []):
            got = G.multi_copy_ref(segs, src, dst0, (m,))
            assert not torch.equal(got.isnan(), want.isnan()) or _differs(got.nan_to_num(7.), want.nan_to_num(7.)), (c['name'], m)
    assert max(c['rows'] * (c['c1'] - c['c0']) for c in GC.ZERO_PAD) >= 4096 * 256 + 777 and any(c['c1'] == c['ld'] for c in GC.ZERO_PAD) and any(c['c0'] == 0 for c in GC.ZERO_PAD)
    for c in GC.ZERO_PAD:
        x = GC.rand(c, c['rows'], c['ld'])
        want = G.zero_pad_cols_ref(x, c['c0'], c['c1'])
        assert (want[:, c['c0']:c['c1']] == 0).all() and torch.equal(want[:, :c['c0']], x[:, :c['c0']]) and torch.equal(want[:, c['c1']:], x[:, c['c1']:])
        for m in ['last_row', 'last_col'] + (['ld_as_n'] if c['c1'] - c['c0'] < c['ld'] else []):
            assert _differs(G.zero_pad_cols_ref(x, c['c0'], c['c1'], (m,)), want), (c['name'], m)
