"""Host: the inputs and the bound of tests/test_gpu_wide_infer.py's operator cases can see the errors those tests are for, and the
wide_frames option is recorded like the other constructor arguments.

For every case of tests/wide_infer_cases.py the float32 evaluation of attn_core_ref.small_attn_ref stays within the recorded E32 of the
'small_attn' family against its float64 evaluation (the wide shapes need no bound of their own), and every applicable mutation moves the
output by at least 10 x the GPU bound, on the very inputs the GPU test uses."""
import torch

import attn_core_cases as K
import attn_core_ref as R
import wide_infer_cases as W

ROOM = 10


def test_case_table_covers_what_it_names():
    names = [c['name'] for c in W.WIDE]
    assert len(set(names)) == len(names)
    assert (W.E32, W.BOUND) == (K.E32['small_attn'], 8 * K.E32['small_attn'])
    assert {c['form'] for c in W.WIDE} == {'wide_attn_kernel<16>', 'wide_attn_kernel<32>', 'wide_attn_kernel<64>'}
    assert all(c['nq'] > 64 or c['nk'] > 64 for c in W.WIDE) and all(max(c['nq'], c['nk']) <= 1024 for c in W.WIDE)
    assert all(c['align'] == 'ok' and c['restrict'] is None and (not c['belief'] or c['nq'] == c['nk']) for c in W.WIDE)
    self_n = {c['nq'] for c in W.WIDE if c['belief'] and c['name'].startswith('self-')}
    assert self_n == {65, 79, 80, 81, 128, 129, 257, 1024}
    assert {(c['nq'], c['ms']) for c in W.WIDE if c['name'].startswith('special-')} == {(80, 16), (70, 10), (130, 70), (97, 1), (97, 0)}
    assert {(c['nq'], c['nk']) for c in W.WIDE if not c['belief']} == {(1, 1023), (1, 1024), (5, 200), (70, 200), (300, 16), (16, 300), (65, 64), (64, 65)}
    assert sum(c['ob'] for c in W.WIDE) == 2 and any(not c['gate'] for c in W.WIDE) and {c['clamp'] for c in W.WIDE} == {50., 3.}
    assert {c['vres'] for c in W.WIDE if c['belief']} == {0, 1} and any(c['q0'] for c in W.WIDE)


def test_wide_inputs_see_every_mutation():
    rows = []
    for c in W.WIDE:
        d = K.small_attn_inputs(c)
        ref = K.small_attn_expect(c, d)
        mv = {m: R.rel_err(K.small_attn_expect(c, d, mut=(m,)), ref) for m in K.small_attn_mutations(c)}
        rows.append((c['name'], R.rel_err(K.small_attn_expect(c, d, torch.float32), ref), mv))
    for n, e, mv in rows:
        print(f'{n}: E32 {e:.3e}; ' + ', '.join(f'{m} {v:.2e}' for m, v in mv.items()))
    bad = [f'{n}: float32 evaluation {e:.3e} above the recorded E32 {W.E32:.3e}' for n, e, _ in rows if not e <= W.E32]
    bad += [f'{n}: {m} moves the output by {v:.3e} only (< {ROOM} x bound {W.BOUND:.3e})' for n, _, mv in rows for m, v in mv.items() if not v >= ROOM * W.BOUND]
    assert not bad, '\n'.join(bad)
    assert {m for _, _, mv in rows for m in mv} == {'drop_newest', 'drop_oldest', 'extra_key', 'mask_row', 'no_belief', 'no_vres', 'scale64', 'gamma_only'}


def test_wide_frames_is_a_recorded_constructor_argument():
    from dreamer4_amd import DynamicsWorldModel, VideoTokenizer, _lib
    kw = dict(dim=32, dim_latent=8, num_latent_tokens=4, num_spatial_tokens=4, num_register_tokens=1, depth=2, time_block_every=2, attn_heads=2,
              attn_dim_head=16, max_steps=8)
    off, on = DynamicsWorldModel(**kw), DynamicsWorldModel(**kw, wide_frames=True, train_wide_frames=False)
    assert off.wide_frames is False and on.wide_frames is True and on.train_wide_frames is False
    assert DynamicsWorldModel(**kw, train_wide_frames=True).wide_frames is False                 # independent of the training option
    assert on._config[1]['wide_frames'] is True and off._config[1]['wide_frames'] is False
    assert off._make_config((1, 4, 1, 0)).wide_frames == 0 and on._make_config((1, 4, 1, 0)).wide_frames == 1
    tk = dict(dim=32, dim_latent=8, patch_size=4, image_height=8, image_width=8, num_latent_tokens=4, encoder_depth=2, decoder_depth=2, time_block_every=2, attn_heads=2)
    assert VideoTokenizer(**tk).wide_frames is False
    tok = VideoTokenizer(**tk, wide_frames=True)
    assert tok.wide_frames is True and tok._config[1]['wide_frames'] is True
    assert _lib.Config._fields_[-1] == ('wide_frames', _lib.C.c_int32) and 'd4_small_attn_wide' in _lib.SYMBOLS
    assert _lib.SYMBOLS['d4_small_attn_wide'] == _lib.SYMBOLS['d4_small_attn']
