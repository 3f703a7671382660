"""Host: the bound of tests/test_gpu_train_attn_bf16.py (the bf16-product form of the tiled attention core of the training path,
csrc/attn_tiled_bf16.hip) and the plumbing of the option that needs no GPU.

The bound.  tests/train_bf16_core_ref.py emulates the arithmetic contract, rounding by rounding.  E16[family][tensor] is the largest
train_core_ref.problem_err of that emulation against the exact float64 reference over the core-1 cases of train_core_cases.SELF / CROSS and
four variants (online-softmax tile 64 and 16, everything that is fp32 in the kernels in float64 and in float32), recorded in
train_bf16_core_ref.E16 with a quarter of headroom; the GPU bound is 2 x E16.  Measured (recorded = measured x 1.25):
    self   o3 3.21e-2 (frame-dh16-n33)   dq 2.54e-2 (time-dh16-n100)  dk 1.95e-2 (frame-dh32-n16)   dv 5.46e-2 (frame-dh64-n2)
           dgate 9.37e-2 (frame-dh64-n2) dmix 4.31e-2 (frame-dh64-n2) d_rv 1.06e-2 (time-dh32-n130) dgamma_part 3.76e-2 (time-dh16-n100)
    cross  o3 1.40e-2 (1x74, dh 16)      dq 2.87e-2 (1x1024, dh 16)   dk 2.35e-2 (4x256, dh 32)     dv 2.12e-2 (4x256, dh 32)
           dgate 1.09e-1 (1x1024, dh 64: one scalar per problem)      dgamma_part 2.37e-2 (4x256, dh 32)
With the roundings taken out the emulation is the exact reference (3.7e-14 measured, 1e-12 asserted).  The condition that keeps the bound
from hiding a wrong kernel: every mutation of train_core_cases.mutations moves some tensor of the exact reference by at least 4 x that
tensor's GPU bound on at least two cases.

The plumbing: the world-model option is recorded, independent of the other precision / width options, and survives a checkpoint; 'fp8' is a
ValueError; the switch returns the previous value and refuses 2; the three workspace size queries return today's closed forms with the
switch off and grow linearly in the items with it on (they launch nothing)."""
import collections
import functools

import pytest
import torch

import test_long_clips_host as LC
import test_wide_frames_host as WF
import train_bf16_core_ref as B
import train_core_cases as K
import train_core_ref as R
from dreamer4_amd import _lib

CASES = [c for c in K.SELF + K.CROSS if c['core'] == 1]
VARIANTS = [(tile, dt) for tile in (64, 16) for dt in (torch.float64, torch.float32)]
ROOM = 4


@functools.lru_cache(maxsize=None)
def _measure(key):
    c = next(c for c in CASES if c['key'] == key)
    ref, d = K.expect(c), K.inputs(c)
    exact = K.worst(R.errors(B.evaluate(c, d, rounding=False), ref))
    e16 = {v: R.errors(B.evaluate(c, d, dtype=v[1], tile=v[0]), ref) for v in VARIANTS}
    moved = {m: R.errors(K.evaluate(c, mut=(m,)), ref) for m in K.mutations(c)}
    return exact, e16, moved


def test_the_cases_are_the_core_1_cases():
    assert len(CASES) == len({c['key'] for c in CASES}) and len(CASES) >= 100
    assert {c['items'] for c in CASES if c['family'] != 'cross'} >= {1, 2, 16, 17, 32, 33, 64, 65, 100, 128, 130, 256, 1024}
    assert {(c['nq'], c['nk']) for c in CASES if c['family'] == 'cross'} >= {(1, 1), (64, 64), (1, 74), (4, 256), (130, 5), (65, 65), (1, 1024)}
    assert set(B.E16) == {'self', 'cross'} and B.FACTOR == 2


def test_without_the_roundings_the_emulation_is_the_exact_reference():
    worst = max((_measure(c['key'])[0], c['key']) for c in CASES)
    print(f'emulation without roundings against the exact reference: {worst[0]:.3e} ({worst[1]})')
    assert worst[0] <= 1e-12


def test_the_emulation_stays_within_the_recorded_e16():
    worst = collections.defaultdict(lambda: (0., ''))
    bad = []
    for c in CASES:
        fam = B.family(c)
        for (tile, dt), errs in _measure(c['key'])[1].items():
            for n, (e, _t) in errs.items():
                if e > worst[(fam, n)][0]:
                    worst[(fam, n)] = (e, f"{c['key']}, tile {tile}, {str(dt)[6:]}")
                if not e <= B.E16[fam][n]:
                    bad.append(f"{c['key']} tile {tile} {dt}: {n} {e:.3e} above the recorded E16 {B.E16[fam][n]:.3e}")
    for (fam, n), (e, where) in sorted(worst.items()):
        print(f'E16 {fam} {n}: measured {e:.3e} ({where}), recorded {B.E16[fam][n]:.3e}, GPU bound {B.bound(fam, n):.3e}')
        assert e * 1.25 > 0.8 * B.E16[fam][n], f'the recorded E16 of {fam} {n} is far above the measured {e:.3e} with its quarter of headroom'
    assert {k for k in worst} == {(f, n) for f in B.E16 for n in B.E16[f]} and not bad, '\n'.join(bad)


def test_every_mutation_clears_four_times_the_bound_on_two_cases():
    cleared, applied = collections.defaultdict(list), collections.Counter()
    for c in CASES:
        fam = B.family(c)
        for m, errs in _measure(c['key'])[2].items():
            applied[m] += 1
            if any(e >= ROOM * B.bound(fam, n) for n, (e, _t) in errs.items()):
                cleared[m].append(c['key'])
    for m in sorted(applied):
        print(f'{m}: moves a tensor by >= {ROOM} x its bound on {len(cleared[m])} of {applied[m]} cases')
    assert set(applied) == set(R.MUTATIONS)
    assert all(len(cleared[m]) >= 2 for m in applied), {m: cleared[m] for m in applied if len(cleared[m]) < 2}


# ------------------------------------------------------------------------------------------------------------------- the option
KW = dict(dim=32, dim_latent=8, num_latent_tokens=4, num_spatial_tokens=4, num_register_tokens=1, depth=2, time_block_every=2, attn_heads=2,
          attn_dim_head=16, max_steps=8)


def test_train_attn_products_is_a_recorded_independent_constructor_argument():
    from dreamer4_amd import DynamicsWorldModel
    off, on = DynamicsWorldModel(**KW), DynamicsWorldModel(**KW, train_attn_products='bf16')
    assert (off.train_attn_products, on.train_attn_products) == ('fp32', 'bf16')
    assert off._config[1]['train_attn_products'] == 'fp32' and on._config[1]['train_attn_products'] == 'bf16'
    # needs none of the other options and changes none of them
    assert (on.train_matmul_dtype, on.train_wide_frames, on.matmul_dtype, on.wide_frames, on.attn_products) == ('fp32', False, 'fp32', False, 'fp32')
    m = DynamicsWorldModel(**KW, train_attn_products='bf16', train_matmul_dtype='bf16', train_wide_frames=True, matmul_dtype='bf16', wide_frames=True,
                           attn_products='bf16')
    assert (m.train_attn_products, m.train_matmul_dtype, m.train_wide_frames, m.matmul_dtype, m.wide_frames, m.attn_products) == \
        ('bf16', 'bf16', True, 'bf16', True, 'bf16')
    assert DynamicsWorldModel(**KW, wide_frames=True, attn_products='bf16').train_attn_products == 'fp32'       # the inference option stays the inference option
    assert on._make_config((1, 4, 1, 0)).wide_frames == 0
    for bad in ('fp8', None, 'bf16 '):
        with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
            DynamicsWorldModel(**KW, train_attn_products=bad)


def test_checkpoint_keeps_train_attn_products(tmp_path):
    from dreamer4_amd import DynamicsWorldModel
    path = str(tmp_path / 'm.pt')
    DynamicsWorldModel(**KW, train_attn_products='bf16').save(path)
    back = DynamicsWorldModel.init_and_load(path)
    assert back.train_attn_products == 'bf16' and back.train_wide_frames is False and back.attn_products == 'fp32'


def test_the_operators_refuse_an_unknown_value():
    from dreamer4_amd import trunk_ops
    assert trunk_ops.products_id('fp32') == 0 and trunk_ops.products_id('bf16') == 1
    x = torch.zeros(1, 2, 4)                                         # (the value is checked before anything else: no GPU needed)
    for fn, args in ((trunk_ops.space_attention, (x,) + (None,) * 7), (trunk_ops.time_attention, (x[None],) + (None,) * 8),
                     (trunk_ops.cross_attention, (x, x) + (None,) * 8)):
        with pytest.raises(ValueError, match='fp8'):
            fn(*args, attn_products='fp8')
    with pytest.raises(ValueError, match='fp8'):
        trunk_ops.transformer({}, x[None], is_time=[False], attn_products='fp8')
    with pytest.raises(ValueError, match='fp8'):
        trunk_ops.products_id('fp8')
    assert set(_lib.SYMBOLS) >= {'d4_train_attn_products_set', 'd4_train_attn_core_bf16', 'd4_train_xattn_core_bf16',
                                 'd4_train_attn_core_bf16_plane_floats', 'd4_train_xattn_core_bf16_plane_floats'}
    assert _lib.SYMBOLS['d4_train_attn_core_bf16'] == _lib.SYMBOLS['d4_train_attn_core']
    assert _lib.SYMBOLS['d4_train_xattn_core_bf16'] == _lib.SYMBOLS['d4_train_xattn_core']


def test_the_dispatcher_route_does_not_carry_the_option(monkeypatch):
    from dreamer4_amd import trunk_ops
    monkeypatch.setenv('D4_TRUNK_DISPATCHER', '1')
    with pytest.raises(NotImplementedError, match='attn_products'):
        trunk_ops._no_dispatcher('fp32', False, 'bf16')
    with pytest.raises(ValueError):
        trunk_ops._no_dispatcher('fp32', False, 'fp8')
    trunk_ops._no_dispatcher('fp32', False, 'fp32')


# ------------------------------------------------------------------------------------------------------------------- the switch and the sizes
@pytest.fixture
def lib():
    lib = _lib.load()
    assert lib.d4_train_attn_products_set(0) == 0
    yield lib
    lib.d4_train_wide_set(0)
    lib.d4_train_attn_products_set(0)


def test_the_switch_returns_the_previous_value_and_refuses_2(lib):
    assert lib.d4_train_attn_products_set(1) == 0
    assert lib.d4_train_attn_products_set(1) == 1
    for bad in (2, -1, 5):
        assert lib.d4_train_attn_products_set(bad) == -1
        err = lib.d4_last_error().decode()
        assert 'd4_train_attn_products_set' in err and f'products {bad}' in err, err
        assert lib.d4_train_attn_products_set(1) == 1                # nothing changed
    assert lib.d4_train_attn_products_set(0) == 1
    assert lib.d4_train_attn_products_set(0) == 0


r64 = lambda n: (n + 63) // 64 * 64


def self_planes(groups, items, heads, dh):
    """floats of the fp32 planes of the tiled core (csrc/attn_tiled_rows.h carve): ten [rows][heads][dh] and six [rows][heads], each rounded up to 64"""
    R_ = groups * items
    return 10 * r64(R_ * heads * dh) + 6 * r64(R_ * heads)


def cross_planes(groups, nq, nk, heads, dh):
    return 4 * r64(groups * nq * heads * dh) + 5 * r64(groups * nk * heads * dh) + r64(groups * nk * heads) + 3 * r64(groups * nq * heads)


def images(groups, nq, nk, heads, dh):
    """floats of the bf16 images: four row-major [problem][items][dh], four transposed [problem][dh][items rounded up to 32], each rounded up to 128 elements"""
    r128 = lambda n: (n + 127) // 128 * 128
    gh, p32 = groups * heads, lambda n: (n + 31) // 32 * 32
    return (2 * r128(gh * nq * dh) + 2 * r128(gh * nk * dh) + 2 * r128(gh * dh * p32(nq)) + 2 * r128(gh * dh * p32(nk))) // 2


def time_ws(lib, frames):
    return lib.d4_time_attn_workspace_bytes(LC.BATCH, frames, LC.TOKENS, LC.DIM, LC.HEADS, LC.DH)


def test_switch_off_the_workspaces_are_todays(lib):
    for frames in (16, 64):
        assert time_ws(lib, frames) == LC.lds_core_ws(frames)
    for frames in (65, 100, 256, 1024):
        assert time_ws(lib, frames) == LC.lds_core_ws(frames) + 4 * self_planes(LC.BATCH * LC.TOKENS, frames, LC.HEADS, LC.DH), frames
    for tokens in (16, 64, 70, 256):
        assert WF.space_ws(tokens) == WF.lds_space_ws(tokens)
    for nq, nk in ((1, 7), (64, 64), (4, 256)):
        assert WF.cross_ws(nq, nk) == WF.lds_cross_ws(nq, nk)
    assert lib.d4_train_wide_set(1) == 0
    for tokens in (16, 64):
        assert WF.space_ws(tokens) == WF.lds_space_ws(tokens)
    for tokens in (65, 70, 256):
        assert WF.space_ws(tokens) == WF.lds_space_ws(tokens) + 4 * self_planes(WF.FRAMES, tokens, WF.HEADS, WF.DH), tokens
    for nq, nk in ((4, 256), (65, 3), (1, 65)):
        assert WF.cross_ws(nq, nk) == WF.lds_cross_ws(nq, nk) + 4 * cross_planes(WF.GROUPS, nq, nk, WF.HEADS, WF.DH), (nq, nk)


def test_switch_on_the_images_follow_the_planes_under_the_launch_rule(lib):
    off = {f: time_ws(lib, f) for f in (16, 64, 65, 100, 256, 512, 1024)}
    assert lib.d4_train_attn_products_set(1) == 0
    for f, was in off.items():
        extra = 4 * images(LC.BATCH * LC.TOKENS, f, f, LC.HEADS, LC.DH) if f > 64 else 0
        assert time_ws(lib, f) == was + extra, f
    d = lambda f: time_ws(lib, 2 * f) - time_ws(lib, f)
    assert 0 < d(512) <= 2.05 * d(256)
    # space and cross: without wide frames nothing runs the tiled core, so nothing changes; with them, above 64 items only
    for tokens in (16, 64, 70):
        assert WF.space_ws(tokens) == WF.lds_space_ws(tokens)
    assert lib.d4_train_wide_set(1) == 0
    for tokens in (16, 64):
        assert WF.space_ws(tokens) == WF.lds_space_ws(tokens)
    for tokens in (65, 70, 256):
        want = WF.lds_space_ws(tokens) + 4 * (self_planes(WF.FRAMES, tokens, WF.HEADS, WF.DH) + images(WF.FRAMES, tokens, tokens, WF.HEADS, WF.DH))
        assert WF.space_ws(tokens) == want, tokens
    for nq, nk in ((1, 7), (64, 64)):
        assert WF.cross_ws(nq, nk) == WF.lds_cross_ws(nq, nk)
    for nq, nk in ((4, 256), (65, 3), (1, 65)):
        want = WF.lds_cross_ws(nq, nk) + 4 * (cross_planes(WF.GROUPS, nq, nk, WF.HEADS, WF.DH) + images(WF.GROUPS, nq, nk, WF.HEADS, WF.DH))
        assert WF.cross_ws(nq, nk) == want, (nq, nk)
    d = lambda n: WF.space_ws(2 * n) - WF.space_ws(n)
    assert 0 < d(512) <= 2.05 * d(256)
    d = lambda n: WF.cross_ws(4, 2 * n) - WF.cross_ws(4, n)
    assert 0 < d(512) <= 2.05 * d(256)
    # the operator entries' size queries answer whatever the switch says
    assert lib.d4_train_attn_core_bf16_plane_floats(3, 100, 2, 32) == self_planes(3, 100, 2, 32) + images(3, 100, 100, 2, 32)
    assert lib.d4_train_xattn_core_bf16_plane_floats(2, 4, 256, 3, 16) == cross_planes(2, 4, 256, 3, 16) + images(2, 4, 256, 3, 16)
    assert lib.d4_train_attn_core_plane_floats(300, 2, 32) == self_planes(3, 100, 2, 32)
