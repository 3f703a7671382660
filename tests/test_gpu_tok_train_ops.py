"""GPU: the pixel-side operators of the tokenizer's training forward (csrc/tok_train.hip), each called alone through its C entry point
(d4_flow_noised_patches, d4_layernorm_rows_bwd, d4_mask_rows_fwd / _bwd, d4_recon_loss_fwd_bwd) on the cases of tests/tok_train_cases.py.

A case asserts
  * the values: max |out - float64| <= BOUND[family] x max |float64| (tests/tok_train_ref.py; mask_rows_fwd and the masked half of its backward
    are copies: bit for bit);
  * untouched memory: every output sits between NaN guards, padded rows keep NaN gaps, and all of it is still NaN afterwards; operand gaps are NaN
    too, so a kernel that reads past a row poisons its output;
  * determinism: a second run into fresh buffers gives the same bits (the column sums and the loss sum have a fixed order: no float atomics).
flow_noised_patches with t = 1 is d4_video_patches bit for bit.  Patch rows that are no multiple of 4 floats and null pointers are refused.

Tolerance (tok_train_cases.py): E32 = float32 against float64 evaluation of the same reference on the CPU with sums added term after term, worst
case of the family, recorded with 25 % headroom; the GPU bound is 8 x E32 of the output's max-abs:
    family               measured E32   recorded E32   bound (8 x)
    flow_noised_patches  4.12e-8        5.2e-8         4.2e-7
    layernorm_rows_bwd   4.79e-6        6.0e-6         4.8e-5
    mask_rows_bwd        2.68e-7        3.4e-7         2.7e-6
    recon_loss           1.59e-6        2.0e-6         1.6e-5
The last test prints each family's worst error as a fraction of its bound."""
import ctypes as C
import math

import pytest
import torch

import tok_train_cases as TC
import tok_train_ref as R
from dreamer4_amd import _lib
from test_gpu_attn_cores import DEV, GUARD, Buf, bits, check_image

pytestmark = pytest.mark.gpu

WORST = {f: (0., '') for f in TC.BOUND}
ids = lambda table: [c['name'] for c in table]


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return _lib.load()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def note(family, name, err):
    print(f'{family} {name}: err {err:.3e} (bound {TC.BOUND[family]:.3e})')
    if err > WORST[family][0]:
        WORST[family] = (err, name)


def inp(x, ld=None):
    """x [..., w] (CPU fp32) as rows of leading dimension ld (default: dense) between NaN guards, gaps NaN"""
    x2 = x.reshape(-1, x.shape[-1]) if x.ndim > 1 else x.reshape(1, -1)
    rows, w = x2.shape
    ld = w if ld is None else ld
    b = Buf((rows - 1) * ld + w)
    b.view((rows, w), (ld, 1)).copy_(x2)
    return b.upload()


def out(size):
    return Buf(size).upload()


def image(buf, want, rows=None, w=None, ld=None):
    """the float64 image of an output buffer: NaN everywhere but where `want` must land"""
    img = torch.full((buf.host.numel(),), math.nan, dtype=torch.float64)
    if rows is None:
        img[GUARD:GUARD + want.numel()] = want.reshape(-1).double()
    else:
        img.as_strided((rows, w), (ld, 1), GUARD).copy_(want.reshape(rows, w).double())
    return img


def guards_intact(buf):
    got = buf.dev.cpu()
    assert got[:GUARD].isnan().all() and got[GUARD + buf.size:].isnan().all(), 'a scratch guard was written'


def twice(run):
    """run() -> tuple of output Bufs; the second run's bits must equal the first's"""
    a, b = run(), run()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(bits(x.dev), bits(y.dev)), 'two runs differ'
    return a


def geom_args(c):
    return (c['B'], c['C'], c['T'], c['nh'], c['nw'], c['ps'])


# ----------------------------------------------------------------------------- flow_noised_patches
@pytest.mark.parametrize('c', TC.FLOW_CASES, ids=ids(TC.FLOW_CASES))
def test_flow_noised_patches(lib, c):
    d = TC.geom_inputs(c)
    video, noise, times = inp(d['video'].reshape(1, -1)), inp(d['noise'].reshape(1, -1)), inp(d['times'])
    n = d['video'].numel()

    def run(t=times):
        o = out(n)
        _lib.check(lib.d4_flow_noised_patches(video.ptr, noise.ptr, t.ptr, o.ptr, *geom_args(c), stream()))
        return (o,)

    (o,) = twice(run)
    want = R.flow_noised_patches_ref(d['video'], d['noise'], d['times'], c['ps'])
    note('flow_noised_patches', c['name'], check_image(o.dev, image(o, want), TC.BOUND['flow_noised_patches']))
    # t = 1: the video's own patch rows, bit for bit what d4_video_patches writes; t = 0 (clip 0 above): the noise's
    (o1,) = run(inp(torch.ones(c['B'])))
    plain = out(n)
    _lib.check(lib.d4_video_patches(video.ptr, plain.ptr, *geom_args(c), 1, stream()))
    bare = out(n)                                                       # without noise: the video's own rows
    _lib.check(lib.d4_flow_noised_patches(video.ptr, None, None, bare.ptr, *geom_args(c), stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(o1.dev), bits(plain.dev)), 't = 1 is not video_to_patches bit for bit'
    assert torch.equal(bits(bare.dev), bits(plain.dev)), 'without noise: not video_to_patches bit for bit'
    per_clip = n // c['B']
    assert torch.equal(o.dev[GUARD:GUARD + per_clip].cpu(), R.patch_rows(d['noise'], c['ps'])[0].reshape(-1)), 't = 0 is not the noise itself'


# ----------------------------------------------------------------------------- layernorm_rows_bwd
@pytest.mark.parametrize('c', TC.LN_CASES, ids=ids(TC.LN_CASES))
def test_layernorm_rows_bwd(lib, c):
    d = TC.ln_inputs(c)
    rows, D, ld = c['rows'], c['D'], c['D'] + c['pad']
    x, dy, g = inp(d['x'], ld), inp(d['dy']), inp(d['g'])
    nparts = lib.d4_tok_rows_part_floats(rows, D)
    assert nparts == TC.part_floats(rows, D)

    def run():
        dx, dg, part = out((rows - 1) * ld + D), out(D), out(nparts)
        _lib.check(lib.d4_layernorm_rows_bwd(x.ptr, ld, dy.ptr, g.ptr, dx.ptr, dg.ptr, part.ptr, nparts, rows, D, TC.LN_EPS, stream()))
        return dx, dg, part

    dx, dg, part = twice(run)
    wdx, wdg = R.layernorm_rows_bwd_ref(d['x'], d['dy'], d['g'], TC.LN_EPS)
    b = TC.BOUND['layernorm_rows_bwd']
    err = max(check_image(dx.dev, image(dx, wdx, rows, D, ld), b), check_image(dg.dev, image(dg, wdg), b))
    guards_intact(part)
    note('layernorm_rows_bwd', c['name'], err)


# ----------------------------------------------------------------------------- mask rows
@pytest.mark.parametrize('c', TC.MASK_CASES, ids=ids(TC.MASK_CASES))
def test_mask_rows_forward_and_backward(lib, c):
    d = TC.mask_inputs(c)
    rows, D = c['rows'], c['D']
    x, dy, token = inp(d['x']), inp(d['dy']), inp(d['token'])
    mask = d['mask'].to(torch.uint8).to(DEV)
    mptr = C.c_void_p(mask.data_ptr())
    nparts = lib.d4_tok_rows_part_floats(rows, D)

    def run():
        y, dx, dt, part = out(rows * D), out(rows * D), out(D), out(nparts)
        _lib.check(lib.d4_mask_rows_fwd(x.ptr, mptr, token.ptr, y.ptr, rows, D, stream()))
        _lib.check(lib.d4_mask_rows_bwd(dy.ptr, mptr, dx.ptr, dt.ptr, part.ptr, nparts, rows, D, stream()))
        return y, dx, dt, part

    y, dx, dt, part = twice(run)
    check_image(y.dev, image(y, R.mask_rows_fwd_ref(d['x'], d['mask'], d['token'])), 0., scale=1.)                    # copies: exact
    wdx, wdt = R.mask_rows_bwd_ref(d['dy'], d['mask'])
    check_image(dx.dev, image(dx, wdx), 0., scale=1.)
    if d['mask'].any():
        note('mask_rows_bwd', c['name'], check_image(dt.dev, image(dt, wdt), TC.BOUND['mask_rows_bwd']))
    else:
        assert torch.equal(dt.dev[GUARD:GUARD + D].cpu(), torch.zeros(D)), 'no masked row: the mask token gets an exactly zero gradient'
        guards_intact(dt)
    guards_intact(part)


# ----------------------------------------------------------------------------- recon_loss_fwd_bwd
@pytest.mark.parametrize('c', TC.LOSS_CASES, ids=ids(TC.LOSS_CASES))
def test_recon_loss_fwd_bwd(lib, c):
    d = TC.geom_inputs(c)
    rows, video, noise, times = inp(d['recon_rows'].reshape(1, -1)), inp(d['video'].reshape(1, -1)), inp(d['noise'].reshape(1, -1)), inp(d['times'])
    n = d['video'].numel()
    # x-space reads neither the noise nor the times: null there
    nz, tm = (noise.ptr, times.ptr) if c['v_space'] else (None, None)

    def run():
        loss, d_rows, part = out(1), out(n), out(TC.LOSS_PARTS)
        _lib.check(lib.d4_recon_loss_fwd_bwd(rows.ptr, video.ptr, nz, tm, *geom_args(c), c['v_space'], loss.ptr, d_rows.ptr, part.ptr, TC.LOSS_PARTS, stream()))
        return loss, d_rows, part

    loss, d_rows, part = twice(run)
    wl, wd = R.recon_loss_ref(d['recon_rows'], d['video'], d['noise'], d['times'], c['ps'], c['v_space'])
    b = TC.BOUND['recon_loss']
    err = max(check_image(loss.dev, image(loss, wl.reshape(1)), b), check_image(d_rows.dev, image(d_rows, wd), b))
    guards_intact(part)
    note('recon_loss', c['name'], err)


# ----------------------------------------------------------------------------- refusals
def test_bad_sizes_and_null_pointers_are_refused(lib):
    buf = out(4096)
    p, null, s = buf.ptr, None, stream()
    for c in TC.REFUSED_GEOMS:                                          # patch rows of 3 and 1 floats: no float4 rows
        assert lib.d4_flow_noised_patches(p, p, p, p, *geom_args(c), s) != 0
        assert lib.d4_recon_loss_fwd_bwd(p, p, p, p, *geom_args(c), 1, p, p, p, TC.LOSS_PARTS, s) != 0
    ok = geom_args(TC.FLOW_CASES[-1])
    for args in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null), (p, null, null, null)):      # noise and t: together or not at all
        assert lib.d4_flow_noised_patches(*args, *ok, s) != 0
    assert lib.d4_recon_loss_fwd_bwd(null, p, p, p, *ok, 1, p, p, p, TC.LOSS_PARTS, s) != 0
    assert lib.d4_recon_loss_fwd_bwd(p, p, null, p, *ok, 1, p, p, p, TC.LOSS_PARTS, s) != 0, 'v-space needs the noise'
    assert lib.d4_recon_loss_fwd_bwd(p, p, p, p, *ok, 1, null, p, p, TC.LOSS_PARTS, s) != 0
    assert lib.d4_recon_loss_fwd_bwd(p, p, p, p, *ok, 1, p, p, p, TC.LOSS_PARTS - 1, s) != 0, 'scratch too small'
    assert lib.d4_layernorm_rows_bwd(p, 32, p, p, p, p, p, 32, 1, 30, 1e-5, s) != 0, 'dim no multiple of 4'
    assert lib.d4_layernorm_rows_bwd(p, 2048, p, p, p, p, p, 4096, 1, 2048, 1e-5, s) != 0, 'dim above 1024'
    assert lib.d4_layernorm_rows_bwd(p, 32, p, p, p, p, p, 31, 1, 32, 1e-5, s) != 0, 'scratch too small'
    assert lib.d4_layernorm_rows_bwd(p, 32, p, p, p, p, p, 32, 0, 32, 1e-5, s) != 0, 'no rows'
    assert lib.d4_layernorm_rows_bwd(p, 32, null, p, p, p, p, 32, 1, 32, 1e-5, s) != 0
    assert lib.d4_mask_rows_fwd(p, null, p, p, 1, 32, s) != 0 and lib.d4_mask_rows_fwd(p, p, p, p, 1, 30, s) != 0
    assert lib.d4_mask_rows_bwd(p, p, p, null, p, 32, 1, 32, s) != 0 and lib.d4_mask_rows_bwd(p, p, p, p, p, 16, 1, 32, s) != 0
    assert b'd4_mask_rows_bwd' in lib.d4_last_error()
    torch.cuda.synchronize()
    assert buf.dev.cpu().isnan().all(), 'a refused call wrote something'


def test_worst_error_of_every_family_as_a_fraction_of_its_bound():
    for f, (err, name) in WORST.items():
        print(f'{f}: worst error {err:.3e} = {err / TC.BOUND[f]:.3f} of the bound {TC.BOUND[f]:.3e} ({name})')
        assert name, f'no case of {f} ran'
        assert err <= TC.BOUND[f]
